"""Per-pair lag windows on the MI355X (asx_xcorr_windowed_f32_dev, Plan.xcorr_windowed_f32, Plan.xcorr_windows_f32(positions=)).

A valid row must give, bit for bit, what the strided call gives for that pair alone on the same plan with the plan window set to
the row; an invalid row gives (0, NaN, -2) and leaves every other pair's bits alone.  The windowed answers themselves are checked
against tests/lag_window_model.py (the reference's rule over the oracle's float64 results[])."""
import numpy as np
import pytest

import oracle
from lag_window_model import model
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
PRODUCTION = (144000, 288000, 480000, 720000, 960000, 1440000)


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    return t


def check(got, want, what):
    lag, coef, ret = got
    w_ret, w_lag, w_coef = want
    assert (int(ret), int(lag)) == (w_ret, w_lag), (what, got, want)
    if w_ret == 0:
        assert abs(float(coef) - w_coef) < COEF_TOL, (what, got, want)


def pair_bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


def alone(plan, src, smp, lo, hi):
    """the pair alone through the strided path with the plan window set to its row; the plan's window restored after"""
    keep = plan.lag_window
    plan.set_lag_window(lo, hi)
    try:
        return plan.xcorr_broadcast_f32(src, smp[None, :])
    finally:
        plan.set_lag_window(*keep)


def decoy_pair(n, a, b, seed):
    """noise; the sample a strong copy of it at lag a plus a weaker copy at lag b (as tests/test_gpu_lag_window.py)"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n).astype(np.float32)
    i = np.arange(n)
    ka, kb = a % (2 * n), b % (2 * n)
    smp = (src[(i + ka) % (2 * n)] + 0.6 * src[(i + kb) % (2 * n)] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return src, smp


def mixed_rows(n, true_lags):
    """full, holds lag 0, positive only, negative only (seed != 0), one lag at the true peak, one lag elsewhere, a tight row"""
    t = true_lags
    return np.array([(-n, n - 1), (-n // 3, n // 3), (n // 10, n // 2), (-n // 2, -n // 10), (t[4], t[4]), (n // 7, n // 7),
                     (max(-n, t[6] - 5), min(n - 1, t[6] + 5))], dtype=np.int64)


@pytest.mark.parametrize("layout,n", [("real-column", n) for n in PRODUCTION] + [("packed", 49000), ("packed", 144000)])
def test_each_pair_equals_the_pair_alone_with_the_plan_window(mod, monkeypatch, layout, n):
    if layout == "packed" and n in PRODUCTION:
        monkeypatch.setenv("ASX_LAYOUT", "packed")
    pairs = [oracle.synth_pair(301, k, n, 1) for k in range(7)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    rows = mixed_rows(n, [p[2] for p in pairs])
    with mod.Plan(n, 7, 0) as plan:
        assert plan.layout == layout, plan.layout
        for spectral in ((True, False) if layout == "real-column" else (False,)):
            plan.set_pearson(spectral)
            got = plan.xcorr_windowed_f32(src, smp, rows)
            for k in range(7):
                want = alone(plan, src[k], smp[k], *rows[k])
                assert pair_bits(got, k) == pair_bits(want, 0), (spectral, k, rows[k], [g[k] for g in got], want)
            assert got[2].tolist() == [0] * 7, got
            assert int(got[0][4]) == rows[4][0] and int(got[0][5]) == rows[5][0]


@pytest.mark.parametrize("n", [144000, 480000])
def test_full_rows_and_one_shared_row(mod, torch, n):
    """every row full: the bits of the strided call without a window; window_stride 0: the strided call with the plan window"""
    pairs = [oracle.synth_pair(302, k, n, 1) for k in range(5)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    with mod.Plan(n, 5, 0) as plan:
        for spectral in (True, False):
            plan.set_pearson(spectral)
            want = plan.xcorr_broadcast_f32(src, smp)
            full = np.array([(-n, n - 1)] * 5, dtype=np.int64)
            assert [a.tobytes() for a in plan.xcorr_windowed_f32(src, smp, full)] == [a.tobytes() for a in want]
            row = (-n // 5, n // 9)
            got = plan.xcorr_windowed_f32(src, smp, row)       # a 1-D row: window_stride 0
            plan.set_lag_window(*row)
            want = plan.xcorr_broadcast_f32(src, smp)
            plan.set_lag_window(-n, n - 1)
            assert [a.tobytes() for a in got] == [a.tobytes() for a in want]


def test_against_the_float64_model_with_decoys(mod):
    """the decoy wins in some rows and the true peak in others, all in one batch"""
    n = 144000
    cases = [  # (a = the strong copy, b = the weaker one, row)
        (5000, 20000, (10000, 30000)), (5000, 20000, (-n, n - 1)), (5000, 20000, (0, 10000)),
        (-5000, -20000, (-30000, -10000)), (-5000, -20000, (-9000, 0)),
        (30000, -3000, (-10000, 10000)), (30000, -3000, (20000, 40000)), (30000, -3000, (-3000, -3000)),
    ]
    src = np.empty((len(cases), 2 * n), np.float32)
    smp = np.empty((len(cases), n), np.float32)
    for k, (a, b, _) in enumerate(cases):
        src[k], smp[k] = decoy_pair(n, a, b, 40 + k)
    rows = np.array([c[2] for c in cases], dtype=np.int64)
    with mod.Plan(n, len(cases), 0) as plan:
        for spectral in (True, False):
            plan.set_pearson(spectral)
            lag, coef, ret = plan.xcorr_windowed_f32(src, smp, rows)
            winners = set()
            for k, (a, b, (lo, hi)) in enumerate(cases):
                want = model(src[k], smp[k], lo, hi)
                check((lag[k], coef[k], ret[k]), want, (spectral, k))
                winners.add("decoy" if want[1] == b else "true" if want[1] == a else "other")
            assert {"decoy", "true"} <= winners, winners


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_several_launch_groups(mod, monkeypatch, lanes):
    """a batch over several groups (and two lanes): every group must read its own pairs' rows"""
    monkeypatch.setenv("ASX_WS_MB", "24")
    monkeypatch.setenv("ASX_LANES", lanes)
    n, b = 144000, 9
    pairs = [oracle.synth_pair(303, k, n, 1) for k in range(b)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    # rows that differ from pair to pair: half of them exclude the true lag, so a row read for the wrong pair shows
    rows = []
    for k, (_, _, t) in enumerate(pairs):
        if k % 2:
            rows.append((max(-n, t - 40 - k), min(n - 1, t + 3 * k)))
        else:
            lo = t + 1000 + 37 * k if t < n // 2 else t - 30000
            rows.append((min(lo, n - 1), min(lo + 20000, n - 1)))
    rows = np.array(rows, dtype=np.int64)
    with mod.Plan(n, b, 0) as plan:
        assert plan.group < b, plan.group
        got = plan.xcorr_windowed_f32(src, smp, rows)
        for k in range(b):
            assert pair_bits(got, k) == pair_bits(alone(plan, src[k], smp[k], *rows[k]), 0), (k, rows[k])
            if k % 2:
                assert int(got[0][k]) == pairs[k][2]
            check((got[0][k], got[1][k], got[2][k]), model(src[k], smp[k], *rows[k]), k)


def periodic_inputs(n):
    """tests/test_gpu_lag_window.py::test_exact_under_the_window: exactly tied peaks every 8 lags"""
    base = np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32)
    per = np.tile(base, 2 * n // 8)
    r8 = np.array([np.dot(np.roll(base, -k).astype(np.float64), base.astype(np.float64)) for k in range(8)]) * (n // 8)
    return per, per[:n].copy(), r8[np.arange(2 * n) % 8]


def counters(plan):
    return plan.peak_overflows(), plan.peak_repairs()


def test_overflowing_pairs(mod, torch):
    n = 48000
    per, psmp, r = periodic_inputs(n)
    lo, hi = 1003, 40000
    want = model(per, psmp, lo, hi, r=r)
    assert want[1] == 1008
    other_src, other_smp, other_lag = oracle.synth_pair(304, 0, n, 1)
    src = np.stack([per, other_src, per, other_src])
    smp = np.stack([psmp, other_smp, psmp, other_smp])
    rows = np.array([(lo, hi), (-n, n - 1), (-20000, -2001), (other_lag - 3, other_lag + 3)], dtype=np.int64)
    with mod.Plan(n, 4, 0) as plan:
        assert (hi - lo) // 8 > plan.peak_capacity
        # alone, then beside other pairs: the second look runs with the pair's own row
        c0 = counters(plan)
        got1 = plan.xcorr_windowed_f32(per, psmp, rows[0])
        check((got1[0][0], got1[1][0], got1[2][0]), want, "alone")
        c1 = counters(plan)
        assert c1[0] > c0[0] and c1[1] > c0[1]
        per_pair = [alone(plan, src[k], smp[k], *rows[k]) for k in range(4)]
        c2 = counters(plan)
        got = plan.xcorr_windowed_f32(src, smp, rows)
        c3 = counters(plan)
        assert (c3[0] - c2[0], c3[1] - c2[1]) == (c2[0] - c1[0], c2[1] - c1[1]), (c1, c2, c3)
        for k in range(4):
            assert pair_bits(got, k) == pair_bits(per_pair[k], 0), k
        check((got[0][0], got[1][0], got[2][0]), want, "exact")
        check((got[0][2], got[1][2], got[2][2]), model(per, psmp, -20000, -2001, r=r), "exact, negative row")
        # the asynchronous mode: the overflowing pairs come back with ret = 1, inside their rows
        d_src = torch.from_numpy(src).cuda()
        d_smp = torch.from_numpy(smp).cuda()
        d_rows = torch.from_numpy(rows).cuda()
        d_lag = torch.full((4,), -99, dtype=torch.int64, device="cuda")
        d_coef = torch.zeros(4, dtype=torch.float64, device="cuda")
        d_ret = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.set_exact(False)
        try:
            plan.xcorr_windowed_dev(d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, d_rows.data_ptr(), 1, 4, d_lag.data_ptr(),
                                    d_coef.data_ptr(), d_ret.data_ptr())
            plan.sync()
        finally:
            plan.set_exact(True)
        ret, lag = d_ret.cpu().numpy(), d_lag.cpu().numpy()
        assert ret[0] == 1 and lo <= lag[0] <= hi and ret[2] == 1 and -20000 <= lag[2] <= -2001, (ret, lag)
        assert ret[1] == 0 and ret[3] == 0 and lag[1] == lag[3] == other_lag, (ret, lag)


def test_invalid_and_empty_rows(mod, torch):
    n = 144000
    pairs = [oracle.synth_pair(305, k, n, 1) for k in range(6)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    good = np.array([(-n, n - 1), (-n // 4, n // 4), (n // 10, n // 2), (-n // 2, -1), (-n, n - 1), (pairs[5][2], pairs[5][2])],
                    dtype=np.int64)
    bad_rows = [(5, 4), (-n - 1, 0), (0, n), (-n - 5, n + 5), (2 ** 40, 2 ** 40 + 1), (-2 ** 62, -2 ** 62)]
    with mod.Plan(n, 6, 0) as plan:
        for spectral in (True, False):
            plan.set_pearson(spectral)
            modes0, c0 = plan.pearson_modes(), counters(plan)
            ref = plan.xcorr_windowed_f32(src, smp, good)
            modes1, c1 = plan.pearson_modes(), counters(plan)
            for j, bad in enumerate(bad_rows):
                rows = good.copy()
                k = 1 + j % 4                       # a pair in the middle of the batch
                rows[k] = bad
                got = plan.xcorr_windowed_f32(src, smp, rows)
                assert int(got[0][k]) == 0 and np.isnan(got[1][k]) and int(got[2][k]) == -2, (bad, [g[k] for g in got])
                for i in range(6):
                    if i != k:
                        assert pair_bits(got, i) == pair_bits(ref, i), (bad, i)
                assert counters(plan) == c1 == c0, (bad, counters(plan), c0)
            # the Pearson-mode counter counts an invalid pair once, as a direct reduction (ASX_PM_DIRECT)
            modes2 = plan.pearson_modes()
            rows = good.copy()
            rows[2] = (1, 0)
            plan.xcorr_windowed_f32(src, smp, rows)
            modes3 = plan.pearson_modes()
            d_ref = np.subtract(modes1, modes0)
            d_bad = np.subtract(modes3, modes2)
            if spectral:
                assert d_bad.sum() == d_ref.sum() == 6, (d_ref, d_bad)
                plan.xcorr_windowed_f32(src[2], smp[2], good[2])       # what pair 2 counts when its row is valid
                d_two = np.subtract(plan.pearson_modes(), modes3)
                assert (d_bad - (d_ref - d_two)).tolist() == [0, 0, 1], (d_ref, d_bad, d_two)
            else:
                assert d_bad.sum() == d_ref.sum() == 0, (d_ref, d_bad)   # the direct form counts no modes
        # a whole batch of invalid rows
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, (3, 2))
        assert lag.tolist() == [0] * 6 and np.isnan(coef).all() and ret.tolist() == [-2] * 6


def test_plan_window_is_ignored_and_intact(mod):
    n = 144000
    src, smp = decoy_pair(n, 5000, 20000, 7)
    with mod.Plan(n, 1, 0) as plan:
        full = plan.xcorr_windowed_f32(src, smp, (-n, n - 1))
        plan.set_lag_window(10000, 30000)                  # holds the decoy only
        got = plan.xcorr_windowed_f32(src, smp, (-n, n - 1))
        assert [a.tobytes() for a in got] == [a.tobytes() for a in full]
        assert int(got[0][0]) == 5000
        assert plan.lag_window == (10000, 30000)
        lag, coef, ret = plan.xcorr_broadcast_f32(src, smp[None, :])
        assert int(lag[0]) == 20000 and int(ret[0]) == 0


def test_windows_with_positions(mod):
    """a clip planted in a long recording, a louder copy of it outside the range of positions"""
    n, hop = 144000, 36000
    rng = np.random.default_rng(17)
    rec = (0.5 * rng.standard_normal(2 * n + hop * 11)).astype(np.float32)
    clip = rng.standard_normal(n).astype(np.float32)
    at, loud_at = 250000, 40000
    rec[at:at + n] += clip
    rec[loud_at:loud_at + n] += 3.0 * clip
    with mod.Plan(n, 12, 0) as plan:
        plain = plan.xcorr_windows_f32(rec, clip, hop)
        assert [a.tobytes() for a in plan.xcorr_windows_f32(rec, clip, hop, positions=None)] == [a.tobytes() for a in plain]
        p_lo, p_hi = 200000, 300000
        lag, coef, ret = plan.xcorr_windows_f32(rec, clip, hop, positions=(p_lo, p_hi))
        batch = (rec.size - 2 * n) // hop + 1
        assert lag.shape == (batch,)
        from audiosync_amd.hipxcorr import position_rows
        k0, k1, rows = position_rows(n, hop, batch, p_lo, p_hi)
        assert 0 < k1 - k0 < batch
        for k in range(batch):
            if k0 <= k < k1:
                assert ret[k] == 0 and rows[k - k0][0] <= lag[k] <= rows[k - k0][1], (k, lag[k], ret[k])
            else:
                assert (lag[k], ret[k]) == (0, -2) and np.isnan(coef[k]), k
        best = k0 + int(np.argmax(np.abs(coef[k0:k1])))
        assert best * hop + int(lag[best]) == at, (best, lag[best])
        # without positions the louder copy wins
        pb = int(np.argmax(np.where(plain[2] == 0, np.abs(plain[1]), -1)))
        assert pb * hop + int(plain[0][pb]) == loud_at


def test_argument_checks(mod, torch):
    n = 144000
    src, smp, _ = oracle.synth_pair(306, 0, n, 1)
    d_src = torch.from_numpy(src).cuda()
    d_smp = torch.from_numpy(smp).cuda()
    d_rows = torch.tensor([[-n, n - 1]], dtype=torch.int64, device="cuda")
    d_lag = torch.full((1,), -99, dtype=torch.int64, device="cuda")
    d_coef = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    d_ret = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "real-column"
        calls = [
            (d_src.data_ptr(), 0, d_smp.data_ptr(), 0, 0, 1, 1, d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr()),  # no windows
            (d_src.data_ptr(), 0, d_smp.data_ptr(), 0, d_rows.data_ptr(), 1, 1, d_lag.data_ptr(), d_coef.data_ptr(), 0),  # no ret
            (d_src.data_ptr(), 0, d_smp.data_ptr(), 0, d_rows.data_ptr(), 1, 1, d_lag.data_ptr(), 0, d_ret.data_ptr()),   # no coef
            (d_src.data_ptr(), 6, d_smp.data_ptr(), 0, d_rows.data_ptr(), 1, 1, d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr()),
            (d_src.data_ptr() + 4, 0, d_smp.data_ptr(), 0, d_rows.data_ptr(), 1, 1, d_lag.data_ptr(), d_coef.data_ptr(),
             d_ret.data_ptr()),
        ]
        for args in calls:
            with pytest.raises(mod.AsxError):
                plan.xcorr_windowed_dev(*args)
            plan.sync()
            assert (int(d_lag[0]), float(d_coef[0]), int(d_ret[0])) == (-99, 5.0, 7), args
        # d_lag may be NULL
        plan.xcorr_windowed_dev(d_src.data_ptr(), 0, d_smp.data_ptr(), 0, d_rows.data_ptr(), 1, 1, 0, d_coef.data_ptr(),
                                d_ret.data_ptr())
        plan.sync()
        assert int(d_ret[0]) == 0 and int(d_lag[0]) == -99
