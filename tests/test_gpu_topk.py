"""Top-k peaks on the MI355X (asx_xcorr_topk_f32_dev, Plan.xcorr_topk_f32, Plan.xcorr_topk_dev).

k = 1 must be, bit for bit, the strided call (no rows) or the windowed call (rows), counters included.  Every entry of larger k is
checked against tests/topk_model.py: the reference's max_abs_index over the window minus the zones around the earlier entries, on
the oracle's float64 results[], then the reference's wrap and Pearson coefficient."""
import math

import numpy as np
import pytest

import oracle
from topk_model import model
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
PRODUCTION = (144000, 288000, 480000, 720000, 960000, 1440000)


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def bits(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def counters(plan):
    return (plan.peak_overflows(), plan.peak_repairs()) + tuple(plan.pearson_modes())


def delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


def check_entries(got, want, what):
    """got: (lag[k], coef[k], ret[k]) of one pair; want: the model's k (ret, lag, coef)"""
    lag, coef, ret = got
    for j, (w_ret, w_lag, w_coef) in enumerate(want):
        assert (int(ret[j]), int(lag[j])) == (w_ret, w_lag), (what, j, [list(g) for g in got], want)
        if w_ret == 0:
            assert abs(float(coef[j]) - w_coef) < COEF_TOL, (what, j, float(coef[j]), w_coef)
        if w_ret in (-2, -3):
            assert math.isnan(float(coef[j])), (what, j)


def decoys(n, lags, gains, seed, noise=0.1):
    """noise; the sample a sum of copies of it at the given lags with falling gains"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n).astype(np.float32)
    i = np.arange(n)
    smp = noise * rng.standard_normal(n)
    for l, g in zip(lags, gains):
        smp = smp + g * src[(i + l % (2 * n)) % (2 * n)]
    return src, smp.astype(np.float32)


def short_overlap(n, true_lag, decoy_lag, seed):
    """The motivating case: the sample's tail is the source at a large negative lag (a short overlap), its head a weaker copy
    near lag 0 over a longer stretch -- a larger raw |r| with a lower coefficient"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n).astype(np.float32)
    i = np.arange(n)
    smp = np.empty(n)
    cut = -true_lag
    smp[:cut] = 0.5 * src[(i[:cut] + decoy_lag) % (2 * n)] + 0.3 * rng.standard_normal(cut)
    smp[cut:] = src[i[cut:] + true_lag] + 0.05 * rng.standard_normal(n - cut)
    return src, smp.astype(np.float32)


@pytest.mark.parametrize("layout,n", [("real-column", n) for n in PRODUCTION] + [("packed", 49000), ("packed", 144000)])
def test_k1_is_the_strided_and_the_windowed_call(mod, monkeypatch, layout, n):
    if layout == "packed" and n in PRODUCTION:
        monkeypatch.setenv("ASX_LAYOUT", "packed")
    pairs = [oracle.synth_pair(411, k, n, 1) for k in range(5)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    t = [p[2] for p in pairs]
    rows = np.array([(-n, n - 1), (-n // 3, n // 3), (n // 10, n // 2), (t[3], t[3]), (5, 4)], dtype=np.int64)
    with mod.Plan(n, 5, 0) as plan:
        assert plan.layout == layout, plan.layout
        for spectral in ((True, False) if layout == "real-column" else (False,)):
            plan.set_pearson(spectral)
            for window in (None, (-n // 3, n // 4)):
                if window:
                    plan.set_lag_window(*window)
                c0 = counters(plan)
                want = plan.xcorr_broadcast_f32(src, smp)
                c1 = counters(plan)
                got = plan.xcorr_topk_f32(src, smp, 1, 0)
                c2 = counters(plan)
                assert got[0].shape == (5, 1)
                assert bits(*(g[:, 0] for g in got)) == bits(*want), (spectral, window)
                assert delta(c0, c1) == delta(c1, c2), (c0, c1, c2)
                plan.set_lag_window(-n, n - 1)
            c0 = counters(plan)
            want = plan.xcorr_windowed_f32(src, smp, rows)
            c1 = counters(plan)
            got = plan.xcorr_topk_f32(src, smp, 1, 12345, rows)
            c2 = counters(plan)
            assert bits(*(g[:, 0] for g in got)) == bits(*want), spectral
            assert delta(c0, c1) == delta(c1, c2), (c0, c1, c2)
            assert int(want[2][4]) == -2


@pytest.mark.parametrize("layout,n", [("real-column", 144000), ("real-column", 480000), ("packed", 49000)])
def test_decoys_against_the_model(mod, layout, n):
    """copies at lags a, b, c with falling strength: k = 4 with a separation below their spacing gives a, b, c and then the noise
    floor; a separation above |a - b| skips b"""
    a, b, c = 5000, 20000, -12000
    src, smp = decoys(n, (a, b, c), (1.0, 0.7, 0.45), 9)
    r = oracle.cross_correlation(src.astype(np.float64), smp.astype(np.float64), want_results=True)[3]
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == layout
        for spectral in ((True, False) if layout == "real-column" else (False,)):
            plan.set_pearson(spectral)
            m0 = plan.pearson_modes()
            lag, coef, ret = plan.xcorr_topk_f32(np.stack([src, src]), np.stack([smp, smp]), 4, 1000)
            m1 = plan.pearson_modes()
            want = model(src, smp, 4, 1000, r=r)
            assert [w[1] for w in want[:3]] == [a, b, c], want
            for p in range(2):
                check_entries((lag[p], coef[p], ret[p]), want, (spectral, p))
            # under the spectral setting every entry of every pair is counted once (a call before it: m0); the direct one counts none
            assert sum(m1) - sum(m0) == (2 * 4 if spectral else 0), (spectral, m0, m1)
            sep = abs(a - b) + 1
            lag, coef, ret = plan.xcorr_topk_f32(src, smp, 3, sep)
            want = model(src, smp, 3, sep, r=r)
            assert want[1][1] == c and b not in [w[1] for w in want], want
            check_entries((lag[0], coef[0], ret[0]), want, (spectral, "skip b"))


def test_the_runner_up_is_the_true_offset(mod):
    """the argmax of r is a decoy near lag 0 with a long overlap and a low coefficient; the true offset, a large negative lag with a
    short overlap, is entry 1 with a coefficient >= 0.95 (MIN_CONFIDENCE)"""
    n = 144000
    true_lag, decoy_lag = -110000, 1000
    src, smp = short_overlap(n, true_lag, decoy_lag, 5)
    want = model(src, smp, 2, 200)
    assert [w[1] for w in want] == [decoy_lag, true_lag], want
    with mod.Plan(n, 1, 0) as plan:
        for spectral in (True, False):
            plan.set_pearson(spectral)
            lag, coef, ret = plan.xcorr_topk_f32(src, smp, 2, 200)
            check_entries((lag[0], coef[0], ret[0]), want, spectral)
            assert coef[0][1] >= 0.95 > coef[0][0], coef


def test_direct_form_is_the_windowed_call_at_each_lag(mod):
    """with the direct Pearson form, entry j's coefficient is bit for bit the windowed call's for the row [lag_j, lag_j]"""
    n = 144000
    src, smp = decoys(n, (3000, -40000, 60000), (1.0, 0.8, 0.6), 21)
    with mod.Plan(n, 4, 0) as plan:
        plan.set_pearson(False)
        lag, coef, ret = plan.xcorr_topk_f32(src, smp, 4, 500)
        rows = np.array([(int(l), int(l)) for l in lag[0]], dtype=np.int64)
        w_lag, w_coef, w_ret = plan.xcorr_windowed_f32(src, np.stack([smp] * 4), rows)
        assert bits(lag[0], coef[0], ret[0]) == bits(w_lag, w_coef, w_ret)


@pytest.mark.parametrize("layout,n", [("real-column", 144000), ("packed", 49000)])
def test_exhaustion_and_invalid_rows(mod, layout, n):
    pairs = [oracle.synth_pair(412, k, n, 1) for k in range(5)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    t = pairs[0][2]
    rows = np.array([(max(-n, t - 10), min(n - 1, t + 10)), (7, 3), (-n, n - 1), (-3, 2), (n - 1, -n)], dtype=np.int64)
    k, sep = 5, 4
    with mod.Plan(n, 5, 0) as plan:
        assert plan.layout == layout
        lag, coef, ret = plan.xcorr_topk_f32(src, smp, k, sep, rows)
        for p in (0, 2, 3):
            lo, hi = rows[p]
            check_entries((lag[p], coef[p], ret[p]), model(src[p], smp[p], k, sep, int(lo), int(hi)), p)
        assert ret[3].tolist()[2:] == [-3] * 3, ret                 # six lags, separation 4: two entries at most
        for p in (1, 4):
            assert ret[p].tolist() == [-2] * k and lag[p].tolist() == [0] * k and np.isnan(coef[p]).all(), (p, ret[p])
        # the other pairs' bits do not depend on the invalid rows
        fixed = rows.copy()
        fixed[1] = fixed[4] = (-n, n - 1)
        lag2, coef2, ret2 = plan.xcorr_topk_f32(src, smp, k, sep, fixed)
        for p in (0, 2, 3):
            assert bits(lag[p], coef[p], ret[p]) == bits(lag2[p], coef2[p], ret2[p]), p


def period8(n):
    base = np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32)
    return np.tile(base, 2 * n // 8)


def over_list(mod, plan):
    """the plan's list of overflowed pairs as it stands (device count, host mirror), read without emptying it"""
    return plan.debug_over_list()


def check_exact_and_async(mod, n, src, smp, k, sep, first_overflow, exact_r=None):
    """exact mode: the model, and one overflow and one repair per pair and call; asynchronous mode: ret = 1 from entry
    first_overflow on, the entries before it as the asynchronous strided call gives them, and nothing left on the overflow list.
    exact_r: r of each pair where the oracle's float64 transforms would round exact ties apart"""
    want = [model(s, t, k, sep, r=None if exact_r is None else exact_r[p]) for p, (s, t) in enumerate(zip(src, smp))]
    with mod.Plan(n, 2, 0) as plan:
        assert plan.peak_capacity < 2 * n
        c0 = (plan.peak_overflows(), plan.peak_repairs())
        lag, coef, ret = plan.xcorr_topk_f32(src, smp, k, sep)
        c1 = (plan.peak_overflows(), plan.peak_repairs())
        assert delta(c0, c1) == (len(src), len(src)), (c0, c1)
        for p in range(len(src)):
            check_entries((lag[p], coef[p], ret[p]), want[p], ("exact", p))
        assert over_list(mod, plan) == (0, 0)
        one = plan.xcorr_broadcast_f32(src, smp)                    # (exact: the first pass is clean when first_overflow > 0)
        plan.set_exact(False)
        c2 = (plan.peak_overflows(), plan.peak_repairs())
        alag, acoef, aret = plan.xcorr_topk_f32(src, smp, k, sep)
        # the asynchronous call counts, marks, and lists nothing: the list is read here, before anything could empty it
        assert over_list(mod, plan) == (0, 0)
        c3 = (plan.peak_overflows(), plan.peak_repairs())
        assert delta(c2, c3) == (len(src), 0), (c2, c3)
        for p in range(len(src)):
            assert aret[p].tolist() == [int(v) for v in ret[p][:first_overflow]] + [1] * (k - first_overflow), (p, aret[p])
            # (exact mode's second look recomputed these entries with the direct form: the same lags)
            assert alag[p][:first_overflow].tolist() == lag[p][:first_overflow].tolist(), p
            if first_overflow:
                assert bits(alag[p][0], acoef[p][0], aret[p][0]) == bits(*(o[p] for o in one)), p


def test_overflow_in_the_first_pass(mod):
    """the period-8 pair of test_gpu_exact_peak.py: 2N/8 exact ties already in pass 1"""
    n = 48000
    per = period8(n)
    check_exact_and_async(mod, n, np.stack([per]), np.stack([per[:n]]), 3, 3, first_overflow=0)


def spike_run_ties(n, m2, pos, sign):
    """r = the source (the sample is a unit impulse at frame 0): the period-8 pattern (2N/4 exact ties at |r| = 3) everywhere but a
    spike at index pos and, right behind it, a run of 4 M2 + 8 distinct, strictly falling values from 100 down to 10.  The run
    holds every column of the transform matrix in both layouts at least twice, so every column tile of pass 1 has a clear maximum
    of its own and lists no tie; a separation that covers the run leaves pass 2 nothing but the ties."""
    src = period8(n)
    run = 4 * m2 + 8
    src[pos] = sign * 1000.0
    src[pos + 1:pos + 1 + run] = sign * np.linspace(100.0, 10.0, run, dtype=np.float32)
    assert len(np.unique(src[pos + 1:pos + 1 + run])) == run
    return src, run


@pytest.mark.parametrize("layout,n", [("packed", 48000), ("real-column", 144000)])
def test_overflow_in_the_second_pass_only(mod, layout, n):
    """pass 1 is clean, pass 2 overflows: the pair is counted, listed and looked at again once, the exact entries are the
    model's; in the asynchronous mode entry 0 is the strided call's, bit for bit, and entries 1.. are marked"""
    with mod.Plan(n, 1, 0) as probe:
        assert probe.layout == layout
        m2 = probe.split[1]
    a, run = spike_run_ties(n, m2, n // 2, 1.0)                     # lag N/2
    b, _ = spike_run_ties(n, m2, 2 * n - n // 2, -1.0)              # lag -N/2, its run towards lag -1
    src = np.stack([a, b])
    smp = np.zeros((2, n), np.float32)
    smp[:, 0] = 1.0
    sep = run + 2
    # r[l] = source[l] exactly (one product per lag): the exact values the device re-evaluates, ties included
    check_exact_and_async(mod, n, src, smp, 3, sep, first_overflow=1, exact_r=src.astype(np.float64))


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_groups_lanes_and_broadcast(mod, monkeypatch, lanes):
    """a batch over several launch groups (one and two lanes) gives each pair what it gets alone; one source broadcast to every
    pair (stride 0) gives the materialised batch's bits"""
    monkeypatch.setenv("ASX_WS_MB", "24")
    monkeypatch.setenv("ASX_LANES", lanes)
    n = 144000
    B = 13
    src0, _ = decoys(n, (0,), (1.0,), 31)
    rng = np.random.default_rng(32)
    lags = rng.integers(-n + 1, n - 1, (B, 3))
    smp = np.stack([decoys(n, tuple(int(v) for v in lags[p]), (1.0, 0.7, 0.5), 31)[1] for p in range(B)])
    src = np.stack([src0] * B)
    with mod.Plan(n, B, 0) as plan:
        assert plan.group < B
        for spectral in (True, False):
            plan.set_pearson(spectral)
            full = plan.xcorr_topk_f32(src, smp, 3, 2000)
            bc = plan.xcorr_topk_f32(src0, smp, 3, 2000)
            assert bits(*full) == bits(*bc), spectral
            for p in (0, 6, 12):
                alone = plan.xcorr_topk_f32(src0, smp[p], 3, 2000)
                assert bits(*(g[p] for g in full)) == bits(*(g[0] for g in alone)), (spectral, p)


def test_bad_arguments_return_minus_one_with_outputs_untouched(mod):
    import torch
    n = 144000
    s, t, _ = oracle.synth_pair(5, 5, n, 1)
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column"
        d_src = torch.from_numpy(np.stack([s, s])).cuda()
        d_smp = torch.from_numpy(np.stack([t, t])).cuda()
        d_win = torch.tensor([[-n, n - 1]] * 2, dtype=torch.int64, device="cuda")
        d_lag = torch.full((16,), -99, dtype=torch.int64, device="cuda")
        d_coef = torch.full((16,), 7.5, dtype=torch.float64, device="cuda")
        d_ret = torch.full((16,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        src_p, smp_p = d_src.data_ptr(), d_smp.data_ptr()
        bad = [
            dict(k=0), dict(k=9), dict(k=-1), dict(sep=-1), dict(coef=0), dict(ret=0),
            dict(src=src_p + 4), dict(ss=2 * n + 2),            # the real-column layout rule
        ]
        for b in bad:
            with pytest.raises(mod.AsxError):
                plan.xcorr_topk_dev(b.get("src", src_p), b.get("ss", 2 * n), smp_p, n, d_win.data_ptr(), 1, 2, b.get("k", 4),
                                    b.get("sep", 10), d_lag.data_ptr(), b.get("coef", d_coef.data_ptr()),
                                    b.get("ret", d_ret.data_ptr()))
        plan.sync()
        torch.cuda.synchronize()
        assert (d_lag == -99).all() and (d_coef == 7.5).all() and (d_ret == 9).all()
        # and a good call with d_lag = NULL writes coef and ret only, k entries per pair
        plan.xcorr_topk_dev(src_p, 2 * n, smp_p, n, 0, 0, 2, 4, 10, 0, d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
        torch.cuda.synchronize()
        assert (d_lag == -99).all() and (d_ret[:8] == 0).all() and (d_ret[8:] == 9).all() and (d_coef[8:] == 7.5).all()


def test_plan_window_is_honoured_and_left_alone(mod):
    n = 144000
    src, smp = decoys(n, (5000, 20000, -12000), (1.0, 0.7, 0.45), 9)
    r = oracle.cross_correlation(src.astype(np.float64), smp.astype(np.float64), want_results=True)[3]
    with mod.Plan(n, 1, 0) as plan:
        plan.set_lag_window(-15000, 15000)
        lag, coef, ret = plan.xcorr_topk_f32(src, smp, 3, 1000)
        check_entries((lag[0], coef[0], ret[0]), model(src, smp, 3, 1000, -15000, 15000, r=r), "plan window")
        lag, coef, ret = plan.xcorr_topk_f32(src, smp, 3, 1000, (10000, 30000))
        check_entries((lag[0], coef[0], ret[0]), model(src, smp, 3, 1000, 10000, 30000, r=r), "rows")
        assert plan.lag_window == (-15000, 15000)
