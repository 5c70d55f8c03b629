"""GCC-PHAT over track pools on the MI355X (asx_xcorr_pool_phat_f32_dev, Plan.xcorr_pool_phat_f32, Plan.xcorr_pool_phat_dev).

Every pair whose indices lie inside their pools must give, bit for bit, what the banded strided PHAT call gives for that pair alone
on the same plan with the same band and window: no tolerance is involved.  An index outside its pool gives (0, NaN, NaN, -4) and
leaves the other pairs alone.  The planted pairs are also checked against the float64 model of tests/phat_band_model.py.  Lengths:
the smallest of each row form (480-point rows, 1200 in one piece, the two-half form)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import phat_band_model
from test_gpu_pool import shifted
from util import ROOT, asx

pytestmark = pytest.mark.gpu

LENGTHS = [144000, 480000, 960000]
CURVE_TOL = 3e-6   # test_gpu_phat_band.py: four times the worst error of the banded curve against the float64 model
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    assert t.cuda.is_available()
    return t


def bits(out, k):
    return [np.asarray(a).reshape(-1)[k].tobytes() for a in out]


def all_bits(out):
    return [np.asarray(a).tobytes() for a in out]


def alone(plan, src, smp, band, windows=None):
    """the pair alone through the banded strided PHAT call (asx_xcorr_phat_band_f32_dev, one pair)"""
    return plan.xcorr_phat_f32(src, smp[None, :], windows, band=band)


def is_refused(out, i, code):
    lag, coef, peak, ret = (np.asarray(a).reshape(-1)[i] for a in out)
    return (int(lag), int(ret)) == (0, code) and np.isnan(coef) and np.isnan(peak)


def outputs(torch, b):
    return (torch.full((b,), -99, dtype=torch.int64, device="cuda"), torch.full((b,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((b,), 7.0, dtype=torch.float64, device="cuda"), torch.full((b,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    b = out[0].numel()
    return [a.cpu().tolist() for a in out] == [[-99] * b, [7.0] * b, [7.0] * b, [7] * b]


def pool_dev(plan, torch, d_src, ss, ns, d_smp, ms, nm, pairs, batch, band, windows=None, ws=0, skip=()):
    """the raw call on device pools; skip: the outputs (0 lag, 2 peak) passed as NULL, which come back as the sentinels"""
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda() if pairs is not None else None
    d_win = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.int64)).cuda() if windows is not None else None
    out = outputs(torch, batch)
    torch.cuda.synchronize()
    plan.xcorr_pool_phat_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ms, nm, d_pairs.data_ptr() if d_pairs is not None else 0,
                             d_win.data_ptr() if d_win is not None else 0, ws, batch, band[0], band[1],
                             *(0 if k in skip else a.data_ptr() for k, a in enumerate(out)))
    plan.sync()
    return tuple(a.cpu().numpy() for a in out)


@pytest.mark.parametrize("n", LENGTHS)
def test_small_matrix_at_every_length(mod, n):
    """3 sources x 2 samples, d_pairs NULL: planted lags of both signs (noise 0.1), the rest unrelated; every pair equals the pair
    alone under the full band, [1, N/6] and [N - 1, N].  The planted pairs against the float64 model: the peak height within
    CURVE_TOL under every band, and the planted lag under every band in which the model's own peak is the planted lag.  Under
    [N - 1, N] it is not: three bins vote, the curve is a cosine of magnitude near 1 at every other lag, and no lag stands out in
    float64 either -- there the bit equality and the peak height are what is checked."""
    rng = np.random.default_rng(n % 1000 + 5)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    l0, l1 = n // 3 + 17, -(n // 5) - 3
    smp = np.stack([shifted(src[0], l0, rng), shifted(src[2], l1, rng)])
    bands = [(0, n), (1, n // 6), (n - 1, n)]
    planted = {(0, 0): l0, (2, 1): l1}
    models = {}
    for (a, b), lag in planted.items():
        s, t = src[a].astype(np.float64), smp[b].astype(np.float64)
        q = np.fft.rfft(s) * np.conj(np.fft.rfft(t, 2 * n))
        mag = np.abs(q)
        unit = np.divide(q, mag, out=np.zeros_like(q), where=mag > 0)
        for lo, hi in bands:
            u = unit.copy()
            u[:lo] = 0.0
            u[hi + 1:] = 0.0
            r = np.fft.irfft(u, 2 * n) * (2.0 * n / phat_band_model.votes(n, lo, hi))
            models[a, b, lo, hi] = phat_band_model.model(s, t, lo, hi, r=r)
        # the bands that are meant to find the lag do find it in float64
        assert models[a, b, 0, n][1] == lag and models[a, b, 1, n // 6][1] == lag, (n, a, b, models)
    with mod.Plan(n, 8, 0) as plan:
        assert plan.layout == "real-column"
        for band in bands:
            fills = plan.debug_bank()[2]
            got = plan.xcorr_pool_phat_f32(src, smp, band=band)
            assert plan.debug_bank()[:2] == (3, 2) and plan.debug_bank()[2] == fills + 1
            assert all(a.shape == (3, 2) for a in got) and [a.dtype for a in got] == [np.int64, np.float64, np.float64, np.int32]
            for a in range(3):
                for b in range(2):
                    assert bits(got, 2 * a + b) == bits(alone(plan, src[a], smp[b], band), 0), (n, band, a, b)
            for (a, b), lag in planted.items():
                m = models[(a, b) + band]
                print("pool phat n", n, "band", band, "pair", (a, b), "lag", int(got[0][a, b]), "planted", lag, "model", m,
                      "peak", float(got[2][a, b]), "diff", abs(float(got[2][a, b]) - m[3]))
                assert abs(float(got[2][a, b]) - m[3]) <= CURVE_TOL, (n, band, a, b, got[2][a, b], m)
                if m[1] == lag:
                    assert (int(got[3][a, b]), int(got[0][a, b])) == (0, lag), (n, band, a, b, got[0][a, b])
        assert all_bits(plan.xcorr_pool_phat_f32(src, smp)) == all_bits(plan.xcorr_pool_phat_f32(src, smp, band=(0, n)))


@pytest.mark.parametrize("band", ["full", "low"])
def test_listed_pairs_in_several_groups(mod, torch, band):
    """a plan of four pairs a group and 11 listed pairs, two full groups and a partial one, with repeats and out of order; one pool as
    both pools, the tracks windows of one recording (a stride below 2N): a window against the first N frames of another peaks at the
    distance between them"""
    n, hop, nwin = 144000, 36000, 6
    band = (0, n) if band == "full" else (1, n // 6)
    rec = np.random.default_rng(17).standard_normal(2 * n + (nwin - 1) * hop).astype(np.float32)
    pairs = np.array([[3, 1], [0, 0], [0, 0], [5, 2], [1, 3], [2, 2], [4, 2], [0, 3], [5, 5], [2, 1], [3, 1]], dtype=np.int32)
    assert all(-n < (b - a) * hop <= n for a, b in pairs)     # the lags at which the two windows overlap
    d_rec = torch.from_numpy(rec).cuda()
    with mod.Plan(n, 4, 0) as plan:
        assert plan.group == 4
        fills = plan.debug_bank()[2]
        got = pool_dev(plan, torch, d_rec, hop, nwin, d_rec, hop, nwin, pairs, len(pairs), band)
        assert plan.debug_bank() == (nwin, nwin, fills + 1)
        for i, (a, b) in enumerate(pairs):
            assert bits(got, i) == bits(alone(plan, rec[a * hop:a * hop + 2 * n], rec[b * hop:b * hop + n], band), 0), (i, a, b)
            assert (int(got[0][i]), int(got[3][i])) == ((b - a) * hop, 0), (i, a, b, got[0][i])
        assert bits(got, 1) == bits(got, 2) and bits(got, 0) == bits(got, 10)


def test_windows(mod):
    """per-pair rows (window_stride 1) with a full row, a one-lag row and a row that is not a window; one row for every pair
    (window_stride 0); the plan's own window with d_windows NULL"""
    n = 144000
    band = (300, n // 4)
    rng = np.random.default_rng(23)
    src = rng.standard_normal((2, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], 5000, rng) + 0.6 * shifted(src[0], -9000, rng), shifted(src[1], -777, rng)])
    pairs = np.array([[0, 0], [0, 0], [1, 1], [0, 1], [1, 1], [0, 0]], dtype=np.int32)
    rows = np.array([[-n, n - 1], [-20000, -1000], [-800, -700], [3, 2], [10, 10], [4000, 6000]], dtype=np.int64)   # row 3: not a window
    with mod.Plan(n, 4, 0) as plan:
        got = plan.xcorr_pool_phat_f32(src, smp, pairs, rows, band)
        for i, (a, b) in enumerate(pairs):
            assert bits(got, i) == bits(alone(plan, src[a], smp[b], band, rows[i]), 0), (i, rows[i])
        assert is_refused(got, 3, -2), got
        assert [int(got[0][i]) for i in (0, 1, 2, 4, 5)] == [5000, -9000, -777, 10, 5000], got[0]
        assert bits(got, 0) == bits(plan.xcorr_pool_phat_f32(src, smp, pairs[:1], band=band), 0)   # a full row is no window
        got = plan.xcorr_pool_phat_f32(src, smp, pairs, np.array([-800, 6000], dtype=np.int64), band)
        for i, (a, b) in enumerate(pairs):
            assert bits(got, i) == bits(alone(plan, src[a], smp[b], band, (-800, 6000)), 0), i
        plan.set_lag_window(-20000, -1000)
        win = plan.xcorr_pool_phat_f32(src, smp, pairs, band=band)
        assert plan.lag_window == (-20000, -1000)
        for i, (a, b) in enumerate(pairs):
            assert bits(win, i) == bits(alone(plan, src[a], smp[b], band), 0), i          # (alone under the plan's window too)
            assert bits(win, i) == bits(alone(plan, src[a], smp[b], band, (-20000, -1000)), 0), i
        assert int(win[0][0]) == -9000


def test_indices_outside_the_pools(mod):
    """-1, nsources, nsamples and INT32_MAX give (0, NaN, NaN, -4), one of them over a row that is not a window; every other pair
    is what the same call returns without the bad rows"""
    n = 144000
    band = (1, n // 6)
    rng = np.random.default_rng(31)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[2], 4321, rng), rng.standard_normal(n).astype(np.float32)])
    ns, nm = src.shape[0], smp.shape[0]
    bad = [[-1, 0], [ns, 0], [0, nm], [0, -1], [INT32_MAX, 1], [1, INT32_MAX]]
    good = [[0, 0], [2, 0], [1, 1]]
    pairs = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2], bad[4], good[1], bad[5]], dtype=np.int32)
    is_bad = np.array([p in bad for p in pairs.tolist()])
    rows = np.tile(np.array([[-n, n - 1]], dtype=np.int64), (len(pairs), 1))
    rows[2] = (5, 4)                                   # -4 takes precedence over -2
    rows[3] = (4000, 5000)
    rows[6] = (7, 6)                                   # a pair inside its pools whose row is not a window: -2
    with mod.Plan(n, 4, 0) as plan:
        for windows in (None, rows):
            got = plan.xcorr_pool_phat_f32(src, smp, pairs, windows, band)
            ref = plan.xcorr_pool_phat_f32(src, smp, pairs[~is_bad], None if windows is None else windows[~is_bad], band)
            k = 0
            for i, p in enumerate(pairs.tolist()):
                if is_bad[i]:
                    assert is_refused(got, i, -4), (i, p, [a[i] for a in got])
                else:
                    assert bits(got, i) == bits(ref, k), (i, p)
                    k += 1
            assert int(got[0][3]) == 4321 and int(got[3][3]) == 0
            if windows is not None:
                assert is_refused(got, 6, -2), [a[6] for a in got]


def test_a_silent_track_in_a_pool(mod):
    """every pair with the silent track: the seed's lag, peak exactly 0, ret following the NaN coefficient; the others untouched"""
    n = 144000
    band = (300, n // 4)
    rng = np.random.default_rng(37)
    src = rng.standard_normal((2, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], 1234, rng), rng.standard_normal(n).astype(np.float32), shifted(src[1], -4321, rng)])
    quiet = smp.copy()
    quiet[1] = 0.0
    with mod.Plan(n, 4, 0) as plan:
        base = plan.xcorr_pool_phat_f32(src, smp, band=band)
        for window, seed in ((None, 0), ((100, 5000), 100)):
            if window:
                plan.set_lag_window(*window)
                base = plan.xcorr_pool_phat_f32(src, smp, band=band)
            got = plan.xcorr_pool_phat_f32(src, quiet, band=band)
            for a in range(2):
                for b in range(3):
                    if b == 1:
                        assert (int(got[0][a, b]), float(got[2][a, b]), int(got[3][a, b])) == (seed, 0.0, -1), (a, b, got)
                        assert np.isnan(got[1][a, b]) and not np.signbit(got[2][a, b])
                    else:
                        assert bits(got, 3 * a + b) == bits(base, 3 * a + b), (a, b)
        assert int(base[0][0, 0]) == 1234


def test_what_the_call_leaves_alone(mod, torch):
    """the counters, the exact switch, a plain pool call and a plain batch call afterwards, and NULL d_lag and d_peak"""
    n = 144000
    band = (1, n // 6)
    rng = np.random.default_rng(41)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[k], 1000 * (k + 1) * (-1) ** k, rng) for k in range(3)])

    def counters(plan):
        return plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats()

    with mod.Plan(n, 4, 0) as fresh:
        want_pool = fresh.xcorr_pool_f32(src, smp)
        want_batch = fresh.xcorr_batch_f32(src, smp)
    with mod.Plan(n, 4, 0) as plan:
        plan.xcorr_batch_f32(src, smp)                               # the counters hold something to begin with
        before = counters(plan)
        assert before[2] != (0, 0, 0) and before[3][1] > 0, before
        results = []
        for exact in (True, False):
            plan.set_exact(exact)
            results.append(plan.xcorr_pool_phat_f32(src, smp, band=band))
            results.append(plan.xcorr_pool_phat_f32(src, smp))
            plan.xcorr_pool_phat_f32(src, smp, [[0, 0], [5, 5], [1, 2]], [[-9, 9], [3, 2], [3, 2]], band)
        plan.set_exact(True)
        assert counters(plan) == before
        assert all_bits(results[0]) == all_bits(results[2]) and all_bits(results[1]) == all_bits(results[3])
        assert results[0][0].diagonal().tolist() == [1000, -2000, 3000]
        assert all_bits(plan.xcorr_pool_f32(src, smp)) == all_bits(want_pool)
        assert all_bits(plan.xcorr_batch_f32(src, smp)) == all_bits(want_batch)
        d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        whole = pool_dev(plan, torch, d_src, 2 * n, 3, d_smp, n, 3, None, 9, band)
        assert all_bits(whole) == all_bits(results[0])
        part = pool_dev(plan, torch, d_src, 2 * n, 3, d_smp, n, 3, None, 9, band, skip=(0, 2))
        assert (part[0] == -99).all() and (part[2] == 7.0).all()
        assert part[1].tobytes() == whole[1].tobytes() and part[3].tobytes() == whole[3].tobytes()


def test_refusals(mod, torch):
    n = 144000
    rng = np.random.default_rng(43)
    d_src = torch.from_numpy(rng.standard_normal(3 * 2 * n + 8).astype(np.float32)).cuda()
    d_smp = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    d_pairs = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    out = outputs(torch, 6)
    L, C, K, R = (a.data_ptr() for a in out)
    S, T, P = d_src.data_ptr(), d_smp.data_ptr(), d_pairs.data_ptr()

    def rejected(plan, text, *args):
        with pytest.raises(mod.AsxError, match=text):
            plan.xcorr_pool_phat_dev(*args)
        assert untouched(torch, out), args

    with mod.Plan(n, 4, 0) as plan:
        rejected(plan, "null", S, 2 * n, 3, T, n, 2, P, 0, 0, 4, 1, 100, L, 0, K, R)              # no coefficients
        rejected(plan, "null", S, 2 * n, 3, T, n, 2, P, 0, 0, 4, 1, 100, L, C, K, 0)              # no ret
        rejected(plan, "null", 0, 2 * n, 3, T, n, 2, P, 0, 0, 4, 1, 100, L, C, K, R)              # no sources
        rejected(plan, "null", S, 2 * n, 3, 0, n, 2, P, 0, 0, 4, 1, 100, L, C, K, R)              # no samples
        rejected(plan, "empty pool", S, 2 * n, 0, T, n, 2, P, 0, 0, 4, 1, 100, L, C, K, R)
        rejected(plan, "empty pool", S, 2 * n, 3, T, n, 0, P, 0, 0, 4, 1, 100, L, C, K, R)
        rejected(plan, "aligned", S + 4, 2 * n, 3, T, n, 2, P, 0, 0, 4, 1, 100, L, C, K, R)
        rejected(plan, "multiples of 4", S, 2 * n + 2, 3, T, n, 2, P, 0, 0, 4, 1, 100, L, C, K, R)
        rejected(plan, "every combination", S, 2 * n, 3, T, n, 2, 0, 0, 0, 5, 1, 100, L, C, K, R)  # 3 x 2 is 6 pairs
        for lo, hi in [(-1, 5), (0, n + 1), (5, 4)]:
            rejected(plan, "not a band", S, 2 * n, 3, T, n, 2, P, 0, 0, 4, lo, hi, L, C, K, R)
        assert plan.debug_bank() == (0, 0, 0)                                                     # nothing was filled either
        plan.xcorr_pool_phat_dev(S, 2 * n, 3, T, n, 2, P, 0, 0, 0, 1, 100, L, C, K, R)            # batch 0: nothing
        plan.sync()
        assert untouched(torch, out)
    m = 1000  # a length outside the tuned table: a packed plan
    with mod.Plan(m, 4, 0) as plan:
        assert plan.layout == "packed"
        for lo, hi in [(10, 100), (0, m)]:
            rejected(plan, "real-column", S, 2 * m, 3, T, m, 2, P, 0, 0, 4, lo, hi, L, C, K, R)


PACKED_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as graft
mod = graft.load()
n = 144000
with mod.Plan(n, 1, 0) as plan:
    assert plan.layout == "packed", plan.layout
    for band in ((1, n // 6), None):
        try:
            plan.xcorr_pool_phat_f32(np.ones((1, 2 * n), dtype=np.float32), np.ones((1, n), dtype=np.float32), band=band)
        except mod.AsxError as e:
            assert "real-column" in str(e), e
            print("refused", band)
"""


def test_a_production_length_forced_to_a_packed_plan_is_refused(mod):
    """ASX_LAYOUT=packed is read when a plan is made; a fresh process, so that nothing of this one's state is involved"""
    env = dict(os.environ, ASX_LAYOUT="packed")
    done = subprocess.run([sys.executable, "-c", PACKED_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split("\n")[:2] == ["refused (1, 24000)", "refused None"], (done.stdout, done.stderr)
