"""Top-k over pools on the MI355X (asx_xcorr_pool_topk_f32_dev, Plan.xcorr_pool_topk_f32, Plan.xcorr_pool_topk_dev) and the best-entry
consumer (asx_topk_best_dev, topk_best_dev).

Every pair inside its pools must give, in all k entries and bit for bit, what the top-k call gives for that pair alone on the same
plan with the same k, separation and window; the rule itself is checked against tests/topk_model.py (float64, built on the oracle):
lags and rets equal, coefficients within the project's 1e-5.  k = 1 is the pool call; an index outside its pool gives (0, NaN, -4)
in all k entries."""
import functools

import numpy as np
import pytest

from test_gpu_pool import INT32_MAX, periodic_pools, shifted
from test_gpu_topk import check_entries, counters, delta, over_list, period8, short_overlap, spike_run_ties
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


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    return t


def flat(out):
    """(lag, coef, ret) of any leading shape -> [B, k] each"""
    return tuple(np.ascontiguousarray(a).reshape(-1, a.shape[-1]) for a in out)


def ebits(out, i):
    """the bytes of all k entries of pair i"""
    return [a[i].tobytes() for a in flat(out)]


def alone(plan, src, smp, k, sep, row=None):
    """the pair alone through the top-k call (asx_xcorr_topk_f32_dev, one pair): the bytes of its k entries"""
    return ebits(plan.xcorr_topk_f32(src, smp, k, sep, row), 0)


def outputs(torch, entries):
    return (torch.full((entries,), -99, dtype=torch.int64, device="cuda"), torch.full((entries,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((entries,), 7, dtype=torch.int32, device="cuda"))


def pool_topk_dev(plan, torch, d_src, ss, ns, d_smp, ms, nm, pairs, batch, k, sep, windows=None, ws=0):
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda() if pairs is not None else None
    d_win = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.int64)).cuda() if windows is not None else None
    lag, coef, ret = outputs(torch, batch * k)
    torch.cuda.synchronize()
    plan.xcorr_pool_topk_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ms, nm, d_pairs.data_ptr() if d_pairs is not None else 0,
                             d_win.data_ptr() if d_win is not None else 0, ws, batch, k, sep, lag.data_ptr(), coef.data_ptr(),
                             ret.data_ptr())
    plan.sync()
    return tuple(a.cpu().numpy().reshape(batch, k) for a in (lag, coef, ret))


def is_invalid(out, i, code):
    lag, coef, ret = flat(out)
    return lag[i].tolist() == [0] * lag.shape[1] and bool(np.isnan(coef[i]).all()) and ret[i].tolist() == [code] * lag.shape[1]


# ---- 1. the small matrix ------------------------------------------------------------------------------------------------------
MATRIX_K, MATRIX_SEP = 3, 1000


@functools.lru_cache(maxsize=None)
def matrix_inputs(n):
    """3 sources x 2 samples: sample 0 = source 0 at lags a and b (0.6) + source 1 at lag c (0.35), sample 1 = source 2 at lags d and
    e (0.5); the lags of the N = 144 000 design scaled with N.  -> (sources, samples, lags, the model of the three related pairs)"""
    lags = tuple(v * (n // 144000) for v in (30000, -41000, 7000, -9000, 52000))
    a, b, c, d, e = lags
    rng = np.random.default_rng(53)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], a, rng) + 0.6 * shifted(src[0], b, rng) + 0.35 * shifted(src[1], c, rng),
                    shifted(src[2], d, rng) + 0.5 * shifted(src[2], e, rng)]).astype(np.float32)
    want = {p: model(src[p[0]], smp[p[1]], MATRIX_K, MATRIX_SEP) for p in ((0, 0), (1, 0), (2, 1))}
    return src, smp, lags, want


@functools.lru_cache(maxsize=None)
def matrix_run(n, spectral):
    mod = asx()
    src, smp, _, _ = matrix_inputs(n)
    with mod.Plan(n, 8, 0) as plan:
        assert plan.layout == "real-column"
        plan.set_pearson(spectral)
        fills = plan.debug_bank()[2]
        m0 = plan.pearson_modes()
        got = plan.xcorr_pool_topk_f32(src, smp, MATRIX_K, MATRIX_SEP)
        m1 = plan.pearson_modes()
        assert plan.debug_bank()[:2] == (3, 2) and plan.debug_bank()[2] == fills + 1
        # every entry of every pair is counted once under the spectral setting, none under the direct one
        assert sum(m1) - sum(m0) == (6 * MATRIX_K if spectral else 0), (spectral, m0, m1)
        ref = [alone(plan, src[a], smp[b], MATRIX_K, MATRIX_SEP) for a in range(3) for b in range(2)]
    return got, ref


@pytest.mark.parametrize("spectral", [True, False])
@pytest.mark.parametrize("n", PRODUCTION)
def test_small_matrix_at_every_length(mod, n, spectral):
    """all 18 entries equal the top-k call alone, bit for bit; the related pairs equal the model, the planted lags in front"""
    src, smp, (a, b, c, d, e), want = matrix_inputs(n)
    assert [w[1] for w in want[(0, 0)][:2]] == [a, b] and want[(1, 0)][0][1] == c and [w[1] for w in want[(2, 1)][:2]] == [d, e], want
    got, ref = matrix_run(n, spectral)
    assert got[0].shape == (3, 2, MATRIX_K)
    for i in range(6):
        assert ebits(got, i) == ref[i], (n, spectral, divmod(i, 2))
    lag, coef, ret = flat(got)
    for (s, t), w in want.items():
        i = 2 * s + t
        check_entries((lag[i], coef[i], ret[i]), w, (n, spectral, s, t))
    for i in (1, 3, 4):                                     # the unrelated pairs (0, 1), (1, 1), (2, 0)
        assert (np.abs(coef[i]) < 0.1).all() and (ret[i] == 0).all(), (i, coef[i])


# ---- 2. explicit lists ---------------------------------------------------------------------------------------------------------
def test_explicit_list_aliases_and_overlapping_windows(mod, torch):
    """arbitrary order and duplicates; one pool of clips as both sources and samples; a source pool of overlapping windows"""
    n, hop, k, sep = 144000, 36000, 3, 500
    rng = np.random.default_rng(17)
    rec = rng.standard_normal(2 * n + 5 * hop).astype(np.float32)          # windows k * hop .. k * hop + 2N, k = 0..5
    nwin = 6
    clips = np.stack([np.concatenate([shifted(rec[j * hop:j * hop + 2 * n], (-1) ** j * (1000 + 7 * j), rng),
                                      rng.standard_normal(n).astype(np.float32)]) for j in range(4)])   # [4, 2N]
    pairs = np.array([[3, 1], [0, 0], [0, 0], [5, 2], [1, 3], [2, 2], [4, 0], [0, 3]], dtype=np.int32)
    d_rec = torch.from_numpy(rec).cuda()
    d_clips = torch.from_numpy(clips).cuda()
    with mod.Plan(n, 8, 0) as plan:
        got = pool_topk_dev(plan, torch, d_rec, hop, nwin, d_clips, 2 * n, 4, pairs, len(pairs), k, sep)
        for i, (a, b) in enumerate(pairs):
            assert ebits(got, i) == alone(plan, rec[a * hop:a * hop + 2 * n], clips[b, :n], k, sep), (i, a, b)
        assert ebits(got, 1) == ebits(got, 2)
        for i, (a, b) in enumerate(pairs):
            if a == b:
                assert int(got[0][i][0]) == (-1) ** a * (1000 + 7 * a) and int(got[2][i][0]) == 0
        # all pairs a != b of one pool: the same buffer as sources (2N) and samples (its first N frames)
        allp = np.array([[a, b] for a in range(4) for b in range(4) if a != b][::-1], dtype=np.int32)
        got = pool_topk_dev(plan, torch, d_clips, 2 * n, 4, d_clips, 2 * n, 4, allp, len(allp), k, sep)
        for i, (a, b) in enumerate(allp):
            assert ebits(got, i) == alone(plan, clips[a], clips[b, :n], k, sep), (i, a, b)


# ---- 3. per-pair rows ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_run():
    mod = asx()
    n, k, sep = 288000, 2, 1000
    rng = np.random.default_rng(23)
    src = rng.standard_normal((2, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], 5000, rng) + 0.6 * shifted(src[0], -9000, rng), shifted(src[1], -777, rng)])
    pairs = np.array([[0, 0], [0, 0], [1, 1], [0, 1], [1, 1]], dtype=np.int32)
    # a full row, one without the strongest copy, a one-lag row, a row that is not a window, a short one
    rows = np.array([[-n, n - 1], [-20000, -1000], [-777, -777], [3, 2], [-5000, 20]], dtype=np.int64)
    with mod.Plan(n, 8, 0) as plan:
        got = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs, rows)
        ref = [alone(plan, src[a], smp[b], k, sep, rows[i]) for i, (a, b) in enumerate(pairs)]
        one = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs, np.array([-800, 6000], dtype=np.int64))
        ref_one = [alone(plan, src[a], smp[b], k, sep, (-800, 6000)) for a, b in pairs]
        want = {i: model(src[a], smp[b], k, sep, int(rows[i][0]), int(rows[i][1])) for i, (a, b) in enumerate(pairs) if i != 3}
    return got, ref, one, ref_one, want


def test_per_pair_rows_match_the_topk_call(mod):
    got, ref, one, ref_one, want = rows_run()
    lag, coef, ret = flat(got)
    for i in range(5):
        assert ebits(got, i) == ref[i], i
        assert ebits(one, i) == ref_one[i], i
        if i != 3:
            check_entries((lag[i], coef[i], ret[i]), want[i], i)
    assert lag[0].tolist() == [5000, -9000] and int(lag[1][0]) == -9000      # without the strongest copy the runner-up leads
    assert (int(lag[2][0]), int(ret[2][0])) == (-777, 0)
    assert (int(lag[2][1]), int(ret[2][1])) == (0, -3) and np.isnan(coef[2][1])   # a one-lag row has no second entry
    assert is_invalid(got, 3, -2)


# ---- 4. the plan's window ------------------------------------------------------------------------------------------------------
def test_plan_window_is_honoured_and_left_alone(mod):
    n, k, sep = 144000, 3, 1000
    rng = np.random.default_rng(61)
    src = rng.standard_normal((2, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], 5000, rng) + 0.7 * shifted(src[0], 20000, rng) + 0.45 * shifted(src[0], -12000, rng),
                    shifted(src[1], 14000, rng)]).astype(np.float32)
    with mod.Plan(n, 4, 0) as plan:
        plan.set_lag_window(-15000, 15000)
        got = plan.xcorr_pool_topk_f32(src, smp, k, sep)
        assert plan.lag_window == (-15000, 15000)
        lag, coef, ret = flat(got)
        for a in range(2):
            for b in range(2):
                assert ebits(got, 2 * a + b) == alone(plan, src[a], smp[b], k, sep), (a, b)
        for i, (a, b) in ((0, (0, 0)), (3, (1, 1))):
            check_entries((lag[i], coef[i], ret[i]), model(src[a], smp[b], k, sep, -15000, 15000), (a, b))
        assert lag[0].tolist()[:2] == [5000, -12000] and int(lag[3][0]) == 14000    # lag 20000 is outside the window
        assert plan.lag_window == (-15000, 15000)


# ---- 5. k = 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectral", [True, False])
def test_k1_is_the_pool_call(mod, spectral):
    n = 144000
    src, smp = periodic_pools(n)
    pairs = np.array([[1, 3], [0, 0], [0, 1], [1, 0], [0, 2], [0, 3], [0, 0], [5, 0]], dtype=np.int32)
    rows = np.tile(np.array([[-n, n - 1]], dtype=np.int64), (len(pairs), 1))
    rows[3] = (7, 3)
    with mod.Plan(n, 8, 0) as plan:
        plan.set_pearson(spectral)
        for exact in (True, False):
            plan.set_exact(exact)
            for w in (None, rows):
                c0 = counters(plan)
                want = plan.xcorr_pool_f32(src, smp, pairs, w)
                c1 = counters(plan)
                got = plan.xcorr_pool_topk_f32(src, smp, 1, 12345, pairs, w)
                c2 = counters(plan)
                assert got[0].shape == (len(pairs), 1)
                assert [a.tobytes() for a in got] == [a.tobytes() for a in want], (spectral, exact, w is None)
                assert delta(c0, c1) == delta(c1, c2) and delta(c0, c1)[0] >= 3, (c0, c1, c2)
        plan.set_exact(True)
        full = plan.xcorr_pool_f32(src, smp)
        got = plan.xcorr_pool_topk_f32(src, smp, 1, 0)
        assert got[0].shape == (2, 4, 1) and [a.tobytes() for a in got] == [a.tobytes() for a in full]


# ---- 6. indices outside the pools ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def invalid_run():
    mod = asx()
    n, k, sep = 144000, 3, 1000
    src, smp = periodic_pools(n)
    rng = np.random.default_rng(31)
    src = np.concatenate([src, rng.standard_normal((1, 2 * n)).astype(np.float32)])
    smp = np.concatenate([smp, shifted(src[2], 4321, rng)[None, :]])
    ns, nm = src.shape[0], smp.shape[0]
    bad = [[-1, 0], [ns, 0], [0, nm], [0, -1], [INT32_MAX, 1], [1, INT32_MAX], [-2 ** 31, -2 ** 31]]
    good = [[0, 0], [2, 4], [1, 3]]
    pairs = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2], bad[4], good[0], bad[5], bad[6]], dtype=np.int32)
    is_bad = [list(p) in bad for p in pairs.tolist()]
    rows = np.tile(np.array([[-n, n - 1]], dtype=np.int64), (len(pairs), 1))
    rows[2] = (5, 4)                                   # -4 takes precedence over -2
    rows[3] = (4000, 5000)
    rows[6] = (9, 8)                                   # a valid pair with an invalid row keeps its -2
    with mod.Plan(n, 4, 0) as plan:
        ref = {tuple(p): alone(plan, src[p[0]], smp[p[1]], k, sep) for p in good}
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        got = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs)
        counted = (plan.peak_overflows() - o0, plan.peak_repairs() - r0)
        ref_rows = {i: alone(plan, src[p[0]], smp[p[1]], k, sep, rows[i]) for i, p in enumerate(pairs.tolist()) if not is_bad[i]}
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        got_rows = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs, rows)
        counted_rows = (plan.peak_overflows() - o0, plan.peak_repairs() - r0)
    return pairs, is_bad, got, ref, counted, got_rows, ref_rows, counted_rows


def test_indices_outside_the_pools(mod):
    """(0, NaN, -4) in all k entries, between ordinary and overflowing pairs, which stay as they are alone; -4 wins over -2"""
    pairs, is_bad, got, ref, counted, got_rows, ref_rows, counted_rows = invalid_run()
    assert counted == (2, 2) and counted_rows == (2, 2)       # pairs 0 and 8, the periodic pair twice: the valid overflowing pairs
    for i, p in enumerate(pairs.tolist()):
        if is_bad[i]:
            assert is_invalid(got, i, -4) and is_invalid(got_rows, i, -4), (i, p)
        else:
            assert ebits(got, i) == ref[tuple(p)], (i, p)
            assert ebits(got_rows, i) == ref_rows[i], (i, p)
    assert int(got[0][3][0]) == 4321 and int(got_rows[0][3][0]) == 4321
    assert is_invalid(got_rows, 6, -2)


# ---- 7. overflows --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow_run():
    """pools with the period-8 track (2N/8 exact ties: pass 1 overflows), the spike-and-run track against a unit impulse (pass 1 is
    clean, pass 2 is left nothing but ties) and an ordinary pair"""
    mod = asx()
    n, k = 144000, 3
    with mod.Plan(n, 1, 0) as probe:
        m2 = probe.split[1]
    per = period8(n)
    spike, run = spike_run_ties(n, m2, n // 2, 1.0)
    sep = run + 2
    rng = np.random.default_rng(67)
    plain = rng.standard_normal(2 * n).astype(np.float32)
    impulse = np.zeros(n, np.float32)
    impulse[0] = 1.0
    src = np.stack([per, spike, plain])
    smp = np.stack([per[:n], impulse, shifted(plain, 4321, rng)])
    pairs = np.array([[2, 2], [0, 0], [1, 1], [2, 2]], dtype=np.int32)
    first_overflow = [k, 0, 1, k]
    # exact r where the oracle's float64 transforms would round exact ties apart: the period-8 pair's r has period 8 and integer
    # values, the impulse's r is the source itself
    base = per[:8].astype(np.float64)
    r8 = np.array([(n // 8) * float(np.dot(np.roll(base, -m), base)) for m in range(8)])
    exact_r = {0: np.tile(r8, 2 * n // 8), 1: spike.astype(np.float64), 2: None}
    want = [model(src[a], smp[b], k, sep, r=exact_r[a]) for a, b in pairs]
    res = {}
    with mod.Plan(n, 4, 0) as plan:
        assert plan.peak_capacity < 2 * n
        for exact in (True, False):
            plan.set_exact(exact)
            ref = [alone(plan, src[a], smp[b], k, sep) for a, b in pairs]
            c0 = (plan.peak_overflows(), plan.peak_repairs())
            got = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs)
            listed = over_list(mod, plan)
            c1 = (plan.peak_overflows(), plan.peak_repairs())
            res[exact] = (got, ref, delta(c0, c1), listed)
        plan.set_exact(True)
    return pairs, first_overflow, want, res


def test_overflow_in_the_first_and_in_the_second_pass(mod):
    pairs, first_overflow, want, res = overflow_run()
    k = 3
    got, ref, counted, listed = res[True]
    lag, coef, ret = flat(got)
    assert counted == (2, 2) and listed == (0, 0)             # one overflow and one repair per such pair and call
    for i in range(len(pairs)):
        assert ebits(got, i) == ref[i], ("exact", i)
        check_entries((lag[i], coef[i], ret[i]), want[i], ("exact", i))
    agot, aref, acounted, alisted = res[False]
    alag, acoef, aret = flat(agot)
    assert acounted == (2, 0) and alisted == (0, 0)           # counted, never listed, repairs do not move
    for i in range(len(pairs)):
        f = first_overflow[i]
        assert ebits(agot, i) == aref[i], ("async", i)
        assert aret[i].tolist() == ret[i].tolist()[:f] + [1] * (k - f), (i, aret[i])
        assert alag[i].tolist()[:f] == lag[i].tolist()[:f], i
    # an ordinary pair is the same in both modes, bit for bit
    assert ebits(agot, 0) == ebits(got, 0) == ebits(got, 3)


# ---- 8. launch groups and lanes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_several_launch_groups(mod, monkeypatch, lanes):
    """group 3, one and two lanes: consecutive groups share slots; the bank is filled once per call, whatever k is"""
    monkeypatch.setenv("ASX_LANES", lanes)
    n, k, sep = 144000, 3, 2000
    rng = np.random.default_rng(29)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    lags = [(j * 37717) % n - n // 2 for j in range(4)]
    smp = np.stack([shifted(src[j % 3], lags[j], rng, 0.3) + 0.5 * shifted(src[j % 3], lags[j] // 2 + 5000, rng, 0.3) for j in range(4)])
    pairs = np.array([[j % 3, j % 4] for j in range(10)] + [[0, 3], [0, 3]], dtype=np.int32)
    with mod.Plan(n, 3, 0) as plan:
        assert plan.group == 3
        f0 = plan.debug_bank()[2]
        got = plan.xcorr_pool_topk_f32(src, smp, k, sep, pairs)
        assert plan.debug_bank()[2] == f0 + 1
        ref = {}
        for i, (a, b) in enumerate(pairs.tolist()):
            if (a, b) not in ref:
                ref[(a, b)] = alone(plan, src[a], smp[b], k, sep)
            assert ebits(got, i) == ref[(a, b)], (lanes, i)
            if a == b % 3:
                assert got[0][i].tolist()[:2] == [lags[b], lags[b] // 2 + 5000], (i, got[0][i])
        full = plan.xcorr_pool_topk_f32(src, smp, k, sep)
        assert plan.debug_bank()[2] == f0 + 2 and full[0].shape == (3, 4, k)
        for a in range(3):
            for b in range(4):
                if (a, b) in ref:
                    assert ebits(full, 4 * a + b) == ref[(a, b)], (lanes, a, b)


# ---- 9. bad arguments ----------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_alone(mod, torch, monkeypatch):
    n, k = 144000, 4
    rng = np.random.default_rng(37)
    d_src = torch.from_numpy(rng.standard_normal(3 * 2 * n).astype(np.float32)).cuda()
    d_smp = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    d_pairs = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    lag, coef, ret = outputs(torch, 6 * k)
    L, C, R = lag.data_ptr(), coef.data_ptr(), ret.data_ptr()
    S, T, P = d_src.data_ptr(), d_smp.data_ptr(), d_pairs.data_ptr()

    def rejected(plan, *args):
        with pytest.raises(mod.AsxError):
            plan.xcorr_pool_topk_dev(*args)
        torch.cuda.synchronize()
        assert (lag == -99).all() and (coef == 7.0).all() and (ret == 7).all()

    with mod.Plan(n, 4, 0) as plan:
        f0 = plan.debug_bank()[2]
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, L, 0, R)              # no coefficients
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, L, C, 0)              # no ret
        rejected(plan, 0, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, L, C, R)              # no sources
        rejected(plan, S, 2 * n, 3, 0, n, 2, P, 0, 0, 4, k, 10, L, C, R)              # no samples
        rejected(plan, S, 2 * n, 0, T, n, 2, P, 0, 0, 4, k, 10, L, C, R)              # empty source pool
        rejected(plan, S, 2 * n, 3, T, n, 0, P, 0, 0, 4, k, 10, L, C, R)              # empty sample pool
        rejected(plan, S + 4, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, L, C, R)          # not 16-byte aligned
        rejected(plan, S, 2 * n + 2, 2, T, n, 2, P, 0, 0, 4, k, 10, L, C, R)          # stride not a multiple of 4
        rejected(plan, S, 2 * n, 3, T, n, 2, 0, 0, 0, 5, k, 10, L, C, R)              # implicit product of 3 x 2 is 6 pairs
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, 0, 10, L, C, R)              # k = 0
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, 9, 10, L, C, R)              # k = 9
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, -1, 10, L, C, R)             # k = -1
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, -1, L, C, R)              # a negative separation
        plan.xcorr_pool_topk_dev(S, 2 * n, 3, T, n, 2, P, 0, 0, 0, k, 10, L, C, R)    # batch 0: nothing
        plan.sync()
        assert (lag == -99).all() and (ret == 7).all()
        assert plan.debug_bank()[2] == f0                                             # nothing was launched
        # and a good call with d_lag = NULL writes coef and ret only, k entries per pair
        plan.xcorr_pool_topk_dev(S, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, 0, C, R)
        plan.sync()
        torch.cuda.synchronize()
        assert (lag == -99).all() and (ret[:4 * k] == 0).all() and (ret[4 * k:] == 7).all() and (coef[4 * k:] == 7.0).all()
        lag2, coef2, ret2 = outputs(torch, 6 * k)
    lag, coef, ret = lag2, coef2, ret2
    L, C, R = lag.data_ptr(), coef.data_ptr(), ret.data_ptr()
    monkeypatch.setenv("ASX_LAYOUT", "packed")
    with mod.Plan(n, 4, 0) as plan:
        assert plan.layout == "packed"
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, k, 10, L, C, R)


# ---- 10. other calls afterwards ------------------------------------------------------------------------------------------------
def test_other_calls_after_a_pool_topk_call(mod):
    """a pool call, a top-k call, a broadcast strided call and a contiguous call after a pool top-k call return what they return on
    a plan that never made one"""
    n, k, sep = 144000, 3, 800
    rng = np.random.default_rng(41)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[j], 1000 * (j + 1) * (-1) ** j, rng) + 0.5 * shifted(src[j], 30000 + j, rng) for j in range(3)])

    def others(plan):
        return (plan.xcorr_pool_f32(src, smp), plan.xcorr_topk_f32(src, smp, k, sep), plan.xcorr_broadcast_f32(src[0], smp),
                plan.xcorr_batch_f32(src, smp))

    with mod.Plan(n, 4, 0) as fresh:
        want = others(fresh)
    with mod.Plan(n, 4, 0) as plan:
        first = plan.xcorr_pool_topk_f32(src, smp, k, sep)
        got = others(plan)
        again = plan.xcorr_pool_topk_f32(src, smp, k, sep)
    for w, g in zip(want, got):
        assert [a.tobytes() for a in w] == [a.tobytes() for a in g]
    assert [a.tobytes() for a in first] == [a.tobytes() for a in again]
    for j in range(3):                                       # the diagonal of the matrix is the top-k call's batch
        assert ebits(first, 3 * j + j) == ebits(want[1], j), j


# ---- 11, 12. the result consumers ----------------------------------------------------------------------------------------------
def to_dev(torch, out):
    lag, coef, ret = flat(out)
    return (torch.from_numpy(lag.copy()).cuda(), torch.from_numpy(coef.copy()).cuda(), torch.from_numpy(ret.copy()).cuda())


def test_results_to_ms_takes_the_flat_layout(mod, torch):
    """results_to_ms_dev over the flat batch * k arrays gives, per entry, what it gives for that entry alone"""
    got, _ = matrix_run(144000, True)
    d_lag, d_coef, d_ret = to_dev(torch, got)
    entries = d_lag.numel()
    assert entries == 18
    ms = torch.full((entries,), -5, dtype=torch.int64, device="cuda")
    acc = torch.full((entries,), -5, dtype=torch.int32, device="cuda")
    one_ms = torch.full((entries,), -6, dtype=torch.int64, device="cuda")
    one_acc = torch.full((entries,), -6, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mod.results_to_ms_dev(d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr(), entries, ms.data_ptr(), acc.data_ptr(), 0.4, 48000.0)
    for e in range(entries):
        mod.results_to_ms_dev(d_lag.data_ptr() + 8 * e, d_coef.data_ptr() + 8 * e, d_ret.data_ptr() + 4 * e, 1, one_ms.data_ptr() + 8 * e,
                              one_acc.data_ptr() + 4 * e, 0.4, 48000.0)
    torch.cuda.synchronize()
    assert torch.equal(ms, one_ms) and torch.equal(acc, one_acc)
    lag, coef, ret = flat(got)
    x = lag * (1000.0 / 48000.0)                            # C round(): halves away from zero
    assert ms.cpu().numpy().reshape(6, 3).tolist() == (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64).tolist()
    assert acc.cpu().numpy().reshape(6, 3).tolist() == ((ret == 0) & (coef >= 0.4)).astype(np.int32).tolist()
    assert acc.cpu().numpy().reshape(6, 3)[0].tolist() == [1, 1, 0]        # the two planted copies of pair (0, 0)


def best_rule(lag, coef, ret):
    """the rule of asx_topk_best_dev: among the entries with ret == 0 the largest signed coefficient, the smallest j among equals;
    none: entry 0 as it is"""
    ok = ret == 0
    j = np.where(ok.any(axis=1), np.argmax(np.where(ok, coef, -np.inf), axis=1), 0)
    i = np.arange(ret.shape[0])
    return lag[i, j], coef[i, j], ret[i, j], j.astype(np.int32)


def best_dev(mod, torch, out, want_lag=True, want_entry=True):
    d_lag, d_coef, d_ret = to_dev(torch, out)
    batch, k = flat(out)[0].shape
    b_lag = torch.full((batch,), -99, dtype=torch.int64, device="cuda")
    b_coef = torch.full((batch,), 7.0, dtype=torch.float64, device="cuda")
    b_ret = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    b_entry = torch.full((batch,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    mod.topk_best_dev(d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr(), batch, k, b_coef.data_ptr(), b_ret.data_ptr(),
                      b_lag.data_ptr() if want_lag else 0, b_entry.data_ptr() if want_entry else 0)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (b_lag, b_coef, b_ret, b_entry))


def test_best_entry(mod, torch):
    """topk_best_dev over the outputs of the tests above (a runner-up with the higher coefficient, -3 and -2 entries, -4 pairs,
    ret = 1 entries of the asynchronous mode), a NaN coefficient with ret = -1 and a constructed tie, against best_rule"""
    n = 144000
    src, smp = short_overlap(n, -110000, 1000, 5)
    silent = np.zeros(n, np.float32)                        # a silent sample: NaN coefficients with ret = -1
    with mod.Plan(n, 2, 0) as plan:
        runner = plan.xcorr_topk_f32(np.stack([src, src]), np.stack([smp, silent]), 2, 200)
    assert runner[2].tolist() == [[0, 0], [-1, -1]] and np.isnan(runner[1][1]).all(), runner
    tie = (np.array([[5, 6, 7, 8], [1, 2, 3, 4]], dtype=np.int64), np.array([[0.25, 0.5, 0.5, 0.5], [0.9, -0.5, 0.9, 0.1]]),
           np.array([[0, 0, 0, 1], [-1, 0, 0, 0]], dtype=np.int32))
    cases = {"matrix": matrix_run(n, True)[0], "matrix direct": matrix_run(n, False)[0], "rows": rows_run()[0],
             "invalid": invalid_run()[2], "invalid rows": invalid_run()[5], "exact": overflow_run()[3][True][0],
             "async": overflow_run()[3][False][0], "runner-up": runner, "tie": tie}
    for what, out in cases.items():
        lag, coef, ret = flat(out)
        want = best_rule(lag, coef, ret)
        got = best_dev(mod, torch, out)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), (what, got, want)
    # what the cases hold: the true offset of the runner-up pair is entry 1; a pair with nothing to accept returns entry 0
    got = best_dev(mod, torch, runner)
    assert (int(got[0][0]), int(got[2][0]), int(got[3][0])) == (-110000, 0, 1) and got[1][0] >= 0.95
    assert (int(got[2][1]), int(got[3][1])) == (-1, 0) and np.isnan(got[1][1])
    got = best_dev(mod, torch, tie)
    assert got[3].tolist() == [1, 2] and got[0].tolist() == [6, 3]
    got = best_dev(mod, torch, cases["invalid rows"])
    assert int(got[2][1]) == -4 and int(got[2][6]) == -2 and int(got[3][1]) == 0
    got = best_dev(mod, torch, cases["async"])
    assert got[2].tolist()[1:3] == [1, 0] and int(got[3][2]) == 0      # all entries inexact: entry 0; else the exact entry 0
    got = best_dev(mod, torch, cases["rows"])
    assert (int(got[0][2]), int(got[3][2])) == (-777, 0)               # the -3 entry never wins
    # d_best_lag and d_best_entry may be NULL
    got = best_dev(mod, torch, runner, want_lag=False, want_entry=False)
    assert got[0].tolist() == [-99, -99] and got[3].tolist() == [7, 7] and int(got[2][0]) == 0


def test_best_entry_bad_arguments(mod, torch):
    d_lag = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_coef = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_ret = torch.zeros(8, dtype=torch.int32, device="cuda")
    b_lag, b_coef, b_ret = outputs(torch, 2)
    b_entry = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L, C, R, BL, BC, BR, BE = (a.data_ptr() for a in (d_lag, d_coef, d_ret, b_lag, b_coef, b_ret, b_entry))
    for args in ((L, C, R, 2, 0, BC, BR, BL, BE), (L, C, R, 2, 9, BC, BR, BL, BE), (L, C, R, 2, -1, BC, BR, BL, BE),
                 (0, C, R, 2, 4, BC, BR, BL, BE), (L, 0, R, 2, 4, BC, BR, BL, BE), (L, C, 0, 2, 4, BC, BR, BL, BE),
                 (L, C, R, 2, 4, 0, BR, BL, BE), (L, C, R, 2, 4, BC, 0, BL, BE)):
        with pytest.raises(mod.AsxError):
            mod.topk_best_dev(*args)
    torch.cuda.synchronize()
    assert (b_lag == -99).all() and (b_coef == 7.0).all() and (b_ret == 7).all() and (b_entry == 7).all()
    mod.topk_best_dev(L, C, R, 0, 4, BC, BR, BL, BE)        # batch 0: nothing
    torch.cuda.synchronize()
    assert (b_lag == -99).all() and (b_ret == 7).all()
