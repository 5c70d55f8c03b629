"""Full-range normalised cross-correlation on the MI355X (asx_xcorr_ncc_full_f32_dev, asx_xcorr_ncc_full_topk_f32_dev,
asx_xcorr_ncc_full_debug_c_dev) against the float64 model of tests/ncc_full_model.py: the whole signed curve at the lengths the chunk
arithmetic tells apart on both sides of zero, fixture D, the two consequences against the NCC call, parity over groups, broadcast and
overlap, rows, min_overlap, pairs in which nothing competes, top-k on fixture E, edges, the state the call must leave alone,
refusals."""
import numpy as np
import pytest

import edges
import ncc_full_model as fm
import oracle
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
# max over the competing lags l < 0 of |d_c - model| * sqrt(Vx[l] Vy[l] / (Vmax Vy)): the error brought to the full window's scale,
# where the error of r32 lives (test_whole_curve_*, with min_overlap = 1; the model's r is float64).  Measured on an MI355X, the
# generator pair / fixture D: N = 3 2.4e-17 / -, 1000 2.39e-8 / 1.69e-8, 2047 5.67e-8 / 2.25e-8, 2048 1.64e-8 / 4.60e-8, 2049 1.82e-8
# / 4.18e-8, 5000 3.48e-8 / 1.94e-8, 144 000 1.61e-8 / 1.14e-8 (the unscaled error: between 4.5e-8 and 4.4e-7, the short overlaps'; a
# few float32 ulps of rlo32 over the full window's energies, and half an ulp of c32 itself).  Asserted at four times the largest
# value seen, 2.3e-7, rounded up to one significant digit; the hard cap is 1e-3.  profiles/ncc/full_cost.txt holds the same figures.
# Every lag assertion below rests on a model margin of at least 0.2 (asserted where the pair's model is formed), so the tolerance
# cannot hide a wrong lag.
FULL_TOL = 3e-7
assert FULL_TOL <= 1e-3
MARGIN = 0.2
# Packed plans at the lengths the chunk arithmetic tells apart (2048 frames per chunk, 2048 indices of the 2N - 1 per peak block): 1
# (one lag), 2 and 3 (one and two negative lags), 1000 (a partial chunk), 2047 / 2048 / 2049 (the chunk edge of the tracks, and of the
# curve's two halves), 5000 (three chunks per track; a sample's suffix starts from two whole chunks).
SMALL = (1, 2, 3, 1000, 2047, 2048, 2049, 5000)
BIG = 144000   # a real-column plan

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pair_d(n, p=0):
    return cached(("d", n, p), lambda: fm.fixture_d(n, p))


def pair_e(n, p=0):
    return cached(("e", n, p), lambda: fm.fixture_e(n, p))


def pair_g(n, k=0):
    """a generator pair (planted on either side of zero)"""
    return cached(("g", n, k), lambda: oracle.synth_pair(31, n % 7 + k, n, 1))


def curve_of(key, src, smp):
    """the model's curve of a pair, computed once and never written to"""
    def make():
        cv = fm.curve(src, smp)
        for a in (cv[0], cv[1], cv[4]):
            a.setflags(write=False)
        return cv
    return cached(("curve",) + tuple(key), make)


def model_of(key, src, smp, row=None, min_overlap=None, margin=True):
    """the model's (ret, lag, coef, peak); margin: its |c| stands MARGIN above every other competing lag of the row"""
    n = smp.size
    cv = curve_of(key, src, smp)
    m = fm.model(src, smp, row=row, min_overlap=min_overlap, cv=cv)
    if margin:
        ok = fm.competing(cv, min_overlap=min_overlap).copy()
        if row is not None:
            ok[:row[0] + n - 1] = False
            ok[row[1] + n:] = False
        assert m[0] == 0 and m[3] - fm.runner_up(cv, ok, m[1]) >= MARGIN, (key, row, m)
    return m


def scale_at(cv, lag):
    """sqrt(Vx[l] Vy[l] / (Vmax Vy)): what brings an error of c[l] to the full window's scale"""
    n = (cv[0].size + 1) // 2
    return float(np.sqrt(cv[1][lag + n - 1] / (cv[2] * cv[3])))


def bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


def same(a, b):
    return [x.tobytes() for x in a] == [x.tobytes() for x in b]


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


def outputs(torch, count=1):
    return (torch.zeros(count, dtype=torch.int64, device="cuda"), torch.zeros(count, dtype=torch.float64, device="cuda"),
            torch.zeros(count, dtype=torch.float64, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"))


def debug_curves(plan, torch, src, smp, min_overlap=1, min_energy=fm.DEFAULT_ENERGY):
    """-> (d_c float32 [2N - 1] and its results, the NCC debug call's d_c [N] and its results)"""
    n = smp.size
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    d_c = torch.full((2 * n - 1,), 7.0, dtype=torch.float32, device="cuda")
    d_h = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    out, out_h = outputs(torch), outputs(torch)
    torch.cuda.synchronize()
    plan.ncc_full_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), min_energy, min_overlap, d_c.data_ptr(), *(a.data_ptr() for a in out))
    plan.ncc_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), min_energy, d_h.data_ptr(), *(a.data_ptr() for a in out_h))
    plan.sync()
    return d_c.cpu().numpy(), tuple(a.cpu().numpy() for a in out), d_h.cpu().numpy(), tuple(a.cpu().numpy() for a in out_h)


def check_curve(what, plan, torch, src, smp):
    """The debug call with min_overlap = 1 against the model and against the NCC debug call.  -> the worst scaled error"""
    n = smp.size
    c32, got, hi32, _ = debug_curves(plan, torch, src, smp)
    cv = curve_of(what, src, smp)
    # l >= 0: the NCC call's curve, bit for bit
    assert c32[n - 1:].tobytes() == hi32.tobytes(), what
    # l < 0: the model's competing set but for the lags within a factor 2 of the threshold, at most 2 % of the curve
    ok = fm.competing(cv, min_overlap=1)
    near = fm.near_threshold(cv)
    assert near.sum() <= 0.02 * c32.size, (what, int(near.sum()))
    lo = np.arange(c32.size) < n - 1
    sure = lo & ~near
    assert np.array_equal(np.isnan(c32)[sure], ~ok[sure]), (what, np.flatnonzero(sure & (np.isnan(c32) != ~ok))[:8])
    both = lo & ok & ~np.isnan(c32)
    err = scaled = 0.0
    if both.any():
        diff = np.abs(c32[both].astype(np.float64) - cv[0][both])
        err = float(diff.max())
        scaled = float((diff * np.sqrt(cv[1][both] / (cv[2] * cv[3]))).max())
    print("ncc full curve", what, "competing l<0", int((ok & lo).sum()), "of", n - 1, "near the threshold", int(near.sum()),
          "max scaled |d_c - model|", scaled, "unscaled", err)
    # the returned lag: the smallest index of the maximum of |d_c| itself
    lag, coef, peak, ret = (a[0] for a in got)
    mine = np.where(np.isnan(c32), np.float32(-1.0), np.abs(c32))
    if mine.max() >= 0:
        assert int(lag) == int(np.argmax(mine)) - (n - 1) and float(peak) == float(mine.max()), (what, lag, peak, int(np.argmax(mine)))
    else:
        assert (int(lag), float(peak)) == (-(n - 1), 0.0), (what, lag, peak)
    assert scaled <= FULL_TOL, (what, scaled)
    return scaled


@pytest.mark.parametrize("n", SMALL)
def test_whole_curve_at_small_lengths_on_packed_plans(mod, torch, n):
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "packed"
        src, smp, _ = pair_g(n)
        check_curve(("g", n), plan, torch, src, smp)
        if n >= 1000:
            src, smp, planted = pair_d(n)
            check_curve(("d", n), plan, torch, src, smp)


def test_whole_curve_on_a_real_column_plan(mod, torch):
    n = BIG
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "real-column"
        check_curve(("d", n), plan, torch, *pair_d(n)[:2])
        check_curve(("g", n), plan, torch, *pair_g(n)[:2])


def check_pair(got, k, m, cv, what):
    lag, coef, peak, ret = (a[k] for a in got)
    print("ncc full", what, "lag", int(lag), "model", m[1], "peak", float(peak), "model", m[3], "diff", abs(float(peak) - m[3]))
    assert (int(ret), int(lag)) == (m[0], m[1]), (what, lag, coef, peak, ret, m)
    assert abs(float(coef) - m[2]) < COEF_TOL, (what, coef, m)
    assert abs(float(peak) - m[3]) <= FULL_TOL / scale_at(cv, m[1]) + 1e-7, (what, peak, m)


def parity_pairs(n):
    """fixture D three times, fixture E, a generator pair"""
    return [pair_d(n, 0), pair_d(n, 1), pair_d(n, 2), pair_e(n, 0), pair_g(n, 1)]


@pytest.mark.parametrize("n", [2049, BIG])
def test_fixture_d_and_parity_over_groups(mod, n):
    """max_batch 2 and five pairs: three groups.  Fixture D returns the planted lag; each pair alone gives the bits it gives inside
    the batch, in either order; coef is the windowed call's at [lag, lag]"""
    pairs = parity_pairs(n)
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        assert plan.group <= 2
        if plan.layout == "real-column":
            plan.set_pearson(False)
        got = plan.xcorr_ncc_full_f32(src, smp)
        for k in range(3):
            key = ("d", n, k) if k else ("d", n)
            check_pair(got, k, model_of(key, *pairs[k][:2]), curve_of(key, *pairs[k][:2]), (n, k))
            assert int(got[0][k]) == pairs[k][2] < 0
            lag = int(got[0][k])
            assert abs(float(got[1][k]) - oracle.pearson_coefficient(src[k][:n + lag], smp[k][-lag:])) < COEF_TOL
        assert int(got[0][3]) == pairs[3][2][0]
        for k in range(5):
            assert bits(plan.xcorr_ncc_full_f32(src[k], smp[k]), 0) == bits(got, k), k
        back = plan.xcorr_ncc_full_f32(src[::-1].copy(), smp[::-1].copy())
        for k in range(5):
            assert bits(back, 4 - k) == bits(got, k), k
        rows = np.stack([got[0], got[0]], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, rows)
        assert lag.tolist() == got[0].tolist() and ret.tolist() == got[3].tolist()
        assert coef.tobytes() == got[1].tobytes(), (coef, got[1])
        if plan.layout == "real-column":
            plan.set_pearson(True)  # the coefficient is the direct form's whatever the plan's setting
            assert same(plan.xcorr_ncc_full_f32(src, smp), got)


@pytest.mark.parametrize("n", [2049, BIG])
def test_consequences_against_the_ncc_call(mod, n):
    """(a) a row inside [0, N-1]: the NCC call's result for that row; (b) min_overlap = N: the NCC call's result without rows"""
    pairs = [pair_g(n, k) for k in range(4)] + [pair_e(n, 0)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    rows = np.array([(0, n - 1), (5, n // 2), (n // 3, n // 3), (n - 1, n - 1), (0, n - 2)], dtype=np.int64)
    with mod.Plan(n, 2, 0) as plan:
        assert same(plan.xcorr_ncc_full_f32(src, smp, rows, min_overlap=1), plan.xcorr_ncc_f32(src, smp, rows))
        want = plan.xcorr_ncc_f32(src, smp)
        assert all(float(p) > 0 for p in want[2])                     # every pair's NCC result has a competing lag
        assert same(plan.xcorr_ncc_full_f32(src, smp, min_overlap=n), want)
        assert same(plan.xcorr_ncc_f32(src, smp), want)               # the NCC call behind a full-range call: the same bits


def test_broadcast_and_strides(mod, torch):
    """stride 0 for either operand (more than one group: the slot is refilled before each pass) and an overlapping hop: the bits of
    the call on materialised contiguous pairs"""
    n = BIG
    pairs = [pair_d(n, 0), pair_d(n, 1), pair_e(n, 0), pair_g(n, 1)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_ncc_full_f32(np.broadcast_to(src[0], (4, 2 * n)), smp)
        assert same(plan.xcorr_ncc_full_f32(src[0], smp), want)               # one source against four samples, two groups
        assert int(want[0][0]) == pairs[0][2]
        want = plan.xcorr_ncc_full_f32(src, np.broadcast_to(smp[1], (4, n)))
        assert same(plan.xcorr_ncc_full_f32(src, smp[1]), want)               # one sample against four sources
        assert int(want[0][1]) == pairs[1][2]
        hop = 1000
        rec = np.concatenate([np.zeros(2 * hop, np.float32), src[0]])
        wins = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        want = plan.xcorr_ncc_full_f32(wins, np.broadcast_to(smp[0], (3, n)))
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(smp[0].copy()).cuda()
        out = outputs(torch, 3)
        torch.cuda.synchronize()
        plan.xcorr_ncc_full_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, 0, 0, 3, 1e-3, n // 2, *(a.data_ptr() for a in out))
        plan.sync()
        assert [a.cpu().numpy().tobytes() for a in out] == [a.tobytes() for a in want]
        for k in range(3):
            m = model_of(("hop", k), wins[k], smp[0])
            assert int(want[0][k]) == m[1] == pairs[0][2] + (2 - k) * hop, (k, want[0], m)
    # a packed plan transforms a shared track per pair; its moments, staged copy and tables are still the call's
    m = 2049
    ps = [pair_d(m, k) for k in range(3)]
    s, t = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        assert same(plan.xcorr_ncc_full_f32(s[0], t), plan.xcorr_ncc_full_f32(np.broadcast_to(s[0], (3, 2 * m)), t))
        assert same(plan.xcorr_ncc_full_f32(s, t[1]), plan.xcorr_ncc_full_f32(s, np.broadcast_to(t[1], (3, m))))


@pytest.mark.parametrize("n", [2049, BIG])
def test_rows(mod, n):
    pairs = [pair_d(n, 0), pair_e(n, 0), pair_d(n, 1), pair_g(n, 1), pair_d(n, 2)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ld, (le_neg, le_pos) = pairs[0][2], pairs[1][2]
    with mod.Plan(n, 2, 0) as plan:
        alone = [plan.xcorr_ncc_full_f32(src[k], smp[k]) for k in range(5)]
        # the negative side only, straddling zero (fixture E's positive copy: the negative one is left out), the whole range, the two ends
        rows = np.array([(ld - 50, -1), (le_neg + 60, n - 1), (-(n - 1), n - 1), (-(n - 1), -(n - 1)), (n - 1, n - 1)], dtype=np.int64)
        got = plan.xcorr_ncc_full_f32(src, smp, rows)
        check_pair(got, 0, model_of(("d", n), *pairs[0][:2], row=tuple(int(v) for v in rows[0])), curve_of(("d", n), *pairs[0][:2]), "neg")
        assert int(got[0][0]) == ld
        check_pair(got, 1, model_of(("e", n), *pairs[1][:2], row=tuple(int(v) for v in rows[1])), curve_of(("e", n), *pairs[1][:2]), "straddle")
        assert int(got[0][1]) == le_pos
        assert bits(got, 2) == bits(alone[2], 0)
        # the ends: an overlap of one frame is below min_overlap, lag_min comes back with peak 0; lag N-1 is the NCC call's
        assert (int(got[0][3]), float(got[2][3])) == (-(n - 1), 0.0), got
        assert bits(got, 4) == bits(plan.xcorr_ncc_f32(src[4], smp[4], np.array([n - 1, n - 1], dtype=np.int64)), 0)
        # rows that are not rows of this call: (0, NaN, NaN, -2), the neighbours bit for bit what they are alone
        for bad in ((-n, 5), (0, n), (7, 3)):
            rows = np.array([(-(n - 1), n - 1), bad, (-(n - 1), n - 1), bad, (-(n - 1), n - 1)], dtype=np.int64)
            got = plan.xcorr_ncc_full_f32(src, smp, rows)
            for k in (1, 3):
                assert (int(got[0][k]), int(got[3][k])) == (0, -2) and np.isnan(got[1][k]) and np.isnan(got[2][k]), (bad, got)
            for k in (0, 2, 4):
                assert bits(got, k) == bits(alone[k], 0), (bad, k)
        # d_windows == NULL under a plan window: unaffected, and the window is left as it is
        plan.set_lag_window(5, 9)
        assert bits(plan.xcorr_ncc_full_f32(src[0], smp[0]), 0) == bits(alone[0], 0) and plan.lag_window == (5, 9)


def test_min_overlap(mod):
    """the planted overlap just below min_overlap: the planted lag is not returned; just above: it is"""
    n = 2049
    src, smp, planted = pair_d(n)
    m = n + planted
    with mod.Plan(n, 1, 0) as plan:
        got = plan.xcorr_ncc_full_f32(src, smp, min_overlap=m)
        check_pair(got, 0, model_of(("d", n), src, smp, min_overlap=m), curve_of(("d", n), src, smp), "at")
        assert int(got[0][0]) == planted
        got = plan.xcorr_ncc_full_f32(src, smp, min_overlap=m + 1)
        assert int(got[0][0]) != planted and int(got[3][0]) == 0 and float(got[2][0]) < 0.3, got
        assert not -(n - 1) <= int(got[0][0]) < planted              # nothing below the planted overlap competes


def test_no_lag_competes(mod):
    n = 2049
    src, smp, _ = pair_d(n)
    flat = np.full(n, 0.25, dtype=np.float32)
    half = src.copy()
    half[:n] = 0.0
    with mod.Plan(n, 2, 0) as plan:
        base = plan.xcorr_ncc_full_f32(src, smp)
        got = plan.xcorr_ncc_full_f32(np.stack([src, src, np.zeros(2 * n, np.float32)]), np.stack([flat, smp, smp]),
                                      np.array([(-17, 900), (-(n - 1), n - 1), (-5, -5)], dtype=np.int64))
        assert bits(got, 1) == bits(base, 0)
        for k, first in ((0, -17), (2, -5)):
            assert (int(got[0][k]), float(got[2][k]), int(got[3][k])) == (first, 0.0, -1) and np.isnan(got[1][k]), (k, got)
        none = plan.xcorr_ncc_full_f32(src, flat)
        assert (int(none[0][0]), float(none[2][0]), int(none[3][0])) == (-(n - 1), 0.0, -1)
        # the first N frames silent: no negative lag competes, the non-negative ones still do -- the NCC call's answer
        assert same(plan.xcorr_ncc_full_f32(half, smp, min_overlap=1), plan.xcorr_ncc_f32(half, smp))
        assert plan.xcorr_ncc_full_f32(half, smp, np.array([-(n - 1), -1], dtype=np.int64), min_overlap=1)[2][0] == 0.0
    with mod.Plan(1, 1, 0) as plan:
        one = plan.xcorr_ncc_full_f32(np.array([1.0, 2.0], np.float32), np.array([3.0], np.float32))
        assert (int(one[0][0]), float(one[2][0]), int(one[3][0])) == (0, 0.0, -1), one


@pytest.mark.parametrize("n", [2049, BIG])
def test_topk_on_fixture_e(mod, torch, n):
    src, smp, (ln, lp) = pair_e(n)
    other = pair_d(n)
    cv = curve_of(("e", n), src, smp)
    sep = 50
    with mod.Plan(n, 2, 0) as plan:
        # the entries against the model (margins: tests/test_ncc_full.py at the small lengths, asserted here too)
        want = fm.topk(src, smp, 2, sep, cv=cv)
        ok = fm.competing(cv).copy()
        for lag in (ln, lp):
            ok[lag + n - 1 - sep:lag + n + sep] = False
        assert [e[1] for e in want] == [ln, lp] and want[1][3] - float(np.max(np.where(ok, np.abs(cv[0]), -1.0))) >= MARGIN
        got = plan.xcorr_ncc_full_topk_f32(np.stack([src, other[0], src]), np.stack([smp, other[1], smp]), 2, sep)
        for j in range(2):
            check_pair([a[:, j] for a in got], 0, want[j], cv, ("topk", j))
        assert bits(got, 2) == bits(got, 0)                            # another group, the same bits
        # entry 0 against k = 1, bit for bit
        one = plan.xcorr_ncc_full_f32(np.stack([src, other[0]]), np.stack([smp, other[1]]))
        for k in range(2):
            assert [a[k, 0].tobytes() for a in got] == bits(one, k), k
        assert same(plan.xcorr_ncc_full_topk_f32(src, smp, 1, sep), plan.xcorr_ncc_full_f32(src, smp))
        # The rule itself, over the curve the device returns (the debug call's d_c, min_overlap = 1): lags and peaks exactly.  A zone
        # that straddles 0 (a row around zero, whose winner's zone takes lags of both signs); -3 entries (a row of five lags astride
        # zero and a separation that empties it); k = 8 with min_separation = 0.
        d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        d_c = torch.zeros(2 * n - 1, dtype=torch.float32, device="cuda")
        plan.ncc_full_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), 1e-3, 1, d_c.data_ptr(), *(a.data_ptr() for a in outputs(torch)))
        plan.sync()
        keys = np.abs(d_c.cpu().numpy())
        for k, sep2, row in ((3, 30, (-40, 40)), (3, 4, (-2, 2)), (8, 0, None), (4, 3 * n, None), (3, n // 2, (-(n - 1), 0))):
            got = plan.xcorr_ncc_full_topk_f32(src, smp, k, sep2, None if row is None else np.array(row, dtype=np.int64), min_overlap=1)
            want = fm.topk_of_keys(keys, k, sep2, row)
            for j, (status, lag, peak) in enumerate(want):
                mine = (int(got[3][0, j]), int(got[0][0, j]), float(got[2][0, j]))
                if status == 0:
                    assert mine[0] in (0, -1) and mine[1:] == (lag, peak), (k, sep2, row, j, mine, want[j])
                    assert abs(float(got[1][0, j]) - fm.coefficient(src, smp, lag)) < COEF_TOL or mine[0] == -1
                else:
                    assert mine[:2] == (status, 0) and np.isnan(got[1][0, j]) and np.isnan(got[2][0, j]), (k, sep2, row, j, mine)
        want = fm.topk_of_keys(keys, 3, 30, (-40, 40))
        assert any(lag - 30 < 0 < lag + 30 for _, lag, _ in want[:1])           # the first zone does straddle 0
        assert [e[0] for e in fm.topk_of_keys(keys, 3, 4, (-2, 2))] == [0, -3, -3]
        assert [e[0] for e in fm.topk_of_keys(keys, 4, 3 * n, None)] == [0, -3, -3, -3]
        # an invalid row: -2 in all k entries
        got = plan.xcorr_ncc_full_topk_f32(src, smp, 2, sep, np.array([-n, 0], dtype=np.int64))
        assert got[3][0].tolist() == [-2, -2] and np.isnan(got[1][0]).all() and np.isnan(got[2][0]).all()


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("front,gap", [(5, 3), (4, 4)])
def test_edges(mod, torch, poison, front, gap):
    """poisoned surroundings of the tracks (an unaligned layout: the staging kernel's scalar loads; an aligned one: its vector loads)
    and guarded outputs, for all three entry points: the results of the dense call, nothing outside the outputs written"""
    n = 2049
    pairs = [pair_d(n, 0), pair_e(n, 0), pair_d(n, 1)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    kinds = ("int64", "float64", "float64", "int32")
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_ncc_full_f32(src, smp)
        want2 = plan.xcorr_ncc_full_topk_f32(src, smp, 2, 50)
        b_src, o_src, s_src = edges.embed(src, front, 2 * n + gap, poison, torch)
        b_smp, o_smp, s_smp = edges.embed(smp, front, n + gap, poison, torch, back=2 * n)
        before = edges.snapshot(b_src), edges.snapshot(b_smp)
        p_src, p_smp = b_src.data_ptr() + 4 * o_src, b_smp.data_ptr() + 4 * o_smp
        out = [edges.guarded(torch, kind, 3) for kind in kinds]
        torch.cuda.synchronize()
        plan.xcorr_ncc_full_dev(p_src, s_src, p_smp, s_smp, 0, 0, 3, 1e-3, (n + 1) // 2, *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want]
        assert not any(edges.check_guards(w, 3) for w, _ in out)
        out = [edges.guarded(torch, kind, 6) for kind in kinds]
        torch.cuda.synchronize()
        plan.xcorr_ncc_full_topk_dev(p_src, s_src, p_smp, s_smp, 0, 0, 3, 1e-3, (n + 1) // 2, 2, 50, *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want2]
        assert not any(edges.check_guards(w, 6) for w, _ in out)
        # the debug call: one contiguous pair between poison, its curve between guards
        one_s, off_s, _ = edges.embed(src[:1], front, 0, poison, torch)
        one_t, off_t, _ = edges.embed(smp[:1], front, 0, poison, torch, back=2 * n)
        out = [edges.guarded(torch, kind, 1) for kind in kinds]
        whole_c, d_c = edges.guarded(torch, "float32", 2 * n - 1)
        torch.cuda.synchronize()
        plan.ncc_full_debug_c_dev(one_s.data_ptr() + 4 * off_s, one_t.data_ptr() + 4 * off_t, 1e-3, (n + 1) // 2, d_c.data_ptr(),
                                  *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == bits(want, 0)
        assert not edges.check_guards(whole_c, 2 * n - 1) and not any(edges.check_guards(w, 1) for w, _ in out)
        c = d_c.cpu().numpy()
        assert np.isnan(c[:n // 2 - 1]).all() and float(np.nanmax(np.abs(c))) == float(want[2][0])
        assert edges.unchanged(b_src, before[0]) and edges.unchanged(b_smp, before[1])


def test_what_the_call_leaves_alone(mod, torch):
    n = BIG
    pairs = [pair_d(n, 0), pair_d(n, 1), pair_e(n, 0), pair_g(n, 1), pair_g(n, 2)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes)

    with mod.Plan(n, 2, 0) as plan:
        plan.xcorr_batch_f32(src, smp)                                # the counters hold something to begin with
        plan.xcorr_broadcast_f32(src[0], smp)                         # (the broadcast slot is the strided call's, and counted)
        ncc = plan.xcorr_ncc_f32(src, smp)
        before = state(plan)
        first = plan.xcorr_ncc_full_f32(src, smp)
        assert same(plan.xcorr_ncc_full_f32(src, smp), first)         # a second call: the same bits
        for exact, prune in ((False, True), (True, False)):
            plan.set_exact(exact)
            plan.set_prune(prune)
            assert same(plan.xcorr_ncc_full_f32(src, smp), first), (exact, prune)
        plan.set_exact(True)
        plan.set_prune(True)
        plan.xcorr_ncc_full_topk_f32(src[0], smp, 3, 10, np.array([(0, 9), (3, 2), (-9, n - 1), (0, 0), (-n, -n)], dtype=np.int64))
        assert state(plan) == before
        assert same(plan.xcorr_ncc_f32(src, smp), ncc)                # the NCC call: the bits it gave before


def test_refusals(mod, torch):
    n = 2048
    src, smp, _ = pair_d(n)
    d_src = torch.from_numpy(np.concatenate([src, src])).cuda()
    d_smp = torch.from_numpy(np.concatenate([smp, smp])).cuda()
    kinds = ("int64", "float64", "float64", "int32")

    def fresh(count=2):
        return [edges.guarded(torch, kind, count) for kind in kinds]

    def untouched(out, count=2):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, count) and view.cpu().tolist() == [edges.PAYLOAD] * count for whole, view in out)

    with mod.Plan(n, 2, 0) as plan:
        good = (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n)
        cases = [("min_overlap", 1e-3, 0, None), ("min_overlap", 1e-3, n + 1, None), ("min_overlap", 1e-3, -3, None),
                 ("min_energy", 0.0, n, None), ("min_energy", 1.5, n, None), ("min_energy", float("nan"), n, None),
                 ("null", 1e-3, n, 1), ("null", 1e-3, n, 2), ("null", 1e-3, n, 3)]
        for text, energy, overlap, drop in cases:
            out = fresh()
            ptrs = [view.data_ptr() for _, view in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_full_dev(*good, 0, 0, 2, energy, overlap, *ptrs)
            assert untouched(out), (text, energy, overlap, drop)
        for k, sep, text in ((9, 0, "k = 9"), (0, 0, "k = 0"), (2, -1, "min_separation")):
            out = fresh(2 * max(k, 1))
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_full_topk_dev(*good, 0, 0, 2, 1e-3, n, k, sep, *(view.data_ptr() for _, view in out))
            assert untouched(out, 2 * max(k, 1)), (k, sep)
        out = fresh()
        ptrs = [view.data_ptr() for _, view in out]
        with pytest.raises(mod.AsxError, match="null"):
            plan.xcorr_ncc_full_dev(0, 2 * n, d_smp.data_ptr(), n, 0, 0, 2, 1e-3, n, *ptrs)
        assert mod.lib().asx_xcorr_ncc_full_f32_dev(None, *good, None, 0, 2, 1e-3, n, None, None, None, None, None) == -1
        assert mod.lib().asx_xcorr_ncc_full_f32_dev(plan._h, *good, None, 0, 0, 1e-3, n, *ptrs, None) == 0  # batch == 0
        d_c = torch.zeros(2 * n - 1, dtype=torch.float32, device="cuda")
        for energy, overlap, c_ptr, text in ((1e-3, n, 0, "null"), (2.0, n, d_c.data_ptr(), "min_energy"), (1e-3, 0, d_c.data_ptr(), "min_overlap")):
            with pytest.raises(mod.AsxError, match=text):
                plan.ncc_full_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), energy, overlap, c_ptr, *ptrs)
        assert untouched(out)
        # d_lag may be NULL
        plan.xcorr_ncc_full_dev(*good, 0, 0, 2, 1e-3, n // 2, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, 2) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * 2 and out[3][1].cpu().tolist() == [0, 0]
    with mod.Plan(BIG, 1, 0) as plan:   # the layout rule of real-column plans
        big = torch.zeros(2 * BIG + 8, dtype=torch.float32, device="cuda")
        out = fresh(1)
        with pytest.raises(mod.AsxError, match="aligned"):
            plan.xcorr_ncc_full_dev(big.data_ptr() + 4, 2 * BIG, big.data_ptr(), BIG, 0, 0, 1, 1e-3, BIG, *(v.data_ptr() for _, v in out))
        assert untouched(out, 1)
