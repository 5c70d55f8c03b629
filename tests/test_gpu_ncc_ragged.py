"""Ragged normalised cross-correlation on the MI355X (asx_xcorr_ncc_ragged_f32_dev, asx_xcorr_ncc_ragged_topk_f32_dev,
asx_xcorr_ncc_ragged_debug_c_dev) against the float64 model of tests/ncc_ragged_model.py: the whole curve at the plan lengths and
track lengths the chunk arithmetic tells apart, fixtures G and H against the full-range call on the zero-padded pair, poison beyond
the lengths, the plan's own shape against the full-range call, independence of the batch, strides, top-k on fixture K, rows of
lengths that are none, refusals, and a second call that allocates nothing."""
import numpy as np
import pytest

import edges
import ncc_full_model as fm
import ncc_ragged_model as rm
import oracle
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
# max over the competing lags of |d_c - model| * sqrt(Vx[l] Vy[l] / (Vmax Vy)): the error brought to the scale of the loudest window,
# where the error of r32 lives (check_curve, with min_overlap = 1; the model's r is float64).  Measured on an MI355X, the largest over
# the length rows of the generator pair / fixture G: N = 2 3.6e-7 / -, 3 1.2e-7 / -, 1000 6.0e-8 / 1.07e-6, 2047 1.6e-7 / 1.02e-6, 2048
# 1.4e-7 / 1.32e-6, 2049 1.5e-7 / 1.15e-6, 5000 8.5e-8 / 9.1e-7, 144 000 2.5e-8 / - and fixture H 8.5e-7 (the unscaled error: up to 7.5e-6,
# the short overlaps').  Fixtures G and H ride on a DC of 3 next to a level block of 4 in the source: r32 carries Sx Sy / m, some
# tens of times the covariance, and a few of its float32 ulps show at that size.  Asserted at four times the largest value seen,
# 1.32e-6, rounded up to one significant digit; the hard cap is 1e-3.  profiles/ncc/ragged_cost.txt holds the same figures.  Every lag
# assertion below rests on a model margin of at least 0.2 (asserted where the pair's model is formed), so the tolerance cannot hide
# a wrong lag.
RAG_TOL = 6e-6
assert RAG_TOL <= 1e-3
MARGIN = 0.2
SMALL = (1, 2, 3, 1000, 2047, 2048, 2049, 5000)
BIG = 144000   # a real-column plan
KINDS = ("int64", "float64", "float64", "int32")

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pair_s(n, k=0):
    """a generator pair (planted on either side of zero)"""
    return cached(("s", n, k), lambda: oracle.synth_pair(37, n % 7 + k, n, 1)[:2])


def fixture(name, n, p=0):
    return cached((name, n, p), lambda: getattr(rm, "fixture_" + name)(n, p))


def curve_of(key, src, smp, ls, lm):
    """the model's curve of a pair, computed once and never written to"""
    def make():
        cv = rm.curve(src, smp, ls, lm)
        for a in (cv[0], cv[1], cv[4]):
            a.setflags(write=False)
        return cv
    return cached(("curve",) + tuple(key) + (ls, lm), make)


def model_of(key, src, smp, ls, lm, row=None, min_overlap=None):
    """the model's (ret, lag, coef, peak), its |c| MARGIN above every other competing lag of the row"""
    n = smp.size
    cv = curve_of(key, src, smp, ls, lm)
    m = rm.model(src, smp, ls, lm, row=row, min_overlap=min_overlap, cv=cv)
    ok = rm.competing(cv, ls, lm, min_overlap=min_overlap).copy()
    if row is not None:
        ok[:row[0] + n - 1] = False
        ok[row[1] + n:] = False
    assert m[0] == 0 and m[3] - rm.runner_up(cv, ok, m[1]) >= MARGIN, (key, row, m)
    return m


def scale_at(cv, lag):
    n = (cv[0].size + 1) // 2
    return float(np.sqrt(cv[1][lag + n - 1] / (cv[2] * cv[3])))


def poisoned(src, smp, ls, lm, value):
    s, t = src.copy(), smp.copy()
    s[ls:] = value
    t[lm:] = value
    return s, t


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


def debug_curve(plan, torch, src, smp, ls, lm, min_overlap=1):
    n = smp.size
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    d_c = torch.full((2 * n - 1,), 7.0, dtype=torch.float32, device="cuda")
    out = outputs(torch)
    torch.cuda.synchronize()
    plan.ncc_ragged_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), ls, lm, fm.DEFAULT_ENERGY, min_overlap, d_c.data_ptr(),
                                *(a.data_ptr() for a in out))
    plan.sync()
    return d_c.cpu().numpy(), tuple(a.cpu().numpy() for a in out)


def check_curve(what, plan, torch, src, smp, ls, lm):
    """The debug call with min_overlap = 1, NaN beyond the lengths, against the model.  -> the worst scaled error"""
    n = smp.size
    s, t = poisoned(src, smp, ls, lm, np.nan)
    c32, got = debug_curve(plan, torch, s, t, ls, lm)
    cv = curve_of(what, src, smp, ls, lm)
    assert np.isnan(c32[cv[4] <= 0]).all(), what                       # the lags that do not exist
    # the model's competing set but for the lags within a factor 2 of the threshold (the partial overlaps of about 3 % of the window
    # on either side: at most 5 % of the curve)
    ok = rm.competing(cv, ls, lm, min_overlap=1)
    near = rm.near_threshold(cv)
    assert near.sum() <= max(2, 0.05 * c32.size), (what, int(near.sum()))
    sure = ~near
    assert np.array_equal(np.isnan(c32)[sure], ~ok[sure]), (what, np.flatnonzero(sure & (np.isnan(c32) != ~ok))[:8])
    both = ok & ~np.isnan(c32)
    err = scaled = 0.0
    if both.any():
        diff = np.abs(c32[both].astype(np.float64) - cv[0][both])
        err = float(diff.max())
        scaled = float((diff * np.sqrt(cv[1][both] / (cv[2] * cv[3]))).max())
    print("ncc ragged curve", what, "Ls", ls, "Lm", lm, "competing", int(ok.sum()), "of", c32.size, "near the threshold", int(near.sum()),
          "max scaled |d_c - model|", scaled, "unscaled", err)
    # the returned lag: the smallest index of the maximum of |d_c| itself; its coefficient: the oracle's over the shared frames
    lag, coef, peak, ret = (a[0] for a in got)
    mine = np.where(np.isnan(c32), np.float32(-1.0), np.abs(c32))
    if mine.max() >= 0:
        assert int(lag) == int(np.argmax(mine)) - (n - 1) and float(peak) == float(mine.max()), (what, lag, peak, int(np.argmax(mine)))
    else:
        assert (int(lag), float(peak)) == (-(n - 1), 0.0), (what, lag, peak)
    want = rm.coefficient(src, smp, int(lag), ls, lm)
    assert (want != want and coef != coef and int(ret) == -1) or (abs(float(coef) - want) < COEF_TOL and int(ret) == 0), (what, coef, want)
    assert scaled <= RAG_TOL, (what, scaled)
    return scaled


def length_rows(n):
    """the plan's shape, Ls = 1, Lm = 1, Ls < Lm, Ls <= N, and both chunk edges where the tracks are long enough"""
    rows = {(2 * n, n), (1, n), (2 * n, 1), (max(1, n // 2), n), (n, max(1, n - 1)), (max(1, (3 * n) // 2), max(1, (7 * n) // 10))}
    if n >= 2049:
        rows |= {(2047, 2048), (2048, 2049), (2049, 2047), (min(2 * n, 4097), 2048)}
    if n >= 5000:
        rows |= {(4095, 4096), (2 * n - 1, 4097)}
    return sorted(rows)


@pytest.mark.parametrize("n", SMALL)
def test_whole_curve_at_small_lengths_on_packed_plans(mod, torch, n):
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "packed"
        src, smp = pair_s(n)
        for ls, lm in length_rows(n):
            check_curve(("s", n), plan, torch, src, smp, ls, lm)
        if n >= 1000:
            src, smp, ls, lm, _ = fixture("g", n)
            check_curve(("g", n, 0), plan, torch, src, smp, ls, lm)


def test_whole_curve_on_a_real_column_plan(mod, torch):
    n = BIG
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "real-column"
        src, smp = pair_s(n)
        check_curve(("s", n), plan, torch, src, smp, 2 * n, n)
        check_curve(("s", n), plan, torch, src, smp, 100001, 2049)
        src, smp, ls, lm, _ = fixture("h", n)
        check_curve(("h", n, 0), plan, torch, np.nan_to_num(src), np.nan_to_num(smp), ls, lm)


def check_pair(got, k, m, cv, what):
    lag, coef, peak, ret = (a[k] for a in got)
    print("ncc ragged", what, "lag", int(lag), "model", m[1], "peak", float(peak), "model", m[3], "diff", abs(float(peak) - m[3]))
    assert (int(ret), int(lag)) == (m[0], m[1]), (what, lag, coef, peak, ret, m)
    assert abs(float(coef) - m[2]) < COEF_TOL, (what, coef, m)
    assert abs(float(peak) - m[3]) <= RAG_TOL / scale_at(cv, m[1]) + 1e-7, (what, peak, m)


@pytest.mark.parametrize("n", [2049, BIG])
def test_fixtures_g_and_h_need_the_lengths(mod, n):
    """The ragged call returns the planted lag of fixture G (a short sample on an offset) and fixture H (a negative lag, NaN beyond
    both lengths) with the oracle's coefficient; the full-range call on the zero-padded pairs returns other lags.  Three pairs under
    max_batch 2: two groups."""
    fx = [fixture("g", n, 0), fixture("g", n, 1), fixture("h", n, 0)]
    src, smp = np.stack([f[0] for f in fx]), np.stack([f[1] for f in fx])
    lens = np.array([f[2:4] for f in fx], dtype=np.int64)
    mo = n // 4
    with mod.Plan(n, 2, 0) as plan:
        assert plan.group <= 2
        got = plan.xcorr_ncc_ragged_f32(src, smp, lens, min_overlap=mo)
        for k, (name, p) in enumerate((("g", 0), ("g", 1), ("h", 0))):
            s, t, ls, lm, planted = fx[k]
            clean = np.nan_to_num(s), np.nan_to_num(t)
            m = model_of((name, n, p), *clean, ls, lm, min_overlap=mo)
            check_pair(got, k, m, curve_of((name, n, p), *clean, ls, lm), (name, n, p))
            assert int(got[0][k]) == planted and int(got[3][k]) == 0
            assert abs(float(got[1][k]) - rm.coefficient(s, t, planted, ls, lm)) < COEF_TOL
        padded = [rm.padded(*f[:4]) for f in fx]
        far = plan.xcorr_ncc_full_f32(np.stack([q[0] for q in padded]), np.stack([q[1] for q in padded]), min_overlap=mo)
        print("ncc ragged fixtures", n, "planted", [f[4] for f in fx], "ragged", got[0].tolist(), "full-range on the padded pairs", far[0].tolist())
        for k in range(3):
            assert int(far[0][k]) != fx[k][4], (k, far)
        # the coefficient is the direct form's whatever the plan's setting
        if plan.layout == "real-column":
            for pearson, exact, prune in ((False, False, True), (True, True, False)):
                plan.set_pearson(pearson)
                plan.set_exact(exact)
                plan.set_prune(prune)
                assert same(plan.xcorr_ncc_ragged_f32(src, smp, lens, min_overlap=mo), got), (pearson, exact, prune)


@pytest.mark.parametrize("poison", edges.POISONS)
def test_frames_beyond_the_lengths_are_never_read(mod, torch, poison):
    """zeros, NaN or 1e30 at and beyond the lengths: the same bytes, for the one-lag call, the top-k call and the debug call's curve;
    nothing outside the outputs is written"""
    n = 2049
    fx = [fixture("g", n), fixture("h", n), fixture("k", n)]
    lens = np.array([f[2:4] for f in fx] + [(1, n), (2 * n - 1, 1)], dtype=np.int64)
    base = [f[:2] for f in fx] + [pair_s(n), pair_s(n, 1)]
    fill = edges.poison_values(2 * n, poison)
    zero, bad = [], []
    for (s, t), (ls, lm) in zip(base, lens):
        zero.append(poisoned(s, t, ls, lm, 0.0))
        ps, pt = s.copy(), t.copy()
        ps[ls:] = fill[:2 * n - ls]
        pt[lm:] = fill[:n - lm]
        bad.append((ps, pt))
    count = len(base)
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_ncc_ragged_f32(np.stack([z[0] for z in zero]), np.stack([z[1] for z in zero]), lens, min_overlap=n // 4)
        want2 = plan.xcorr_ncc_ragged_topk_f32(np.stack([z[0] for z in zero]), np.stack([z[1] for z in zero]), 2, 20, lens, min_overlap=n // 4)
        assert int(want[0][0]) == fx[0][4] and int(want[0][1]) == fx[1][4] and int(want[0][2]) == fx[2][4][0]
        d_src = torch.from_numpy(np.stack([b[0] for b in bad])).cuda()
        d_smp = torch.from_numpy(np.stack([b[1] for b in bad])).cuda()
        d_len = torch.from_numpy(lens).cuda()
        before = edges.snapshot(d_src), edges.snapshot(d_smp)
        out = [edges.guarded(torch, kind, count) for kind in KINDS]
        torch.cuda.synchronize()
        plan.xcorr_ncc_ragged_dev(d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, d_len.data_ptr(), 1, 0, 0, count, 1e-3, n // 4,
                                  *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want]
        assert not any(edges.check_guards(w, count) for w, _ in out)
        out = [edges.guarded(torch, kind, 2 * count) for kind in KINDS]
        torch.cuda.synchronize()
        plan.xcorr_ncc_ragged_topk_dev(d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, d_len.data_ptr(), 1, 0, 0, count, 1e-3, n // 4, 2, 20,
                                       *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want2]
        assert not any(edges.check_guards(w, 2 * count) for w, _ in out)
        assert edges.unchanged(d_src, before[0]) and edges.unchanged(d_smp, before[1])
        # the debug call: the curve between guards, the same bytes with zeros and with poison
        curves = []
        for s, t in (zero[1], bad[1]):
            d_s, d_t = torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda()
            whole_c, d_c = edges.guarded(torch, "float32", 2 * n - 1)
            out = [edges.guarded(torch, kind, 1) for kind in KINDS]
            torch.cuda.synchronize()
            plan.ncc_ragged_debug_c_dev(d_s.data_ptr(), d_t.data_ptr(), int(lens[1][0]), int(lens[1][1]), 1e-3, n // 4, d_c.data_ptr(),
                                        *(v.data_ptr() for _, v in out))
            plan.sync()
            assert not edges.check_guards(whole_c, 2 * n - 1) and not any(edges.check_guards(w, 1) for w, _ in out)
            assert [v.cpu().numpy().tobytes() for _, v in out] == bits(want, 1)
            curves.append(d_c.cpu().numpy().tobytes())
        assert curves[0] == curves[1]


@pytest.mark.parametrize("n", [2049, BIG])
def test_the_plans_shape_and_null_lengths_against_the_full_range_call(mod, n):
    """rows (2N, N), one row (2N, N) for all pairs and d_lengths == NULL: the same bytes among themselves; the lag and ret of the
    full-range call, its peak within the tolerance"""
    pairs = [fm.fixture_d(n, p)[:2] for p in range(3)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_ncc_full_f32(src, smp)
        got = plan.xcorr_ncc_ragged_f32(src, smp)
        assert same(plan.xcorr_ncc_ragged_f32(src, smp, np.array([(2 * n, n)] * 3, dtype=np.int64)), got)
        assert same(plan.xcorr_ncc_ragged_f32(src, smp, np.array([2 * n, n], dtype=np.int64)), got)
        for k in range(3):
            cv = curve_of(("shape", n, k), *pairs[k], 2 * n, n)
            m = fm.model(*pairs[k])
            ok = fm.competing(fm.curve(*pairs[k]))
            assert m[3] - fm.runner_up(fm.curve(*pairs[k]), ok, m[1]) >= MARGIN, (n, k, m)
            print("ncc ragged (2N, N)", n, k, "lag", int(got[0][k]), "full", int(want[0][k]), "peak", float(got[2][k]), "full", float(want[2][k]))
            assert (int(got[0][k]), int(got[3][k])) == (int(want[0][k]), int(want[3][k])) == (m[1], m[0])
            assert abs(float(got[2][k]) - float(want[2][k])) <= 2 * RAG_TOL / scale_at(cv, m[1]) + 2e-7
            assert got[1][k].tobytes() == want[1][k].tobytes()          # the direct form over the same frames


def test_a_pairs_values_do_not_depend_on_the_batch(mod):
    n = 2049
    fx = [fixture("g", n), fixture("h", n), fixture("k", n)]
    src, smp = np.stack([f[0] for f in fx]), np.stack([f[1] for f in fx])
    lens = np.array([f[2:4] for f in fx], dtype=np.int64)
    with mod.Plan(n, 2, 0) as plan:
        assert plan.group <= 2
        got = plan.xcorr_ncc_ragged_f32(src, smp, lens, min_overlap=n // 4)                   # three pairs: one above a group
        got2 = plan.xcorr_ncc_ragged_topk_f32(src, smp, 3, 20, lens, min_overlap=n // 4)
        for k in range(3):
            assert bits(plan.xcorr_ncc_ragged_f32(src[k], smp[k], lens[k], min_overlap=n // 4), 0) == bits(got, k), k
            assert bits(plan.xcorr_ncc_ragged_topk_f32(src[k], smp[k], 3, 20, lens[k], min_overlap=n // 4), 0) == bits(got2, k), k
        back = plan.xcorr_ncc_ragged_f32(src[::-1].copy(), smp[::-1].copy(), lens[::-1].copy(), min_overlap=n // 4)
        for k in range(3):
            assert bits(back, 2 - k) == bits(got, k), k
        order = [0, 1, 2, 1, 0]
        five = plan.xcorr_ncc_ragged_f32(src[order], smp[order], lens[order], min_overlap=n // 4)
        assert bits(five, 0) == bits(five, 4) == bits(got, 0) and bits(five, 1) == bits(five, 3) == bits(got, 1)
        # whatever the plan's setters say
        for exact in (False, True):
            plan.set_exact(exact)
            assert same(plan.xcorr_ncc_ragged_f32(src, smp, lens, min_overlap=n // 4), got), exact
        plan.set_lag_window(5, 9)
        assert same(plan.xcorr_ncc_ragged_f32(src, smp, lens, min_overlap=n // 4), got) and plan.lag_window == (5, 9)


@pytest.mark.parametrize("n", [2049, BIG])
def test_broadcast_and_strides(mod, torch, n):
    """one source cut four ways (a stride of 0 with per-pair lengths), one sample against many sources, one row of lengths for all
    pairs, and an overlapping hop: the bits of the call on materialised pairs"""
    s, t, ls, lm, planted = fixture("g", n)
    others = [pair_s(n, k) for k in range(3)]
    with mod.Plan(n, 2, 0) as plan:
        lens = np.array([(ls, lm), (2 * n, n), (n, lm), (ls, lm // 2)], dtype=np.int64)
        want = plan.xcorr_ncc_ragged_f32(np.broadcast_to(s, (4, 2 * n)), np.broadcast_to(t, (4, n)), lens)
        assert same(plan.xcorr_ncc_ragged_f32(s, t, lens), want)                      # both tracks shared, four cuts, two groups
        assert int(want[0][0]) == planted and int(want[0][2]) == planted and int(want[0][3]) == planted
        srcs = np.stack([s] + [o[0] for o in others])
        want = plan.xcorr_ncc_ragged_f32(srcs, np.broadcast_to(t, (4, n)), np.array([(ls, lm)] * 4, dtype=np.int64))
        assert same(plan.xcorr_ncc_ragged_f32(srcs, t, np.array([ls, lm], dtype=np.int64)), want)
        assert int(want[0][0]) == planted
        hop = 1000
        rec = np.concatenate([np.zeros(2 * hop, np.float32), s])
        wins = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        want = plan.xcorr_ncc_ragged_f32(wins, np.broadcast_to(t, (3, n)), np.array([ls, lm], dtype=np.int64))
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(t.copy()).cuda()
        d_len = torch.from_numpy(np.array([ls, lm], dtype=np.int64)).cuda()
        out = outputs(torch, 3)
        torch.cuda.synchronize()
        plan.xcorr_ncc_ragged_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, d_len.data_ptr(), 0, 0, 0, 3, 1e-3, (n + 1) // 2,
                                  *(a.data_ptr() for a in out))
        plan.sync()
        assert [a.cpu().numpy().tobytes() for a in out] == [a.tobytes() for a in want]
        assert int(want[0][2]) == planted and int(want[0][1]) == planted + hop


@pytest.mark.parametrize("n", [2049, BIG])
def test_topk_on_fixture_k(mod, n):
    src, smp, ls, lm, (la, lb) = fixture("k", n)
    g = fixture("g", n)
    clean = poisoned(src, smp, ls, lm, 0.0)
    cv = curve_of(("k", n), *clean, ls, lm)
    sep = 20
    with mod.Plan(n, 2, 0) as plan:
        want = rm.topk(*clean, ls, lm, 2, sep, cv=cv)
        ok = rm.competing(cv, ls, lm).copy()
        for lag in (la, lb):
            ok[lag + n - 1 - sep:lag + n + sep] = False
        assert [e[1] for e in want] == [la, lb] and want[1][3] - float(np.max(np.where(ok, np.abs(cv[0]), -1.0))) >= MARGIN
        lens = np.array([(ls, lm), g[2:4], (ls, lm)], dtype=np.int64)
        srcs, smps = np.stack([src, g[0], src]), np.stack([smp, g[1], smp])
        got = plan.xcorr_ncc_ragged_topk_f32(srcs, smps, 2, sep, lens)
        for j in range(2):
            check_pair([a[:, j] for a in got], 0, want[j], cv, ("topk", n, j))
        assert bits(got, 2) == bits(got, 0)                            # another group, the same bits
        # entry 0 against k = 1, bit for bit
        one = plan.xcorr_ncc_ragged_f32(srcs, smps, lens)
        for k in range(3):
            assert [a[k, 0].tobytes() for a in got] == bits(one, k), k
        assert same(plan.xcorr_ncc_ragged_topk_f32(src, smp, 1, sep, lens[0]), plan.xcorr_ncc_ragged_f32(src, smp, lens[0]))
        # -3 behind an empty A_j: a separation that takes the whole curve, and a row of five lags
        got = plan.xcorr_ncc_ragged_topk_f32(src, smp, 3, 3 * n, lens[0])
        assert got[3][0].tolist() == [0, -3, -3] and int(got[0][0, 0]) == la and np.isnan(got[1][0, 1:]).all() and np.isnan(got[2][0, 1:]).all()
        assert got[0][0, 1:].tolist() == [0, 0]
        got = plan.xcorr_ncc_ragged_topk_f32(src, smp, 3, 4, lens[0], np.array([la - 2, la + 2], dtype=np.int64))
        assert got[3][0].tolist() == [0, -3, -3] and int(got[0][0, 0]) == la


def test_rows_of_lengths_that_are_none(mod):
    """-5 rows beside good pairs, which keep their bits; -5 over -2 and in all k entries"""
    n = 2049
    fx = [fixture("g", n), fixture("h", n), fixture("k", n)]
    with mod.Plan(n, 2, 0) as plan:
        alone = [plan.xcorr_ncc_ragged_f32(f[0], f[1], np.array(f[2:4], dtype=np.int64), min_overlap=n // 4) for f in fx]
        alone2 = [plan.xcorr_ncc_ragged_topk_f32(f[0], f[1], 2, 20, np.array(f[2:4], dtype=np.int64), min_overlap=n // 4) for f in fx]
        order = [0, 1, 0, 2, 1, 2]
        src, smp = np.stack([fx[k][0] for k in order]), np.stack([fx[k][1] for k in order])
        for bad in ((0, n), (2 * n + 1, n), (2 * n, n + 1), (2 * n, 0), (-3, 5)):
            lens = np.array([fx[k][2:4] for k in order], dtype=np.int64)
            lens[2], lens[4] = bad, bad
            rows = np.array([(-(n - 1), n - 1)] * 6, dtype=np.int64)
            rows[4] = (-n, 5)                                         # not a row either: -5 all the same
            for w in (None, rows):
                got = plan.xcorr_ncc_ragged_f32(src, smp, lens, w, min_overlap=n // 4)
                got2 = plan.xcorr_ncc_ragged_topk_f32(src, smp, 2, 20, lens, w, min_overlap=n // 4)
                for k in (2, 4):
                    assert (int(got[0][k]), int(got[3][k])) == (0, -5) and np.isnan(got[1][k]) and np.isnan(got[2][k]), (bad, got)
                    assert got2[3][k].tolist() == [-5, -5] and got2[0][k].tolist() == [0, 0], (bad, got2)
                    assert np.isnan(got2[1][k]).all() and np.isnan(got2[2][k]).all()
                for k in (0, 1, 3, 5):
                    assert bits(got, k) == bits(alone[order[k]], 0), (bad, k)
                    assert bits(got2, k) == bits(alone2[order[k]], 0), (bad, k)
        # a row of windows that is none, under good lengths: -2, as in the full-range call
        got = plan.xcorr_ncc_ragged_f32(fx[0][0], fx[0][1], np.array(fx[0][2:4], dtype=np.int64), np.array([-n, 5], dtype=np.int64))
        assert (int(got[0][0]), int(got[3][0])) == (0, -2) and np.isnan(got[1][0]) and np.isnan(got[2][0])
        # the debug call's lengths are judged the same way
        import torch
        d_s, d_t = torch.from_numpy(np.nan_to_num(fx[0][0])).cuda(), torch.from_numpy(np.nan_to_num(fx[0][1])).cuda()
        d_c = torch.zeros(2 * n - 1, dtype=torch.float32, device="cuda")
        out = outputs(torch)
        plan.ncc_ragged_debug_c_dev(d_s.data_ptr(), d_t.data_ptr(), 2 * n + 1, n, 1e-3, 1, d_c.data_ptr(), *(a.data_ptr() for a in out))
        plan.sync()
        assert int(out[3][0]) == -5 and int(out[0][0]) == 0 and bool(torch.isnan(d_c).all())


def test_refusals_and_what_the_call_leaves_alone(mod, torch):
    n = 2048
    src, smp, ls, lm, _ = fixture("g", n)
    d_src = torch.from_numpy(np.concatenate([src, src])).cuda()
    d_smp = torch.from_numpy(np.concatenate([smp, smp])).cuda()
    d_len = torch.from_numpy(np.array([(ls, lm), (ls, lm)], dtype=np.int64)).cuda()

    def fresh(count=2):
        return [edges.guarded(torch, kind, count) for kind in KINDS]

    def untouched(out, count=2):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, count) and view.cpu().tolist() == [edges.PAYLOAD] * count for whole, view in out)

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes, plan.debug_ncc(), plan.debug_ncc_full())

    with mod.Plan(n, 2, 0) as plan:
        plan.xcorr_batch_f32(np.stack([src, src]), np.stack([smp, smp]))          # the counters hold something to begin with
        before = state(plan)
        good = (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n)
        cases = [("min_overlap", 1e-3, 0, None, (d_len.data_ptr(), 1)), ("min_overlap", 1e-3, n + 1, None, (d_len.data_ptr(), 1)),
                 ("min_energy", 0.0, n, None, (d_len.data_ptr(), 1)), ("min_energy", 1.5, n, None, (0, 0)),
                 ("min_energy", float("nan"), n, None, (0, 0)), ("null", 1e-3, n, 1, (d_len.data_ptr(), 1)),
                 ("null", 1e-3, n, 2, (0, 0)), ("null", 1e-3, n, 3, (d_len.data_ptr(), 0)),
                 ("length_stride", 1e-3, n, None, (0, 1)), ("length_stride", 1e-3, n, None, (0, 7))]
        for text, energy, overlap, drop, lens in cases:
            out = fresh()
            ptrs = [view.data_ptr() for _, view in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_ragged_dev(*good, *lens, 0, 0, 2, energy, overlap, *ptrs)
            assert untouched(out), (text, energy, overlap, drop)
            out = fresh(4)
            ptrs = [view.data_ptr() for _, view in out]
            if drop is not None:
                ptrs[drop] = 0
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_ragged_topk_dev(*good, *lens, 0, 0, 2, energy, overlap, 2, 5, *ptrs)
            assert untouched(out, 4), (text, energy, overlap, drop)
        for k, sep, text in ((9, 0, "k = 9"), (0, 0, "k = 0"), (2, -1, "min_separation")):
            out = fresh(2 * max(k, 1))
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_ragged_topk_dev(*good, d_len.data_ptr(), 1, 0, 0, 2, 1e-3, n, k, sep, *(view.data_ptr() for _, view in out))
            assert untouched(out, 2 * max(k, 1)), (k, sep)
        out = fresh()
        ptrs = [view.data_ptr() for _, view in out]
        with pytest.raises(mod.AsxError, match="null"):
            plan.xcorr_ncc_ragged_dev(0, 2 * n, d_smp.data_ptr(), n, d_len.data_ptr(), 1, 0, 0, 2, 1e-3, n, *ptrs)
        assert mod.lib().asx_xcorr_ncc_ragged_f32_dev(None, *good, None, 0, None, 0, 2, 1e-3, n, None, None, None, None, None) == -1
        assert mod.lib().asx_xcorr_ncc_ragged_f32_dev(plan._h, *good, None, 0, None, 0, 0, 1e-3, n, *ptrs, None) == 0  # batch == 0
        d_c = torch.zeros(2 * n - 1, dtype=torch.float32, device="cuda")
        for energy, overlap, c_ptr, text in ((1e-3, n, 0, "null"), (2.0, n, d_c.data_ptr(), "min_energy"), (1e-3, 0, d_c.data_ptr(), "min_overlap")):
            with pytest.raises(mod.AsxError, match=text):
                plan.ncc_ragged_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), ls, lm, energy, overlap, c_ptr, *ptrs)
        assert untouched(out)
        assert state(plan) == before                                  # nothing was launched, allocated or counted
        # d_lag may be NULL
        plan.xcorr_ncc_ragged_dev(*good, d_len.data_ptr(), 1, 0, 0, 2, 1e-3, n // 2, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, 2) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * 2 and out[3][1].cpu().tolist() == [0, 0]
        assert state(plan) == before                                  # a call that ran: no counter, and a set of its own
    with mod.Plan(BIG, 1, 0) as plan:   # the layout rule of real-column plans
        big = torch.zeros(2 * BIG + 8, dtype=torch.float32, device="cuda")
        out = fresh(1)
        with pytest.raises(mod.AsxError, match="aligned"):
            plan.xcorr_ncc_ragged_dev(big.data_ptr() + 4, 2 * BIG, big.data_ptr(), BIG, 0, 0, 0, 0, 1, 1e-3, BIG, *(v.data_ptr() for _, v in out))
        assert untouched(out, 1)


def test_a_second_call_allocates_nothing(mod, torch):
    n = 5000
    src, smp, ls, lm, planted = fixture("g", n)
    lens = np.array([ls, lm], dtype=np.int64)
    with mod.Plan(n, 4, 0) as plan:
        d_src, d_smp, d_len = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda(), torch.from_numpy(lens).cuda()
        out = outputs(torch, 4)

        def call(k):
            if k == 1:
                plan.xcorr_ncc_ragged_dev(d_src.data_ptr(), 0, d_smp.data_ptr(), 0, d_len.data_ptr(), 0, 0, 0, 4, 1e-3, n // 2,
                                          *(a.data_ptr() for a in out))
            else:
                plan.xcorr_ncc_ragged_topk_dev(d_src.data_ptr(), 0, d_smp.data_ptr(), 0, d_len.data_ptr(), 0, 0, 0, 2, 1e-3, n // 2, 2, 9,
                                               *(a.data_ptr() for a in out))
            plan.sync()

        ws = plan.workspace_bytes
        assert plan.debug_ncc_ragged() == (0, 0)
        call(1)
        first = [a.cpu().numpy().copy() for a in out]
        group, held = plan.debug_ncc_ragged()
        # a set of its own, not counted, bounded by its group size: 84N bytes per pair and the small sums
        assert 1 <= group <= plan.group and 84 * n * group <= held <= 90 * n * group and held <= 1 << 30 and plan.workspace_bytes == ws
        call(1)
        call(2)
        call(1)
        assert plan.debug_ncc_ragged() == (group, held) and plan.workspace_bytes == ws
        assert [a.cpu().numpy().tobytes() for a in out] == [a.tobytes() for a in first] and int(first[0][0]) == planted
