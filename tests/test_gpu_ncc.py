"""Normalised cross-correlation on the MI355X (asx_xcorr_ncc_f32_dev, asx_xcorr_ncc_debug_c_dev, Plan.xcorr_ncc_f32) against the
float64 model of tests/ncc_model.py: the whole curve at the lengths the chunk arithmetic tells apart, parity over launch groups, the
fixtures on which the raw search fails, broadcast and overlap, windows, the energy floor, pairs in which no lag competes, scaling, the
state the call must leave alone, refusals."""
import numpy as np
import pytest

import edges
import ncc_model
import oracle
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
# max |d_c - model| over the competing lags (test_whole_curve_*, test_curve_at_production_lengths), the model's r being float64.
# Measured on an MI355X: at N = 144 000 fixture A 1.27e-7, fixture B 1.72e-7, the generator pair 3.1e-8; at N = 960 000 1.82e-7,
# 1.49e-7 and 3.7e-8; the small lengths between 2.3e-8 (N = 5000) and 1.11e-7 (N = 1000); the source with a silent stretch 1.66e-7:
# a few float32 ulps of r32 over sqrt(Vx Vy), and half an ulp of c32 itself (6e-8 near 1).  Asserted at four times the largest value
# seen, 7.3e-7, rounded up to one significant digit (the spread between boxes and pairs); the hard cap is 1e-3.  Every lag assertion
# below rests on a model margin of at least 0.2 (asserted where the pair's model is formed), so neither can hide a wrong lag.
CURVE_TOL = 8e-7
assert CURVE_TOL <= 1e-3
MARGIN = 0.2

# The lengths the kernels' arithmetic tells apart.  A track is cut into chunks of 2048 frames and the lags into blocks of 2048
# (ASX_NCC_CHUNK): 1 and 2 (one block, N = 1: nothing competes), 1000 (one partial block), 2047 / 2048 / 2049 (one below a chunk, a
# multiple: no remainder frames, one above: a second block of one lag and one whole chunk plus a remainder of one frame), 5000 (three
# blocks, two whole chunks per window).  All of them run on packed plans.
SMALL = (1, 2, 1000, 2047, 2048, 2049, 5000)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def synth(n, k):
    """pair k of the generator at length n among those planted at a lag >= 0 (picked on the CPU): (source, sample, planted)"""
    def make():
        found, j = [], 0
        while len(found) <= k:
            p = oracle.synth_pair(91, j, n, 1)
            if p[2] >= 0:
                found.append(p)
            j += 1
        return found[k]
    return cached(("synth", n, k), make)


def parity_pair(n, k):
    """the five pairs of the parity tests: fixtures A and B, then three generator pairs"""
    if k == 0:
        return cached(("a", n), lambda: ncc_model.fixture_a(n, 0))
    if k == 1:
        return cached(("b", n), lambda: ncc_model.fixture_b(n, 0))
    return synth(n, k - 2)


def curve_of(key, src, smp):
    """the model's (c, Vx, Vy) of a pair, computed once and never written to"""
    def make():
        cv = ncc_model.curve(src, smp)
        for a in cv[:2]:
            a.setflags(write=False)
        return cv
    return cached(("curve",) + key, make)


def model_of(key, src, smp, row=None, min_energy=ncc_model.DEFAULT_ENERGY, margin=True):
    """the model's (ret, lag, coef, peak); margin: its |c| stands MARGIN above every other competing lag of the row"""
    cv = curve_of(key, src, smp)
    m = ncc_model.model(src, smp, row=row, min_energy=min_energy, c=cv)
    if margin and m[0] == 0:
        ok = ncc_model.competing(*cv, min_energy)
        if row is not None:
            ok = ok.copy()
            ok[:row[0]] = False
            ok[row[1] + 1:] = False
        assert m[3] - ncc_model.runner_up(cv[0], ok, m[1]) >= MARGIN, (key, row, m)
    return m


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


def debug_curve(plan, torch, src, smp, min_energy=ncc_model.DEFAULT_ENERGY):
    """-> (d_c float32 [N], (lag, coef, peak, ret)) of the debug call"""
    n = smp.size
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    d_c = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    out = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    plan.ncc_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), min_energy, d_c.data_ptr(), *(a.data_ptr() for a in out))
    plan.sync()
    return d_c.cpu().numpy(), tuple(a.cpu().numpy() for a in out)


def check_curve(what, c32, got, cv, min_energy=ncc_model.DEFAULT_ENERGY, band=False):
    """d_c against the model: the same competing set (band: but for the lags within a factor 2 of the threshold), |d_c - model| <=
    CURVE_TOL over it; the returned lag is the smallest index of the maximum of |d_c| itself and peak that value.  -> the worst error"""
    c, vx, vy = cv
    ok = ncc_model.competing(c, vx, vy, min_energy)
    if band:
        ratio = vx / np.max(vx)
        sure = ~((ratio > min_energy / 2) & (ratio < min_energy * 2))
    else:
        sure = np.ones(c.size, dtype=bool)
        assert c.size == 1 or not ok.any() or ncc_model.ratio_clear(vx, min_energy), what
    assert np.array_equal(np.isnan(c32)[sure], ~ok[sure]), (what, np.flatnonzero(np.isnan(c32) != ~ok)[:8])
    both = ok & ~np.isnan(c32)
    err = float(np.max(np.abs(c32[both].astype(np.float64) - c[both]))) if both.any() else 0.0
    print("ncc curve", what, "competing", int(ok.sum()), "of", c.size, "max |d_c - model|", err)
    lag, coef, peak, ret = (a[0] for a in got)
    mine = np.where(np.isnan(c32), np.float32(-1.0), np.abs(c32))
    if mine.max() >= 0:
        assert int(lag) == int(np.argmax(mine)) and float(peak) == float(mine.max()), (what, lag, peak, int(np.argmax(mine)), mine.max())
    else:
        assert (int(lag), float(peak)) == (0, 0.0), (what, lag, peak)
    assert err <= CURVE_TOL, (what, err)
    return err


@pytest.mark.parametrize("n", SMALL)
def test_whole_curve_at_small_lengths_on_packed_plans(mod, torch, n):
    src, smp, _ = oracle.synth_pair(31, n % 7, n, 1)
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "packed"
        c32, got = debug_curve(plan, torch, src, smp)
    cv = curve_of(("small", n), src, smp)
    check_curve(("small", n), c32, got, cv)
    m = ncc_model.model(src, smp, c=cv)
    assert int(got[3][0]) == m[0]
    if n == 1:
        assert int(got[0][0]) == 0 and float(got[2][0]) == 0.0 and int(got[3][0]) == -1 and np.isnan(got[1][0]) and np.isnan(c32[0])
    else:
        lag = int(got[0][0])                                          # (a weak peak may have a rival inside the curve's resolution)
        assert abs(float(got[2][0]) - m[3]) <= CURVE_TOL
        assert abs(float(got[1][0]) - oracle.pearson_coefficient(src[lag:lag + n], smp)) < COEF_TOL


@pytest.mark.parametrize("n", [144000, 960000])
def test_curve_at_production_lengths(mod, torch, n):
    """the debug call on fixtures A and B and a generator pair: what CURVE_TOL is measured on"""
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "real-column"
        for k in (0, 1, 2):
            src, smp, planted = parity_pair(n, k)
            c32, got = debug_curve(plan, torch, src, smp)
            check_curve((n, k), c32, got, curve_of((n, k), src, smp))
            assert int(got[0][0]) == planted


def check_pair(got, k, m, what):
    lag, coef, peak, ret = (a[k] for a in got)
    print("ncc", what, "lag", int(lag), "model", m[1], "peak", float(peak), "model", m[3], "diff", abs(float(peak) - m[3]))
    assert (int(ret), int(lag)) == (m[0], m[1]), (what, lag, coef, peak, ret, m)
    assert abs(float(coef) - m[2]) < COEF_TOL, (what, coef, m)
    assert abs(float(peak) - m[3]) <= CURVE_TOL, (what, peak, m)
    assert abs(float(peak) - abs(float(coef))) <= CURVE_TOL, (what, peak, coef)


@pytest.mark.parametrize("n", [144000, 480000, 960000])
def test_parity_over_several_launch_groups(mod, n):
    """480-point rows, 1200-point rows, the two-half form; max_batch 2 and five pairs: three launch groups"""
    pairs = [parity_pair(n, k) for k in range(5)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        plan.set_pearson(False)
        got = plan.xcorr_ncc_f32(src, smp)
        for k in range(5):
            check_pair(got, k, model_of((n, k), *pairs[k][:2]), (n, k))
            assert int(got[0][k]) == pairs[k][2]
        rows = np.stack([got[0], got[0]], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, rows)
        assert lag.tolist() == got[0].tolist() and ret.tolist() == got[3].tolist()
        assert coef.tobytes() == got[1].tobytes(), (coef, got[1])
        plan.set_pearson(True)  # the coefficient is the direct form's whatever the plan's setting
        assert same(plan.xcorr_ncc_f32(src, smp), got)


def test_parity_600_row_columns(mod):
    n = 1440000
    src, smp, planted = parity_pair(n, 2)
    with mod.Plan(n, 1, 0) as plan:
        got = plan.xcorr_ncc_f32(src, smp)
    check_pair(got, 0, model_of((n, 2), src, smp), (n, 2))
    assert int(got[0][0]) == planted


def test_the_point_of_the_call(mod):
    """on both fixtures the raw search over the same lags returns the wrong lag and the normalised one the planted lag"""
    n = 144000
    pairs = [parity_pair(n, k) for k in (0, 1)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        raw = plan.xcorr_windowed_f32(src, smp, np.array([0, n - 1], dtype=np.int64))
        got = plan.xcorr_ncc_f32(src, smp)
    for k in (0, 1):
        print("fixture", "ab"[k], "planted", pairs[k][2], "raw", int(raw[0][k]), "coef", float(raw[1][k]), "ncc", int(got[0][k]),
              "coef", float(got[1][k]))
        assert int(raw[2][k]) == 0 and int(raw[0][k]) != pairs[k][2]
        assert int(got[0][k]) == pairs[k][2] and int(got[3][k]) == 0
        assert abs(float(got[1][k])) > abs(float(raw[1][k])) + MARGIN


def test_broadcast_and_strides(mod, torch):
    """stride 0 for either operand and an overlapping hop: the bits of the call on materialised contiguous pairs"""
    n = 144000
    pairs = [parity_pair(n, k) for k in (1, 2, 3, 4)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_ncc_f32(np.broadcast_to(src[0], (4, 2 * n)), smp)
        assert same(plan.xcorr_ncc_f32(src[0], smp), want)               # one source against four samples
        assert int(want[0][0]) == pairs[0][2]
        want = plan.xcorr_ncc_f32(src, np.broadcast_to(smp[1], (4, n)))
        assert same(plan.xcorr_ncc_f32(src, smp[1]), want)               # one sample against four sources
        assert int(want[0][1]) == pairs[1][2]
        hop = 1000
        rec = np.concatenate([src[2], src[0][:2 * hop]])
        wins = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        want = plan.xcorr_ncc_f32(wins, np.broadcast_to(smp[2], (3, n)))
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(smp[2].copy()).cuda()
        out = (torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda"),
               torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_ncc_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, 0, 0, 3, 1e-3, *(a.data_ptr() for a in out))
        plan.sync()
        assert [a.cpu().numpy().tobytes() for a in out] == [a.tobytes() for a in want]
        assert pairs[2][2] >= 2 * hop and want[0].tolist() == [pairs[2][2] - k * hop for k in range(3)], want[0]
    # a packed plan transforms a shared track per pair; its moments are still the call's
    m = 2049
    ps = [synth(m, k) for k in range(3)]
    s, t = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        assert same(plan.xcorr_ncc_f32(s[0], t), plan.xcorr_ncc_f32(np.broadcast_to(s[0], (3, 2 * m)), t))
        assert same(plan.xcorr_ncc_f32(s, t[1]), plan.xcorr_ncc_f32(s, np.broadcast_to(t[1], (3, m))))


def test_windows(mod):
    n = 144000
    pairs = [parity_pair(n, k) for k in range(5)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    planted = [p[2] for p in pairs]
    with mod.Plan(n, 2, 0) as plan:
        free = plan.xcorr_ncc_f32(src, smp)
        alone = [plan.xcorr_ncc_f32(src[k], smp[k]) for k in range(5)]
        for k in range(5):
            assert bits(free, k) == bits(alone[k], 0), k
        # a valid row that holds the planted lag, one that leaves it out (the model's answer there has no margin to speak of: only
        # the rule is checked, on the curve the device itself would return, through the windowed model within CURVE_TOL of its peak)
        rows = np.array([(planted[0] - 5, planted[0] + 900), (planted[1], planted[1]), (0, n - 1), (planted[3] + 1, n - 1),
                         (0, planted[4])], dtype=np.int64)
        got = plan.xcorr_ncc_f32(src, smp, rows)
        for k in (0, 1, 2, 4):
            check_pair(got, k, model_of((n, k), *pairs[k][:2], row=tuple(int(v) for v in rows[k])), ("row", k))
            assert int(got[0][k]) == planted[k]
        assert bits(got, 2) == bits(free, 2)
        lo, hi = (int(v) for v in rows[3])
        m = model_of((n, 3), *pairs[3][:2], row=(lo, hi), margin=False)
        assert lo <= int(got[0][3]) <= hi and int(got[3][3]) == 0 and abs(float(got[2][3]) - m[3]) <= CURVE_TOL, (got, m)
        # rows that are not windows of this call: (0, NaN, NaN, -2), the other pairs bit for bit what they are alone
        for bad in ((-1, 5), (0, n), (7, 3)):
            rows = np.array([(0, n - 1), bad, (0, n - 1), bad, (0, n - 1)], dtype=np.int64)
            got = plan.xcorr_ncc_f32(src, smp, rows)
            for k in (1, 3):
                assert (int(got[0][k]), int(got[3][k])) == (0, -2) and np.isnan(got[1][k]) and np.isnan(got[2][k]), (bad, got)
            for k in (0, 2, 4):
                assert bits(got, k) == bits(alone[k], 0), (bad, k)
        # d_windows == NULL under a plan window that holds no lag of this call: unaffected, and the window is left as it is
        plan.set_lag_window(-n, -1)
        assert same(plan.xcorr_ncc_f32(src, smp), free) and plan.lag_window == (-n, -1)


def test_energy_floor_keeps_silence_out(mod, torch):
    """more than N consecutive zero frames in the source: the lags whose window is silent are NaN in d_c and never win"""
    n = 5000
    rng = np.random.default_rng(5)
    src = rng.standard_normal(2 * n)
    z0, planted = 2000, 50
    src[z0:z0 + n + 600] = 0.0
    smp = src[planted:planted + n] + 0.5 * rng.standard_normal(n)
    src, smp = src.astype(np.float32), smp.astype(np.float32)
    m = model_of(("zeros",), src, smp)
    assert m[:2] == (0, planted)
    with mod.Plan(n, 1, 0) as plan:
        c32, got = debug_curve(plan, torch, src, smp)
        check_curve(("zeros",), c32, got, curve_of(("zeros",), src, smp), band=True)
        assert np.isnan(c32[z0:z0 + 600]).all() and not np.isnan(c32[:z0 - 100]).any()
        check_pair(got, 0, m, ("zeros",))
        # a window of nothing but silent lags: none competes, the row's lag_min comes back
        out = plan.xcorr_ncc_f32(src, smp, np.array([z0 + 10, z0 + 500], dtype=np.int64))
        assert (int(out[0][0]), float(out[2][0]), int(out[3][0])) == (z0 + 10, 0.0, -1) and np.isnan(out[1][0]), out


def test_energy_floor_decides_between_a_quiet_exact_copy_and_a_loud_noisy_one(mod):
    """the sample times 1e-3 sits exactly in an otherwise loud source, between two spikes that lift the neighbouring windows over
    both thresholds at once; a loud noisy copy of its second half (times 0.5, as loud as the rest of the source) sits behind it.  min_energy = 1e-6 lets the exact copy win with
    c = 1, 1e-3 keeps it out and the noisy copy wins."""
    n = 5000
    rng = np.random.default_rng(6)
    smp = 2.0 * rng.standard_normal(n)
    src = rng.standard_normal(2 * n)
    la, lb = 1, n // 2
    src[la:la + n] = 1e-3 * smp
    src[la - 1] = src[la + n] = 8.0
    src[la + n + 1:lb + n] = 0.5 * smp[la + n + 1 - lb:] + 0.15 * rng.standard_normal(lb - la - 1)
    smp = smp.astype(np.float32)
    src = src.astype(np.float32)
    src[la:la + n] = np.float32(1e-3) * smp
    cv = curve_of(("quiet",), src, smp)
    assert ncc_model.ratio_clear(cv[1], 1e-6) and ncc_model.ratio_clear(cv[1], 1e-3)
    low = model_of(("quiet",), src, smp, min_energy=1e-6)
    high = model_of(("quiet",), src, smp, min_energy=1e-3)
    assert low[:2] == (0, la) and high[:2] == (0, lb) and low[3] > 0.999, (low, high)
    # what the float32 error of r may move the quiet window's coefficient by: the 2e-5 of max |r| that tests/test_gpu_parity.py holds
    # r to, over sqrt(Vx Vy) of that window
    slack = 2e-5 * float(np.max(np.abs(ncc_model.r_plain(src, smp)))) / float(np.sqrt(cv[1][la] * cv[2])) + CURVE_TOL
    assert slack < 0.05, slack
    with mod.Plan(n, 1, 0) as plan:
        got = plan.xcorr_ncc_f32(src, smp, min_energy=1e-6)
        print("ncc quiet copy: peak", float(got[2][0]), "model", low[3], "allowed", slack)
        assert (int(got[0][0]), int(got[3][0])) == (la, 0) and abs(float(got[2][0]) - low[3]) <= slack, (got, low)
        assert abs(float(got[1][0]) - low[2]) < COEF_TOL
        check_pair(plan.xcorr_ncc_f32(src, smp, min_energy=1e-3), 0, high, ("quiet", 1e-3))
        check_pair(plan.xcorr_ncc_f32(src, smp), 0, high, ("quiet", "default"))


def test_no_lag_competes(mod):
    n = 144000
    src, smp, _ = parity_pair(n, 2)
    flat = np.full(n, 0.25, dtype=np.float32)
    with mod.Plan(n, 2, 0) as plan:
        base = plan.xcorr_ncc_f32(src, smp)
        got = plan.xcorr_ncc_f32(np.stack([src, src, np.zeros(2 * n, np.float32)]), np.stack([flat, smp, smp]),
                                 np.array([(17, 900), (0, n - 1), (n - 1, n - 1)], dtype=np.int64))
        assert bits(got, 1) == bits(base, 0)
        for k, first in ((0, 17), (2, n - 1)):
            assert (int(got[0][k]), float(got[2][k]), int(got[3][k])) == (first, 0.0, -1) and np.isnan(got[1][k]), (k, got)
        none = plan.xcorr_ncc_f32(src, flat)
        assert (int(none[0][0]), float(none[2][0]), int(none[3][0])) == (0, 0.0, -1)


def test_scale(mod):
    """source times 2^10 and sample times 2^-7 (exact in float32): the same lag, the peak within CURVE_TOL"""
    n = 144000
    pairs = [parity_pair(n, k) for k in range(3)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 2, 0) as plan:
        base = plan.xcorr_ncc_f32(src, smp)
        got = plan.xcorr_ncc_f32(src * np.float32(2.0 ** 10), smp * np.float32(2.0 ** -7))
    assert got[0].tolist() == base[0].tolist() == [p[2] for p in pairs] and got[3].tolist() == [0, 0, 0]
    for k in range(3):
        m = model_of((n, k), *pairs[k][:2])
        print("ncc scaled", k, "peak", float(got[2][k]), "model", m[3], "diff", abs(float(got[2][k]) - m[3]))
        assert abs(float(got[2][k]) - m[3]) <= CURVE_TOL and abs(float(got[1][k]) - m[2]) < COEF_TOL


def test_what_the_call_leaves_alone(mod, torch):
    n = 144000
    pairs = [parity_pair(n, k) for k in range(5)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()

    def plain(plan):
        out = (torch.zeros(5, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"),
               torch.zeros(5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), 5, *(a.data_ptr() for a in out))
        plan.sync()
        return [a.cpu().numpy().tobytes() for a in out]

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes)

    with mod.Plan(n, 2, 0) as fresh:
        want_plain = plain(fresh)
    with mod.Plan(n, 2, 0) as plan:
        plain(plan)                                                   # the counters hold something to begin with
        plan.xcorr_broadcast_f32(src[0], smp)                         # (the broadcast slot is the strided call's, and counted)
        before = state(plan)
        assert before[2] != (0, 0, 0) and before[3][1] > 0, before
        first = plan.xcorr_ncc_f32(src, smp)
        assert same(plan.xcorr_ncc_f32(src, smp), first)              # a second call: the same bits
        for exact, prune in ((False, True), (True, False), (False, False)):
            plan.set_exact(exact)
            plan.set_prune(prune)
            assert same(plan.xcorr_ncc_f32(src, smp), first), (exact, prune)
        plan.set_exact(True)
        plan.set_prune(True)
        plan.set_lag_window(100, 5000)
        assert same(plan.xcorr_ncc_f32(src, smp), first) and plan.lag_window == (100, 5000)
        plan.set_lag_window(-n, n - 1)
        plan.xcorr_ncc_f32(src[0], smp, np.array([(0, 9), (3, 2), (0, n - 1), (0, 0), (-n, -n)], dtype=np.int64))
        assert state(plan) == before
        assert plain(plan) == want_plain


def test_refusals(mod, torch):
    n = 144000
    src, smp, _ = parity_pair(n, 2)
    d_src = torch.from_numpy(np.concatenate([src, src, src[:8]])).cuda()
    d_smp = torch.from_numpy(np.concatenate([smp, smp])).cuda()
    kinds = ("int64", "float64", "float64", "int32")

    def outputs():
        return [edges.guarded(torch, kind, 2) for kind in kinds]

    def untouched(out):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, 2) and view.cpu().tolist() == [edges.PAYLOAD] * 2 for whole, view in out)

    with mod.Plan(n, 2, 0) as plan:
        good = (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n)
        cases = [("null", good, 1e-3, 1), ("null", good, 1e-3, 2), ("null", good, 1e-3, 3),
                 ("null", (0, 2 * n, d_smp.data_ptr(), n), 1e-3, None), ("null", (d_src.data_ptr(), 2 * n, 0, n), 1e-3, None),
                 ("aligned", (d_src.data_ptr() + 4, 2 * n, d_smp.data_ptr(), n), 1e-3, None),
                 ("multiples of 4", (d_src.data_ptr(), 6, d_smp.data_ptr(), n), 1e-3, None),
                 ("min_energy", good, 0.0, None), ("min_energy", good, 1e-7, None), ("min_energy", good, 1.5, None),
                 ("min_energy", good, float("nan"), None)]
        for text, (ps, ss, pm, ms), energy, drop in cases:
            out = outputs()
            ptrs = [view.data_ptr() for _, view in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_dev(ps, ss, pm, ms, 0, 0, 2, energy, *ptrs)
            assert untouched(out), (text, energy, drop)
        assert mod.lib().asx_xcorr_ncc_f32_dev(None, d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, None, 0, 2, 1e-3, None,
                                               None, None, None, None) == -1
        out = outputs()
        ptrs = [view.data_ptr() for _, view in out]
        assert mod.lib().asx_xcorr_ncc_f32_dev(plan._h, *good, None, 0, 0, 1e-3, *ptrs, None) == 0  # batch == 0
        assert untouched(out)
        d_c = torch.zeros(n, dtype=torch.float32, device="cuda")
        for energy, c_ptr, text in ((1e-3, 0, "null"), (2.0, d_c.data_ptr(), "min_energy")):
            with pytest.raises(mod.AsxError, match=text):
                plan.ncc_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), energy, c_ptr, *ptrs)
            assert untouched(out), text
        # d_lag may be NULL
        plan.xcorr_ncc_dev(*good, 0, 0, 2, 1e-3, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, 2) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * 2 and out[3][1].cpu().tolist() == [0, 0]
