"""What the spectral Pearson form (csrc/pearson_spectral.hip) builds the coefficient from, against float64, on the device's own numbers
(Plan.debug_spectral over asx_plan_debug_spectral; tests/guards_ref.py holds the references and the checks):

  cells        every band x tile cell k_fwd_cols_r leaves: |sum - sum64| <= 16 u sum |x|, |sumsq - sumsq64| <= 16 u sum x^2 -- the es
               asx_spec_pick relies on; bit-identical after a broadcast call (k_bcast_aux) and a pool call (k_pool_resolve)
  window sums  n exact, |Sx - Sx64| <= es sqrt(n Sxx64), |Sxx - Sxx64| <= es Sxx64 (the terms dSx and dA the bound charges), at lags
               that put the window's edges on, next to and far from band borders and 16-byte boundaries (window_share, direct_range)
  header       |r - r64[peak]| <= rb; rb == 0 and r within one ulp of the exact value when the near-ties were re-evaluated
  the bound    is a bound: |coef - oracle| <= device bound + 1e-12 <= 1e-5 + 1e-12 in the spectral modes; a direct pair has a
               reason to be one; the device's bound is the float64 evaluation's within 2^-10; the recorded mode is the pick's
  sweeps       across 1e-5 (offset, louder surround, negative lag): a pair predicted more than 10 % away from the tolerance takes the
               predicted mode, and every pair is within 1e-5 of the oracle

Lengths: 144 000 (M1 = 300, bands of 10 rows), 288 000 (M1 = 600), 480 000 (M1 = 400, bands of 8 rows), 960 000 (the smallest with
the long-track form of k_pearson_prep): the smallest of each k_fwd_cols_r instance and of each prep form.  A forced lag is a
one-lag window of its own (asx_xcorr_windowed_f32_dev).

Measured on an MI355X (printed under -s), next to the limits:
  N         cell sum / squares   window sums     |r - r64| / rb   |coef - oracle| / bound   |bound / bound64 - 1|
            (limit 16 u)         (of the limit)  (limit 1)        (limit 1)                 (limit 2^-10 = 9.8e-4)
  144 000   2.36 u / 2.75 u      0.003           0.015            0.013                     2.0e-5
  288 000   2.44 u / 2.86 u      0.002           0.016            0.014                     8.3e-6
  480 000   2.35 u / 2.68 u      0.002           0.033            0.029                     1.5e-5
  960 000   2.42 u / 2.57 u      0.001           0.027            0.024                     5.7e-6
  sweeps: the device's bound equals the float64 prediction to three digits in all 42 pairs; |coef - oracle| at most 0.012 of the
  bound at 144 000 and 0.033 at 960 000; tonal pair: header r 0.00 ulp from the exact value, bound 9.6e-7 with rb = 0.
"""
import math

import numpy as np
import pytest

import guards_ref as G
import oracle
from util import asx

pytestmark = pytest.mark.gpu

LENGTHS = [144000, 288000, 480000, 960000]


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def shape(mod, n):
    """(M1, M2, T, band_rows, gs = samples per band) of the plan of n, from the planner alone"""
    d, k = mod.planmath_describe(n), mod.planmath_kernels(n)
    assert k["layout"] == "real-column" and d["F"] == 2 * n and k["band_rows"] in (8, 10)
    return d["M1"], d["M2"], d["T"], k["band_rows"], k["band_rows"] * d["M2"]


PLAIN, SRC30, SMP20 = 0, 1, 2      # uniform noise, plain and with an offset of +30 in the source / +20 in the sample


def forced_lags(n, gs):
    """(lag, input kind): band borders and every residue mod 4, small negative lags, a window that holds no whole band, windows that
    hold no aligned quad.  The plain pairs stay in the spectral modes (bound ~0.8e-5), an offset sends a pair to the direct one."""
    return [(0, PLAIN), (n - 1, SRC30), (gs - 1, PLAIN), (gs, SMP20), (gs + 1, PLAIN), (4001, SRC30), (4002, PLAIN), (4003, SMP20),
            (3 * gs + 5, PLAIN), (-1, PLAIN), (-2, SRC30), (-3, PLAIN), (-5, SMP20), (-gs, PLAIN), (-(gs + 1), PLAIN),
            (-(n - gs // 2), SRC30), (-(n - 5), SMP20), (-(n - 2), PLAIN)]


def pair_of(rng, n, lag, kind, noise=0.25):
    s, t = G.planted(rng, n, lag, noise=noise)
    if kind == SRC30:
        s = s + np.float32(30.0)
    if kind == SMP20:
        t = t + np.float32(20.0)
    return s, t


def check_cells_of(ds, src, smp, M2, T):
    """every cell of the source and every existing cell of the sample -> the worst (sum, squares) errors in u"""
    br, nb = ds["band_rows"], ds["nbands"]
    assert nb * br * M2 == src.size and ds["band"].shape == (2, M2 // T, nb, 2)
    a = G.check_cells(*G.device_cells(ds["band"], 0, nb), G.cells64(src, M2, T, br))
    b = G.check_cells(*G.device_cells(ds["band"], 1, nb // 2), G.cells64(smp, M2, T, br))
    return max(a[0], b[0]), max(a[1], b[1])


def segments(src, smp, peak):
    _, so, mo, ln = G.seg_of(peak, smp.size)
    return src[so: so + ln].astype(np.float64), smp[mo: mo + ln].astype(np.float64)


def check_bound_is_a_bound(ds, coef, src, smp, lag, F):
    """the mode's reason and the coefficient against the oracle's at that lag -> (|coef - oracle| / device bound, or None when
    direct; device bound / float64 bound - 1, or None where rb == 0 or a bound is infinite)"""
    n = smp.size
    peak = G.peak_of_lag(lag, n)
    pick = ds["pick"]
    assert ds["mode"] == pick["mode"], (lag, ds["mode"], pick)
    assert ds["seg"]["peak"] == peak and ds["seg"]["lag"] == lag and not ds["direct"], (lag, ds["seg"])
    w = G.window_sums64(src, smp, peak)
    b64, A, B = G.spec_bound64(*w, G.B64(src, smp, F) if ds["rb"] != 0.0 else 0.0)
    tight = None
    if pick["mode"] in (G.FAST, G.CORR):
        a, b = segments(src, smp, peak)
        o_coef = oracle.pearson_coefficient(a, b)
        assert pick["bound"] <= G.TOL, (lag, pick)
        assert abs(coef - o_coef) <= pick["bound"] + 1e-12, (lag, coef, o_coef, pick["bound"])
        tight = abs(coef - o_coef) / pick["bound"]
    else:
        Ad = pick["Sxx"] - pick["Sx"] ** 2 / pick["n"]
        Bd = pick["Syy"] - pick["Sy"] ** 2 / pick["n"]
        assert pick["bound"] > G.TOL or Ad <= 0.0 or Bd <= 0.0 or lag < -n / 2, (lag, pick)
    ratio = None
    if ds["rb"] != 0.0 and math.isfinite(b64) and math.isfinite(pick["bound"]):
        ratio = pick["bound"] / b64 - 1.0
        assert abs(ratio) <= G.RATIO_TOL, (lag, pick["bound"], b64, ratio)
    return tight, ratio


@pytest.mark.parametrize("n", LENGTHS)
def test_cells_window_sums_header_and_bound_at_forced_lags(mod, n):
    M1, M2, T, band_rows, gs = shape(mod, n)
    rng = np.random.default_rng(n + 1)
    cases = forced_lags(n, gs)
    lags = [c[0] for c in cases]
    pairs = [pair_of(rng, n, lag, kind, [0.05, 0.25, 1.0][i % 3]) for i, (lag, kind) in enumerate(cases)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, len(lags), 0) as plan:
        assert plan.layout == "real-column" and plan.split == (M1, M2, T)
        F = plan.fft_len
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, np.array([[l, l] for l in lags], dtype=np.int64))
        assert plan.peak_overflows() == 0 and plan.group >= len(lags)
        states = [plan.debug_spectral(i) for i in range(len(lags))]
        modes = plan.pearson_modes()
    assert sum(modes) == len(lags)
    assert states[0]["band_rows"] == band_rows and states[0]["prep_blocks"] == (4 if gs >= 16384 else 1)
    worst = {"sum": 0.0, "sq": 0.0, "win": 0.0, "r": 0.0, "tight": 0.0, "ratio": 0.0}
    for i, l in enumerate(lags):
        ds, (s, t) = states[i], pairs[i]
        assert (int(lag[i]), int(ret[i])) == (l, 0), (i, l, int(lag[i]), int(ret[i]))
        w1, w2 = check_cells_of(ds, s, t, M2, T)
        peak = G.peak_of_lag(l, n)
        win = G.check_window(ds["pick"], G.window_sums64(s, t, peak))
        # the header: a one-lag window has no near-ties, so r is the float32 transforms' value and rb = B
        a, b = s.astype(np.float64), t.astype(np.float64)
        r64 = float(np.dot(a[(np.arange(n) + peak) % (2 * n)], b))
        assert ds["rb"] > 0.0 and ds["r"] == ds["pick"]["r"] and abs(ds["r"] - r64) <= ds["rb"], (i, l, ds["r"], r64, ds["rb"])
        tight, ratio = check_bound_is_a_bound(ds, float(coef[i]), s, t, l, F)
        for k, v in (("sum", w1), ("sq", w2), ("win", max(win)), ("r", abs(ds["r"] - r64) / ds["rb"]), ("tight", tight or 0.0),
                     ("ratio", abs(ratio or 0.0))):
            worst[k] = max(worst[k], v)
    print("N=%d (M1=%d, bands of %d rows, %d lags, modes %s): cells worst %.2f u (sum) %.2f u (squares); window sums worst %.3f of "
          "their limit; |r - r64| worst %.3f rb; |coef - oracle| worst %.3f of the bound; bound / bound64 - 1 worst %.2e"
          % (n, M1, band_rows, len(lags), modes, worst["sum"], worst["sq"], worst["win"], worst["r"], worst["tight"], worst["ratio"]))
    assert modes[G.FAST] >= 3 and modes[G.CORR] >= 3 and modes[G.DIRECT] >= 3, modes      # every mode has been through the checks


@pytest.mark.parametrize("n", LENGTHS)
def test_cells_do_not_depend_on_the_place_or_the_call(mod, n):
    """the same track's cells have the same bits at batch position 0, at position 3 of 5, behind a broadcast call (source_stride = 0:
    k_bcast_aux copies the slot's cells) and behind a pool call naming the same tracks (k_pool_resolve)"""
    M1, M2, T, band_rows, gs = shape(mod, n)
    rng = np.random.default_rng(n + 2)
    pairs = [pair_of(rng, n, lag, i % 3) for i, lag in enumerate((1234, -777, gs + 3, 5000, -4001))]
    x, y = pair_of(rng, n, 31337, SRC30)                # the pair under test: an offset source, cells of ~4800 and ~144 000
    five_s, five_t = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    five_s[3], five_t[3] = x, y
    with mod.Plan(n, 5, 0) as plan:
        # One lag competes in every call: the cells come from the forward pass whatever is searched, and an offset source against
        # a sample that does not match it (the broadcast and pool calls below) would otherwise fill its near-tie list
        plan.set_lag_window(31337, 31337)
        plan.xcorr_batch_f32(np.stack([x] + [p[0] for p in pairs[:2]]), np.stack([y] + [p[1] for p in pairs[:2]]))
        at0 = plan.debug_spectral(0)
        lag, coef, ret = plan.xcorr_batch_f32(five_s, five_t)
        at3, other = plan.debug_spectral(3), plan.debug_spectral(1)
        assert int(lag[3]) == 31337
        w0, w3 = check_cells_of(at0, x, y, M2, T), check_cells_of(at3, x, y, M2, T)
        check_cells_of(other, five_s[1], five_t[1], M2, T)
        half = at3["nbands"] // 2
        want_x, want_y = at3["band"][0].view(np.uint32), at3["band"][1, :, :half].view(np.uint32)
        assert np.array_equal(at0["band"][0].view(np.uint32), want_x) and np.array_equal(at0["band"][1, :, :half].view(np.uint32), want_y)
        # broadcast: one source for every pair, the pairs' own samples
        plan.xcorr_broadcast_f32(x, five_t)
        for i in (0, 3, 4):
            bc = plan.debug_spectral(i)
            assert np.array_equal(bc["band"][0].view(np.uint32), want_x), i
            if i == 3:
                assert np.array_equal(bc["band"][1, :, :half].view(np.uint32), want_y)
        # ... and one sample for every pair
        plan.xcorr_broadcast_f32(five_s, y)
        bc = plan.debug_spectral(3)
        assert np.array_equal(bc["band"][0].view(np.uint32), want_x) and np.array_equal(bc["band"][1, :, :half].view(np.uint32), want_y)
        # pool: the tracks named by index, in another order
        plan.xcorr_pool_f32(five_s, five_t, pairs=np.array([[1, 1], [3, 3], [3, 0], [0, 3]]))
        for i, (a, b) in enumerate(((1, 1), (3, 3), (3, 0), (0, 3))):
            pl = plan.debug_spectral(i)
            if a == 3:
                assert np.array_equal(pl["band"][0].view(np.uint32), want_x), i
            if b == 3:
                assert np.array_equal(pl["band"][1, :, :half].view(np.uint32), want_y), i
            check_cells_of(pl, five_s[a], five_t[b], M2, T)
        assert plan.peak_overflows() == 0
    print("N=%d: cells of the offset pair worst %.2f u (sum) %.2f u (squares), the same bits in every place" % (n, max(w0[0], w3[0]), max(w0[1], w3[1])))


def test_exact_peak_value_reaches_the_header(mod):
    """a tonal pair at 144 000: the near-ties were re-evaluated, so rb == 0 and r is the winner's exact value within one ulp"""
    from test_gpu_exact_peak import tonal_pairs
    n = 144000
    src, smp = tonal_pairs(n)["tone + weak noise"]
    with mod.Plan(n, 1, 0) as plan:
        lag, coef, ret = plan.xcorr_batch_f32(src[None], smp[None])
        assert plan.peak_overflows() == 0 and int(ret[0]) == 0
        ds, dp = plan.debug_spectral(0), plan.debug_peak(0)
        F = plan.fft_len
    assert dp["refine_n"] >= 2 and ds["rb"] == 0.0 and not ds["direct"]
    peak = G.peak_of_lag(int(lag[0]), n)
    assert ds["seg"]["peak"] == peak
    ref, sa = G.exact_r(src, smp, peak)
    ulp = G.check_exact(ds["r"], ref, sa, n)
    tight, ratio = check_bound_is_a_bound(ds, float(coef[0]), src, smp, int(lag[0]), F)
    print("N=%d tonal pair: %d near-ties, header r %.2f ulp from the exact value, bound %.3g (rb = 0), |coef - oracle| %s of it"
          % (n, dp["refine_n"], ulp, ds["pick"]["bound"], "%.3f" % tight if tight is not None else "-"))


@pytest.mark.parametrize("n", [144000, 960000])
@pytest.mark.parametrize("kind", sorted(G.SWEEPS))
def test_sweep_across_the_tolerance(mod, n, kind):
    pairs = G.sweep_pairs(n, kind)
    src, smp = np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs])
    with mod.Plan(n, len(pairs), 0) as plan:
        F = plan.fft_len
        lag, coef, ret = plan.xcorr_batch_f32(src, smp)
        assert plan.peak_overflows() == 0 and plan.group >= len(pairs)
        states = [plan.debug_spectral(i) for i in range(len(pairs))]
    line, worst, sides = [], 0.0, [0, 0]
    for i, (v, s, t, l) in enumerate(pairs):
        o_ret, o_lag, o_coef = oracle.cross_correlation(s, t)
        assert (o_ret, o_lag) == (0, l) == (int(ret[i]), int(lag[i])), (kind, v, l, o_lag, int(lag[i]))
        assert abs(float(coef[i]) - o_coef) < G.TOL, (kind, v, float(coef[i]), o_coef)
        pred, pmode, _ = G.predict(s, t, l, F)
        ds = states[i]
        tight, ratio = check_bound_is_a_bound(ds, float(coef[i]), s, t, l, F)
        line.append("%g: %.3f/%.3f %s" % (v, pred / G.TOL, ds["pick"]["bound"] / G.TOL, "fcd"[ds["mode"]]))
        worst = max(worst, tight or 0.0)
        if abs(pred / G.TOL - 1.0) > 0.1:
            assert ds["mode"] == pmode, (kind, v, pred, ds["pick"], pmode)
            sides[pred > G.TOL] += 1
    print("N=%d %s (predicted / device bound in 1e-5, mode): %s; |coef - oracle| worst %.3f of the bound" % (n, kind, "  ".join(line), worst))
    assert sides[0] >= 2 and sides[1] >= 2, sides
