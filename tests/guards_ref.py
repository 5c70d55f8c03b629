"""Float64 references for the guards every result passes through (a plain helper, used by test_guards_ref.py on the CPU and by
test_gpu_peak_guards.py / test_gpu_spectral_inputs.py on the device).

Two shortcuts carry every result (csrc/asx_internal.h, csrc/pearson_spectral.hip):
  * the transforms run in float32, and the lag is still the float64 argmax because every float32 r[k] is within
    B = 4 u log2(F) |source| |sample| of the exact value (u = 2^-24; the device keeps 2 B F as AsxPeakWs::bound2), every lag inside
    that window is listed, and every listed lag is re-evaluated exactly;
  * on real-column plans the Pearson coefficient is built from r[peak], float32 band sums and a first-order error bound
    (asx_spec_pick, es = 16 u) that sends a pair to the direct reduction when it exceeds 1e-5.
Everything here is the plain definition of those quantities in float64 (or exactly, where the check is to the last place), plus the
checks themselves, so that the CPU self-test can show that each check fails on a planted fault.

Limits, each from the code and none from what the device returns:
  16 u        the constant asx_spec_pick charges a band sum with (k_fwd_cols_r: <= 13 roundings on the squares, <= 10 on the sums)
  one ulp     a correctly rounded float64 sum; the double-double accumulation of k_refine_dots adds N 2^-100 of sum |products|
  B / 3 B     see check_list
  2^-10       bound2 and asx_spec_pick's bound are made of float32 norms: sums of positive float32 terms through at most a couple of
              hundred roundings (1.2e-5); one lost column tile of uniform noise moves a norm by 3e-3
What an MI355X returned against them (test_gpu_peak_guards.py, test_gpu_spectral_inputs.py carry the tables): cells at most 2.9 u,
exact values 0.00 ulp (float32 inputs) and 0.33 ulp (doubles), float32 error at most 0.11 B, bound ratios within 1e-7 (bound2) and
2e-5 (the coefficient's bound), |coef - oracle| at most 0.033 of the bound.  The float32 model of the kernel's order below: 2.2 u.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
ES = 16.0 * U                    # what the cell and window checks allow
ES_DEV = 16.0 * 5.9604645e-8     # the same constant as asx_spec_pick spells it
BOUND_C = 4.0                    # ASX_BOUND_C
TOL = 1e-5                       # AsxSpecWs::tol
FAST, CORR, DIRECT = 0, 1, 2     # ASX_PM_*
RATIO_TOL = 2.0 ** -10


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def B64(x, y, F):
    """B = 4 u log2(F) |x| |y| in the plain-sum scale"""
    x, y = f64(x), f64(y)
    return BOUND_C * U * math.log2(F) * math.sqrt(float(np.dot(x, x))) * math.sqrt(float(np.dot(y, y)))


def r64_all(x, y):
    """r[k] = sum_{n<N} x[(n + k) mod 2N] y[n] for every k < 2N (src/cross_correlation.c:159-239), numpy.fft on the float64 inputs"""
    x, y = f64(x), f64(y)
    n = y.size
    t = np.zeros(2 * n)
    t[:n] = y
    return np.fft.irfft(np.fft.rfft(x) * np.conj(np.fft.rfft(t)), 2 * n)


def keys64(r):
    """the reference rule's keys (src/cross_correlation.c:52-67): index 0 competes signed, every other index by fabs"""
    k = np.abs(r)
    k[0] = r[0]
    return k


def exact_r(x, y, k):
    """(r[k], sum |products|) of the circular sum, exactly: Fractions.  float32 inputs: their float64 products are exact and math.fsum
    rounds the sum once; double inputs: integer arithmetic on the mantissas"""
    n = y.size
    idx = (np.arange(n) + int(k)) % (2 * n)
    if x.dtype == np.float32 and y.dtype == np.float32:
        p = f64(x)[idx] * f64(y)
        return Fraction(math.fsum(p)), Fraction(math.fsum(np.abs(p)))
    assert x.dtype == np.float64 and y.dtype == np.float64
    shift = 2200    # every product of two doubles is a multiple of 2^-2148
    tot = tot_abs = 0
    for a, b in zip(x[idx].tolist(), y.tolist()):
        (na, da), (nb, db) = a.as_integer_ratio(), b.as_integer_ratio()
        v = (na * nb) << (shift - (da.bit_length() - 1) - (db.bit_length() - 1))
        tot += v
        tot_abs += abs(v)
    return Fraction(tot, 1 << shift), Fraction(tot_abs, 1 << shift)


def check_exact(val, ref, sum_abs, n):
    """|val - ref| <= 2^-52 |ref| + n 2^-100 sum |products|: one unit in the last place plus the double-double's own rounding.
    -> the error in units of 2^-52 |ref|"""
    val, ref = Fraction(float(val)), Fraction(ref)
    err = abs(val - ref)
    lim = Fraction(1, 2 ** 52) * abs(ref) + n * Fraction(1, 2 ** 100) * Fraction(sum_abs)
    assert err <= lim, "exact value %r against %r: off by %.3g, allowed %.3g" % (float(val), float(ref), float(err), float(lim))
    return float(err / (Fraction(1, 2 ** 52) * abs(ref))) if ref else 0.0


def check_list(listed, key, bp, what=""):
    """The near-tie list is complete and justified.  key: the float64 keys in the plain-sum scale, M their maximum, bp = B as the
    device has it (bound2 / 2F), listed: the lags that were re-evaluated (the float32 argmax alone when refine_n == 0).
    Premise (checked next to this): |r32[k] - r64[k]| <= bp / 2 for every k; the device lists k iff key32(k) >= max32 - 2 bp.
      complete:  key(k) >= M - bp  =>  key32(k) >= M - 1.5 bp >= (max32 - bp / 2) - 1.5 bp = max32 - 2 bp: listed;
      justified: listed  =>  key(k) >= key32(k) - bp / 2 >= max32 - 2.5 bp >= (M - bp / 2) - 2.5 bp = M - 3 bp.
    -> (lags that had to be listed, lags listed)"""
    listed = np.unique(np.asarray(listed, dtype=np.int64))
    m = key.max()
    must = np.nonzero(key >= m - bp)[0]
    missing = np.setdiff1d(must, listed)
    assert missing.size == 0, "%s: %d of %d must-list lags are not listed, first %s" % (what, missing.size, must.size, missing[:8])
    stray = listed[key[listed] < m - 3.0 * bp]
    assert stray.size == 0, "%s: %d of %d listed lags lie under M - 3B, first %s" % (what, stray.size, listed.size, stray[:8])
    return must.size, listed.size


# ---- band cells ------------------------------------------------------------------------------------------------------------------

def cells64(x, M2, T, band_rows):
    """{sum, sq, abs}: [nbands][ntiles] float64 sums over cell (band b, tile t) = rows b band_rows .. (b + 1) band_rows, columns
    t T .. (t + 1) T of the [rows][M2] matrix of x (the sample is N long: only the bands below row M1 exist)"""
    x = f64(x)
    rows = x.size // M2
    assert rows * M2 == x.size and rows % band_rows == 0 and M2 % T == 0
    m = x.reshape(rows // band_rows, band_rows, M2 // T, T)
    return {"sum": m.sum(axis=(1, 3)), "sq": (m * m).sum(axis=(1, 3)), "abs": np.abs(m).sum(axis=(1, 3))}


def model_cells32(x, M2, band_rows, T=16):
    """float32 model of k_fwd_cols_r's summation order (csrc/rlayout.hip) -> (sum, sum of squares), each [nbands][ntiles] float32.
    Four lanes h share a row pair (rows 2m, 2m + 1; lane h holds columns 4h .. 4h + 3 of both); a lane group owns RPQ =
    band_rows / 2 consecutive row pairs.  Squares: a chain of eight fused multiply-adds per row pair (a.w, a.z, a.y, a.x, then
    b.w .. b.x), a balanced tree over the RPQ pairs, the quad sum (v0 + v1) + (v2 + v3).  Plain sums: ((a.x + a.y) + (a.z + a.w)) +
    ((b.x + b.y) + (b.z + b.w)) per pair, added down the pairs in order, the same quad sum."""
    assert T == 16
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, rpq = x.size // M2, band_rows // 2
    m = x.reshape(rows // band_rows, rpq, 2, M2 // T, 4, 4)      # [band][pair i][row a / b][tile][lane h][column]
    f32 = np.float32

    def fma(a, acc):    # float32 fma(a, a, acc): the float64 product is exact
        return (a.astype(np.float64) * a.astype(np.float64) + acc.astype(np.float64)).astype(f32)

    q1 = np.zeros((m.shape[0], m.shape[3], 4), dtype=f32)
    sq = []
    for i in range(rpq):
        a, b = m[:, i, 0], m[:, i, 1]                            # [band][tile][h][column]
        s = (a[..., 3] * a[..., 3]).astype(f32)
        for v in (a[..., 2], a[..., 1], a[..., 0], b[..., 3], b[..., 2], b[..., 1], b[..., 0]):
            s = fma(v, s)
        sq.append(s)
        q1 = q1 + (((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) + ((b[..., 0] + b[..., 1]) + (b[..., 2] + b[..., 3])))
    while len(sq) > 1:                                           # tree_sum<RPQ>
        sq = [sq[j] + sq[j + 1] for j in range(0, len(sq) - 1, 2)] + ([sq[-1]] if len(sq) & 1 else [])

    def quad(v):
        return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    return quad(q1), quad(sq[0])


def check_cells(got_sum, got_sq, ref, es=ES):
    """|sum - sum64| <= 16 u sum |x| and |sumsq - sumsq64| <= 16 u sum x^2 over every cell ([nbands][ntiles] arrays)
    -> the worst of each in units of u"""
    e1 = np.abs(f64(got_sum) - ref["sum"]) / ref["abs"]
    e2 = np.abs(f64(got_sq) - ref["sq"]) / ref["sq"]
    w1, w2 = float(e1.max()), float(e2.max())
    assert w1 <= es, "plain sum of cell %s off by %.2f u of sum |x| (16 u allowed)" % (np.unravel_index(e1.argmax(), e1.shape), w1 / U)
    assert w2 <= es, "sum of squares of cell %s off by %.2f u (16 u allowed)" % (np.unravel_index(e2.argmax(), e2.shape), w2 / U)
    return w1 / U, w2 / U


def device_cells(band, op, nbands_used):
    """Plan.debug_spectral()["band"] -> (sum, sum of squares) of operand op as [nbands_used][ntiles]"""
    c = band[op, :, :nbands_used, :]
    return c[..., 0].T, c[..., 1].T


# ---- segments, window sums, the coefficient's bound ------------------------------------------------------------------------------

def peak_of_lag(lag, n):
    return lag if lag >= 0 else 2 * n + lag


def seg_of(peak, n):
    """make_seg's rule (csrc/xcorr_dev.h; src/cross_correlation.c:256-271) -> (lag, src_off, smp_off, len)"""
    if peak >= n:
        lag = peak % n - n
        return lag, 0, -lag, n + lag
    return peak, peak, 0, n


def window_sums64(x, y, peak):
    """(n, Sx, Sxx, Sy, Syy) over the segments the lag selects"""
    n = y.size
    _, so, mo, ln = seg_of(peak, n)
    a, b = f64(x)[so: so + ln], f64(y)[mo: mo + ln]
    return ln, float(a.sum()), float(np.dot(a, a)), float(b.sum()), float(np.dot(b, b))


def check_window(pick, ref, es=ES):
    """pick: asx_spec_pick's n, Sx, Sxx, Sy, Syy; ref: window_sums64.  n exact, |Sx - Sx64| <= es sqrt(n Sxx64) and |Sxx - Sxx64|
    <= es Sxx64 (the same for y): exactly the terms dSx and dA the bound charges.  -> the four errors in units of their limits"""
    n, sx, sxx, sy, syy = ref
    assert pick["n"] == n, "segment length %r, expected %d" % (pick["n"], n)
    out = []
    for name, got, want, lim in (("Sx", pick["Sx"], sx, es * math.sqrt(n * sxx)), ("Sxx", pick["Sxx"], sxx, es * sxx),
                                 ("Sy", pick["Sy"], sy, es * math.sqrt(n * syy)), ("Syy", pick["Syy"], syy, es * syy)):
        assert abs(got - want) <= lim, "%s = %r against %r: off by %.3g, allowed %.3g" % (name, got, want, abs(got - want), lim)
        out.append(abs(got - want) / lim)
    return out


def spec_bound64(n, sx, sxx, sy, syy, rb):
    """asx_spec_pick's bound (csrc/xcorr_dev.h) in float64 -> (bound, A, B); infinity when A or B is not positive"""
    a, b = sxx - sx * sx / n, syy - sy * sy / n
    if not (a > 0.0 and b > 0.0):
        return math.inf, a, b
    es = ES_DEV
    dsx, dsy = es * math.sqrt(n * sxx), es * math.sqrt(n * syy)
    dc = rb + (abs(sy) * dsx + abs(sx) * dsy) / n
    da, db = es * sxx + 2.0 * abs(sx) / n * dsx, es * syy + 2.0 * abs(sy) / n * dsy
    return dc / math.sqrt(a * b) + 0.5 * (da / a + db / b), a, b


def mode_of(bound, peak, n):
    """the mode asx_spec_pick takes for that bound"""
    ln = seg_of(peak, n)[3]
    if bound <= TOL:
        if peak < n:
            return FAST
        if n - ln < ln:
            return CORR
    return DIRECT


def predict(x, y, lag, F):
    """float64 prediction for a pair whose peak is at `lag` and whose near-ties were not re-evaluated (rb = B)
    -> (bound, mode, window sums)"""
    n = y.size
    peak = peak_of_lag(lag, n)
    w = window_sums64(x, y, peak)
    bound = spec_bound64(*w, B64(x, y, F))[0] if w[0] > 0 else math.inf
    return bound, mode_of(bound, peak, n), w


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def planted(rng, n, lag, gain=0.5, noise=0.25, sign=1.0):
    """test_gpu_pearson_spectral.planted: source = uniform noise; sample[i] = sign * gain * source[i + lag] + noise"""
    big = rng.uniform(-1, 1, 4 * n)
    src = big[n: 3 * n]
    smp = sign * gain * big[n + lag: 2 * n + lag] + noise * rng.uniform(-1, 1, n)
    return src.astype(np.float32), smp.astype(np.float32)


# The sweeps across the tolerance: grids refined (test_guards_ref.py) until each has at least two pairs under 0.9e-5 and two over
# 1.1e-5 in the float64 prediction, at 144 000 and at 960 000.
SWEEPS = {
    "offset": (0.0, 0.15, 0.3, 0.4, 0.5, 0.7, 1.0),          # k sigma added to both tracks
    "surround": (1.0, 1.15, 1.3, 1.6, 2.0, 2.5, 3.0),              # the source outside the matching window, louder by g
    "lag": (0.02, 0.05, 0.1, 0.3, 0.4, 0.45, 0.49),          # a negative lag -f N
}


def sweep_pairs(n, kind):
    """[(parameter, source, sample, lag)] of one sweep, the same pairs wherever it is called"""
    rng = np.random.default_rng([n, sorted(SWEEPS).index(kind)])
    lag0 = n // 3 + 1
    out = []
    for v in SWEEPS[kind]:
        if kind == "offset":
            s, t = planted(rng, n, lag0)
            s, t, lag = (s + np.float32(v * s.std())), (t + np.float32(v * t.std())), lag0
        elif kind == "surround":
            s, t = planted(rng, n, lag0)
            s = s.copy()
            s[:lag0] *= np.float32(v)
            s[lag0 + n:] *= np.float32(v)
            lag = lag0
        else:
            lag = -int(v * n)
            s, t = planted(rng, n, lag)
        out.append((v, np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32), lag))
    return out
