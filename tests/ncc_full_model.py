"""The float64 model of the full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev): the Pearson coefficient c[l] of every
lag -(N-1)..N-1 in the form include/audiosync/xcorr_hip.h states -- tests/ncc_model.py for l >= 0, the prefix / suffix form over the
overlap m = N + l for l < 0 --, which lags compete, the peak rule, the top-k rule over the signed curve, and the returned coefficient
through oracle.pearson_coefficient.  A curve is indexed by i = l + N - 1.  Also fixture D (a planted negative lag that a level step
hides from the raw search) and fixture E (two copies, one on each side of zero).  Plain module: no fixtures, nothing happens on import."""
import numpy as np

import ncc_model
import oracle

DEFAULT_ENERGY = ncc_model.DEFAULT_ENERGY


def default_overlap(n):
    return (n + 1) // 2


def r_low(src, smp):
    """r[l] = sum_n source[n + l] * sample[n] over the overlap, for l = -(N-1)..-1 (index l + N - 1), in float64: the time-domain sum
    for short tracks, else the oracle's float64 transforms on x_lo (the source with its upper half zero: nothing wraps around)"""
    n = smp.size
    if n <= 4096:
        return np.correlate(src[:n].astype(np.float64), smp.astype(np.float64), "full")[:n - 1]
    lo = src.copy()
    lo[n:] = 0
    r = np.asarray(oracle.cross_correlation(lo, smp, want_results=True)[3], dtype=np.float64) / (2 * n)
    return r[n + 1:2 * n]


def curve(src, smp):
    """-> (c[2N-1] float64, e[2N-1], vmax, vy, vx[N]): e[i] = Vx[l] * Vy[l], the product of the two segment energies (l >= 0: Vx[l] *
    Vy); vmax = the maximum of Vx[l] over 0..N-1, vy = the whole sample's Vy, vx = Vx[l] of the lags 0..N-1"""
    n = smp.size
    c_hi, vx, vy = ncc_model.curve(src, smp)
    vmax = float(np.nanmax(np.maximum(vx, 0.0))) if vx.size else 0.0
    x, y = src.astype(np.float64), smp.astype(np.float64)
    mu, my = x.mean(), y.mean()
    a, b = x[:n] - mu, y - my
    m = np.arange(1, n, dtype=np.float64)                      # the overlap of lag l = m - N
    p1, p2 = np.cumsum(a)[:n - 1], np.cumsum(a * a)[:n - 1]
    t1, t2 = np.cumsum(b[::-1])[:n - 1], np.cumsum((b * b)[::-1])[:n - 1]
    sx, vxl = p1 + m * mu, p2 - p1 * p1 / m
    sy, vyl = t1 + m * my, t2 - t1 * t1 / m
    with np.errstate(invalid="ignore", divide="ignore"):
        c_lo = (r_low(src, smp) - sx * sy / m) / np.sqrt(vxl * vyl)
    return np.concatenate([c_lo, c_hi]), np.concatenate([vxl * vyl, vx * vy]), vmax, vy, vx


def competing(cv, min_energy=DEFAULT_ENERGY, min_overlap=None):
    """the lags that compete (index l + N - 1).  l >= 0: the NCC call's rule.  l < 0: m >= min_overlap, Vy > 0, Vx[l] Vy[l] >=
    min_energy Vmax Vy, c[l] finite"""
    c, e, vmax, vy, vx = cv
    n = (c.size + 1) // 2
    mo = default_overlap(n) if min_overlap is None else min_overlap
    ok = np.zeros(c.size, dtype=bool)
    ok[n - 1:] = ncc_model.competing(c[n - 1:], vx, vy, min_energy)
    m = np.arange(1, n)
    ok[:n - 1] = (m >= mo) & (vy > 0) & (e[:n - 1] >= min_energy * vmax * vy) & np.isfinite(c[:n - 1])
    return ok


def near_threshold(cv, min_energy=DEFAULT_ENERGY, factor=2.0):
    """the lags whose energy lies within `factor` of the threshold: the last bits may decide them"""
    c, e, vmax, vy, vx = cv
    thr = min_energy * vmax * vy
    return (e > thr / factor) & (e < thr * factor)


def row_ok(lo, hi, n):
    return -(n - 1) <= lo <= hi <= n - 1


def keys_of(cv, min_energy=DEFAULT_ENERGY, min_overlap=None):
    """|float32(c)| per index, NaN where the lag does not compete"""
    ok = competing(cv, min_energy, min_overlap)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(ok, np.abs(cv[0].astype(np.float32)), np.float32("nan")).astype(np.float32)


def coefficient(src, smp, lag):
    """oracle.pearson_coefficient of the reference's segments at `lag` (src/cross_correlation.c:256-271)"""
    n = smp.size
    return oracle.pearson_coefficient(src[lag:lag + n], smp) if lag >= 0 else oracle.pearson_coefficient(src[:n + lag], smp[-lag:])


def topk_of_keys(keys, k, min_separation, row=None):
    """asx_xcorr_ncc_topk_f32_dev's rule over the signed lags: keys[i] = |c32| of lag i - (N - 1), NaN where the lag does not
    compete (the debug call's d_c in absolute value).  No wrap between N-1 and -(N-1).  -> k entries (status, lag, peak): status 0
    for an entry with a lag, -3 when A_j is empty, -2 for a row that is not a row of the call; lag 0 and a NaN peak with -2 and -3"""
    n = (keys.size + 1) // 2
    nan = float("nan")
    lo, hi = (-(n - 1), n - 1) if row is None else (int(row[0]), int(row[1]))
    if not row_ok(lo, hi, n):
        return [(-2, 0, nan)] * k
    left = np.zeros(keys.size, dtype=bool)          # A_j
    left[lo + n - 1:hi + n] = True
    out = []
    for _ in range(k):
        if not left.any():
            out.append((-3, 0, nan))
            continue
        cand = left & ~np.isnan(keys)
        if cand.any():
            best = np.where(cand, keys, np.float32(-1.0))
            at = int(np.argmax(best))               # the first of equal maxima: the smallest lag
            peak = float(best[at])
        else:
            at, peak = int(np.flatnonzero(left)[0]), 0.0
        out.append((0, at - (n - 1), peak))
        left[max(0, at - min_separation):min(keys.size - 1, at + min_separation) + 1] = False
    return out


def topk(src, smp, k, min_separation, row=None, min_energy=DEFAULT_ENERGY, min_overlap=None, cv=None):
    """-> k entries (ret, lag, coef, peak) of the rule over the float64 model's curve"""
    keys = keys_of(curve(src, smp) if cv is None else cv, min_energy, min_overlap)
    out = []
    for status, lag, peak in topk_of_keys(keys, k, min_separation, row):
        coef = coefficient(src, smp, lag) if status == 0 else float("nan")
        out.append((status if status else (-1 if coef != coef else 0), lag, coef, peak))
    return out


def model(src, smp, row=None, min_energy=DEFAULT_ENERGY, min_overlap=None, cv=None):
    """-> (ret, lag, coef, peak) of one pair"""
    return topk(src, smp, 1, 0, row, min_energy, min_overlap, cv)[0]


def runner_up(cv, ok, lags):
    """the largest |c| among the competing lags other than `lags` (a lag or several)"""
    n = (cv[0].size + 1) // 2
    a = np.where(ok, np.abs(cv[0]), -1.0)
    for lag in np.atleast_1d(lags):
        a[lag + n - 1] = -1.0
    return float(a.max())


# ---- fixtures: (N, p) -> (source float32 [2N], sample float32 [N], planted lag or lags) ----------------------------------------------

def fixture_d(n, p):
    """the sample starts |L| frames before the source: its last N + L frames are 0.6 source[0 : N + L] + 0.8 noise, all of it rides on
    0.5 DC, and the source gets +2.0 from frame 1.2 N on, which wins the raw search"""
    rng = np.random.default_rng(4000 + p)
    lag = -(n // 5 + 7 * p)
    src = rng.standard_normal(2 * n)
    smp = rng.standard_normal(n) + 0.5
    smp[-lag:] = 0.6 * src[:n + lag] + 0.8 * rng.standard_normal(n + lag) + 0.5
    src[(12 * n) // 10:] += 2.0
    return src.astype(np.float32), smp.astype(np.float32), lag


E_GAINS = (0.8, 0.6)   # fixture E: the copy at the negative lag, the copy at the positive lag


def fixture_e(n, p):
    """two copies of the source in one sample: sample[-Ln:] holds 0.8 source[0 : N + Ln], Ln = -(N/4 + 3p), and the whole sample 0.6
    source[Lp : Lp + N], Lp = N/3 + 5p, over 0.5 noise and 0.25 DC; the source gets +2.0 from frame 1.5 N on.  -> the lags, strongest
    first"""
    rng = np.random.default_rng(5000 + p)
    ln, lp = -(n // 4 + 3 * p), n // 3 + 5 * p
    src = rng.standard_normal(2 * n)
    smp = 0.5 * rng.standard_normal(n) + 0.25
    smp += E_GAINS[1] * src[lp:lp + n]
    smp[-ln:] += E_GAINS[0] * src[:n + ln]
    src[(15 * n) // 10:] += 2.0
    return src.astype(np.float32), smp.astype(np.float32), (ln, lp)
