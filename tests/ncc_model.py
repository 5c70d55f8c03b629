"""The float64 model of the normalised cross-correlation (asx_xcorr_ncc_f32_dev): the Pearson coefficient c[l] of every lag 0..N-1 in
the form include/audiosync/xcorr_hip.h states, which lags compete, the peak rule, and the returned coefficient through
oracle.pearson_coefficient.  Also the two fixtures on which the raw search picks the wrong lag: A (a level step in the source) and B
(a louder, merely similar decoy).  Plain module: no fixtures, nothing happens on import."""
import numpy as np

import oracle

MIN_ENERGY = 1e-6   # ASX_NCC_MIN_ENERGY, include/audiosync/xcorr_hip.h
DEFAULT_ENERGY = 1e-3


def r_plain(src, smp):
    """r[l] = sum_{n<N} source[l + n] * sample[n] for the lags 0..N-1, in float64: the time-domain sum for short tracks, else the
    oracle's float64 transforms (unnormalised, 2N times the plain sum)"""
    n = smp.size
    if n <= 4096:
        return np.correlate(src.astype(np.float64), smp.astype(np.float64), mode="valid")[:n]
    return np.asarray(oracle.cross_correlation(src, smp, want_results=True)[3], dtype=np.float64)[:n] / (2 * n)


def moments(src, smp):
    """-> (mu, Sx[N], Vx[N], Sy, Vy): the sliding sums of the source on the mu-shifted values, the sample's about its own mean"""
    n = smp.size
    x = src.astype(np.float64)
    y = smp.astype(np.float64)
    mu = x.mean()
    a = x - mu
    e1 = np.concatenate([[0.0], np.cumsum(a)])
    e2 = np.concatenate([[0.0], np.cumsum(a * a)])
    s1 = e1[n:2 * n] - e1[:n]
    s2 = e2[n:2 * n] - e2[:n]
    vx = s2 - s1 * s1 / n
    b = y - y.mean()
    sy1 = b.sum()
    return mu, s1 + n * mu, vx, sy1 + n * y.mean(), float((b * b).sum() - sy1 * sy1 / n)


def curve(src, smp, r=None):
    """-> (c[N] float64, Vx[N], Vy): c[l] = (r[l] - Sx[l] Sy / N) / sqrt(Vx[l] Vy); r: the plain sums of lags 0..N-1, or None"""
    n = smp.size
    r = r_plain(src, smp) if r is None else np.asarray(r, dtype=np.float64)
    mu, sx, vx, sy, vy = moments(src, smp)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (r - sx * sy / n) / np.sqrt(vx * vy)
    return c, vx, vy


def competing(c, vx, vy, min_energy=DEFAULT_ENERGY):
    """the lags that compete: Vy > 0, Vx[l] >= min_energy * Vmax (Vmax over ALL lags), c[l] finite"""
    vmax = np.nanmax(np.maximum(vx, 0.0)) if vx.size else 0.0
    return (vy > 0) & (vx >= min_energy * vmax) & np.isfinite(c)


def ratio_clear(vx, min_energy, factor=2.0):
    """no lag's Vx / Vmax lies within `factor` of the threshold: the competing set cannot depend on the last bits"""
    ratio = vx / np.max(vx)
    return not np.any((ratio > min_energy / factor) & (ratio < min_energy * factor))


def row_ok(lo, hi, n):
    return 0 <= lo <= hi <= n - 1


def model(src, smp, row=None, min_energy=DEFAULT_ENERGY, c=None):
    """-> (ret, lag, coef, peak) of one pair; row: None (every lag 0..N-1) or (lag_min, lag_max); c: curve()'s result, or None.
    The peak is the largest |float32(c)| among the competing lags of the row, the smallest lag among equals."""
    n = smp.size
    lo, hi = (0, n - 1) if row is None else (int(row[0]), int(row[1]))
    if not row_ok(lo, hi, n):
        return -2, 0, float("nan"), float("nan")
    cc, vx, vy = curve(src, smp) if c is None else c
    ok = competing(cc, vx, vy, min_energy)
    key = np.where(ok, np.abs(cc.astype(np.float32)), np.float32(-1.0))[lo:hi + 1]
    if key.size and key.max() >= 0:
        lag = lo + int(np.argmax(key))   # the first of equal maxima
        peak = float(key.max())
    else:
        lag, peak = lo, 0.0
    coef = oracle.pearson_coefficient(src[lag:lag + n], smp)
    return (-1 if coef != coef else 0), lag, coef, peak


def runner_up(c, ok, lag):
    """the largest |c| among the competing lags other than `lag`"""
    a = np.where(ok, np.abs(c), -1.0)
    a[lag] = -1.0
    return float(a.max())


# ---- fixtures: (N, p) -> (source float32 [2N], sample float32 [N], planted lag) ---------------------------------------------------

def fixture_a(n, p):
    """a level step: sample = 0.3 source[L : L + N] + unit noise + 0.5 DC, and the source gets +1.0 from frame 1.2 N on.  r holds
    Sx[l] Sy / N, so the windows that cover the step win the raw search with a coefficient near 0."""
    rng = np.random.default_rng(1000 + p)
    lag = n // 10 + 11 * p
    src = rng.standard_normal(2 * n)
    smp = 0.3 * src[lag:lag + n] + rng.standard_normal(n) + 0.5
    src[(12 * n) // 10:] += 1.0
    return src.astype(np.float32), smp.astype(np.float32), lag


def fixture_b(n, p):
    """loudness: the sample is a motif of N / 4 frames over a low floor; the source holds a quiet copy of the whole sample at L and,
    at frame 1.25 N, a four times louder stretch that is only 0.6-similar to the motif (lag 0.75 N: the decoy)."""
    rng = np.random.default_rng(2000 + p)
    lag = n // 8 + 13 * p
    q = n // 4
    motif = rng.standard_normal(q)
    smp = 0.1 * rng.standard_normal(n)
    smp[n // 2:n // 2 + q] += motif
    src = 0.02 * rng.standard_normal(2 * n)
    src[lag:lag + n] += 0.25 * smp
    at = n + q
    src[at:at + q] += 4.0 * (0.6 * motif + 0.8 * rng.standard_normal(q))
    return src.astype(np.float32), smp.astype(np.float32), lag
