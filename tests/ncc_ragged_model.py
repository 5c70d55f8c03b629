"""The float64 model of the ragged normalised cross-correlation (asx_xcorr_ncc_ragged_f32_dev): a pair whose source holds Ls <= 2N
frames and whose sample holds Lm <= N, the Pearson coefficient c[l] of every lag -(N-1)..N-1 over the frames the two really share
there, in the form include/audiosync/xcorr_hip.h states (prefix sums about the means of the frames that count), which lags compete,
the peak rule, the top-k rule (tests/ncc_full_model.py's, over the same signed curve) and the returned coefficient through
oracle.pearson_coefficient.  A curve is indexed by i = l + N - 1.  Frames at and beyond a length are never read.  Also fixture G (a
short sample on an offset, which zero padding turns into a pulse that a level block in the source attracts), fixture H (a planted
negative lag, NaN beyond both lengths) and fixture K (two copies of a short sample).  Plain module: no fixtures, nothing happens on
import."""
import numpy as np

import ncc_full_model as fm
import oracle

DEFAULT_ENERGY = fm.DEFAULT_ENERGY
default_overlap = fm.default_overlap
row_ok = fm.row_ok


def lens_ok(ls, lm, n):
    return 1 <= ls <= 2 * n and 1 <= lm <= n


def overlap(n, ls, lm):
    """-> (n0, n1, m) per index: sample frames [n0, n1) meet source frames [n0 + l, n1 + l); m <= 0: the lag does not exist"""
    lag = np.arange(-(n - 1), n)
    n0 = np.maximum(0, -lag)
    n1 = np.minimum(lm, ls - lag)
    return n0, n1, n1 - n0


def r_plain(x, y, n):
    """r[l] = sum over the overlap of x[n + l] * y[n] for l = -(N-1)..N-1 (0 where there is none), in float64: the time-domain sum
    for short tracks, else float64 transforms long enough that nothing wraps"""
    ls, lm = x.size, y.size
    if ls * lm <= 1 << 25:
        full = np.correlate(x, y, "full")                     # index k: lag k - (Lm - 1)
    else:
        size = 1 << int(np.ceil(np.log2(ls + lm)))
        full = np.fft.irfft(np.fft.rfft(x, size) * np.conj(np.fft.rfft(y, size)), size)
        full = np.concatenate([full[size - (lm - 1):], full[:ls]])
    r = np.zeros(2 * n - 1)
    lag = np.arange(-(lm - 1), ls)
    keep = (lag >= -(n - 1)) & (lag <= n - 1)
    r[lag[keep] + n - 1] = full[keep]
    return r


def curve(src, smp, ls, lm):
    """-> (c[2N-1] float64 (NaN: the lag does not exist), e[2N-1] = Vx[l] * Vy[l], vmax, vy, m[2N-1])"""
    n = smp.size
    assert src.size == 2 * n and lens_ok(ls, lm, n)
    x, y = src[:ls].astype(np.float64), smp[:lm].astype(np.float64)
    mu, my = x.mean(), y.mean()
    a, b = x - mu, y - my
    pa1, pa2 = np.concatenate([[0.0], np.cumsum(a)]), np.concatenate([[0.0], np.cumsum(a * a)])
    pb1, pb2 = np.concatenate([[0.0], np.cumsum(b)]), np.concatenate([[0.0], np.cumsum(b * b)])
    n0, n1, m = overlap(n, ls, lm)
    lag = np.arange(-(n - 1), n)
    ok = m > 0
    i0, i1 = np.where(ok, n0, 0), np.where(ok, n1, 0)
    j0, j1 = np.where(ok, n0 + lag, 0), np.where(ok, n1 + lag, 0)
    md = np.where(ok, m, 1).astype(np.float64)
    s1x, s1y = pa1[j1] - pa1[j0], pb1[i1] - pb1[i0]
    vx, vy_l = (pa2[j1] - pa2[j0]) - s1x * s1x / md, (pb2[i1] - pb2[i0]) - s1y * s1y / md
    sx, sy = s1x + md * mu, s1y + md * my
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (r_plain(x, y, n) - sx * sy / md) / np.sqrt(vx * vy_l)
    c = np.where(ok, c, np.nan)
    e = np.where(ok, vx * vy_l, np.nan)
    vy = float(pb2[lm] - pb1[lm] * pb1[lm] / lm)
    w = min(ls, lm)
    j = np.arange(0, min(ls - w, n - 1) + 1)
    d1 = pa1[j + w] - pa1[j]
    vmax = float(np.nanmax(np.maximum((pa2[j + w] - pa2[j]) - d1 * d1 / w, 0.0)))
    return c, e, vmax, vy, m


def competing(cv, ls, lm, min_energy=DEFAULT_ENERGY, min_overlap=None):
    """the lags that compete (index l + N - 1): m >= min(min_overlap, Ls, Lm), Vy > 0, Vx[l] Vy[l] >= min_energy Vmax Vy, c[l] finite"""
    c, e, vmax, vy, m = cv
    n = (c.size + 1) // 2
    mo = default_overlap(n) if min_overlap is None else min_overlap
    with np.errstate(invalid="ignore"):
        return (m > 0) & (m >= min(mo, ls, lm)) & (vy > 0) & (e >= min_energy * vmax * vy) & np.isfinite(c)


def near_threshold(cv, min_energy=DEFAULT_ENERGY, factor=2.0):
    """the lags whose energy lies within `factor` of the threshold: the last bits may decide them"""
    c, e, vmax, vy, m = cv
    thr = min_energy * vmax * vy
    with np.errstate(invalid="ignore"):
        return (e > thr / factor) & (e < thr * factor)


def keys_of(cv, ls, lm, min_energy=DEFAULT_ENERGY, min_overlap=None):
    """|float32(c)| per index, NaN where the lag does not compete"""
    ok = competing(cv, ls, lm, min_energy, min_overlap)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(ok, np.abs(cv[0].astype(np.float32)), np.float32("nan")).astype(np.float32)


def coefficient(src, smp, lag, ls, lm):
    """oracle.pearson_coefficient over source[n0 + l, n1 + l) against sample[n0, n1); NaN for an empty segment"""
    n0, n1 = max(0, -lag), min(lm, ls - lag)
    if n1 <= n0:
        return float("nan")
    return oracle.pearson_coefficient(src[n0 + lag:n1 + lag], smp[n0:n1])


def topk(src, smp, ls, lm, k, min_separation, row=None, min_energy=DEFAULT_ENERGY, min_overlap=None, cv=None):
    """-> k entries (ret, lag, coef, peak): -5 in all of them for lengths that are none, else tests/ncc_full_model.py's rule over the
    ragged curve"""
    n = smp.size
    nan = float("nan")
    if not lens_ok(ls, lm, n):
        return [(-5, 0, nan, nan)] * k
    keys = keys_of(curve(src, smp, ls, lm) if cv is None else cv, ls, lm, min_energy, min_overlap)
    out = []
    for status, lag, peak in fm.topk_of_keys(keys, k, min_separation, row):
        coef = coefficient(src, smp, lag, ls, lm) if status == 0 else nan
        out.append((status if status else (-1 if coef != coef else 0), lag, coef, peak))
    return out


def model(src, smp, ls, lm, row=None, min_energy=DEFAULT_ENERGY, min_overlap=None, cv=None):
    """-> (ret, lag, coef, peak) of one pair"""
    return topk(src, smp, ls, lm, 1, 0, row, min_energy, min_overlap, cv)[0]


def runner_up(cv, ok, lags):
    """the largest |c| among the competing lags other than `lags` (a lag or several)"""
    n = (cv[0].size + 1) // 2
    a = np.where(ok, np.abs(cv[0]), -1.0)
    for lag in np.atleast_1d(lags):
        a[lag + n - 1] = -1.0
    return float(a.max())


def padded(src, smp, ls, lm):
    """the pair as a caller without lengths would hand it over: zeros at and beyond the lengths"""
    s, t = src.copy(), smp.copy()
    s[ls:] = 0
    t[lm:] = 0
    return s, t


# ---- fixtures: (N, p) -> (source float32 [2N], sample float32 [N], Ls, Lm, planted lag or lags) -------------------------------------

def fixture_g(n, p):
    """the sample holds N/4 real frames on +3.0 DC, copied from the source at lag N/3 + 5p, the rest of it is zero; the source
    carries a +4.0 block of N/4 frames at 1.1 N.  Zero-padded, the sample is a pulse and the block attracts it."""
    rng = np.random.default_rng(7000 + p)
    lag, lm, ls = n // 3 + 5 * p, n // 4, 2 * n
    src = rng.standard_normal(2 * n)
    smp = np.zeros(n)
    smp[:lm] = 0.7 * src[lag:lag + lm] + 0.3 * rng.standard_normal(lm) + 3.0
    at = (11 * n) // 10
    src[at:at + lm] += 4.0
    return src.astype(np.float32), smp.astype(np.float32), ls, lm, lag


def fixture_h(n, p):
    """Ls = 1.5 N, Lm = 0.7 N: the sample starts N/5 frames before the source (lag -N/5) and its frames from there on are 0.7
    source + 0.3 noise, all of it on +3.0 DC; the source carries a +4.0 block of N/4 frames at 0.9 N; NaN beyond both lengths"""
    rng = np.random.default_rng(8000 + p)
    lag, lm, ls = -(n // 5), (7 * n) // 10, (3 * n) // 2
    src = rng.standard_normal(2 * n)
    smp = rng.standard_normal(n) + 3.0
    smp[-lag:lm] = 0.7 * src[:lm + lag] + 0.3 * rng.standard_normal(lm + lag) + 3.0
    at = (9 * n) // 10
    src[at:at + n // 4] += 4.0
    src[ls:] = np.nan
    smp[lm:] = np.nan
    return src.astype(np.float32), smp.astype(np.float32), ls, lm, lag


K_GAINS = (0.8, 0.5)


def fixture_k(n, p):
    """two copies: Lm = N/4 sample frames = 0.8 source[La : La + Lm] + 0.5 source[Lb : Lb + Lm] + 0.2 noise + 1.0 DC, La = N/2 + 3p,
    Lb = N/8 + p, Ls = 1.75 N; 1e30 beyond both lengths.  -> the lags, strongest first"""
    rng = np.random.default_rng(9000 + p)
    la, lb, lm, ls = n // 2 + 3 * p, n // 8 + p, n // 4, (7 * n) // 4
    src = rng.standard_normal(2 * n)
    smp = np.zeros(n)
    smp[:lm] = K_GAINS[0] * src[la:la + lm] + K_GAINS[1] * src[lb:lb + lm] + 0.2 * rng.standard_normal(lm) + 1.0
    src[ls:] = 1e30
    smp[lm:] = -1e30
    return src.astype(np.float32), smp.astype(np.float32), ls, lm, (la, lb)
