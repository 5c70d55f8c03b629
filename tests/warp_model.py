"""float64 model of asx_xcorr_warp_f32_dev (include/audiosync/xcorr_hip.h): along the line "sample frame n meets source frame
n + centre + k_n", k_n = floor((b + a n) + 0.5), the sum r[d] = sum_{n<N} source[(n + p + d + k_n) mod 2N] * sample[n] with math.fsum
over the float64 products (exact for float32 inputs), the parabolic vertex of its three centre values (phat_sub_model.frac_of), the
frames V that line up without a wrap, and the reference's Pearson coefficient over them in two passes, every sum with math.fsum.
The tolerances are first-order worst cases of any float64 evaluation order, with or without fused multiply-add."""
import math

import numpy as np

import curve_model
import phat_sub_model

NEAR_MAX = curve_model.NEAR_MAX
DRIFT_MAX = 2.0 ** -6
EPS = 2.0 ** -53

tolerance = curve_model.tolerance  # of r: N * 2^-53 * sum |products|


def shifts(n, a, b):
    """k_0 .. k_{n-1} as int64: the multiply, the two adds and the floor each rounded on their own, in float64"""
    return np.floor((np.float64(b) + np.float64(a) * np.arange(n, dtype=np.float64)) + 0.5).astype(np.int64)


def valid_line(n, a, b):
    return bool(math.isfinite(a) and math.isfinite(b) and abs(a) <= DRIFT_MAX and abs(b) <= n)


def r_at(source, sample, lag, a, b, d):
    """-> (r[d] along the line (a, b) through `lag`, correctly rounded; the sum of the |products| of its terms)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    at = (np.arange(n, dtype=np.int64) + curve_model.index_of(lag, n) + int(d) + shifts(n, a, b)) % (2 * n)
    prod = s[at] * t
    return math.fsum(prod), float(math.fsum(np.abs(prod)))


def valid_range(n, lag, a, b):
    """V = {n in [0, N) : 0 <= n + lag + k_n < 2N} as (first, last + 1); (0, 0) when it is empty.  One contiguous range."""
    u = np.arange(n, dtype=np.int64) + int(lag) + shifts(n, a, b)
    inside = np.flatnonzero((u >= 0) & (u < 2 * n))
    if inside.size == 0:
        return 0, 0
    assert inside[-1] - inside[0] + 1 == inside.size, "V is not contiguous"
    return int(inside[0]), int(inside[-1]) + 1


def pearson(x, y):
    """the reference's pearson_coefficient() (src/cross_correlation.c:74-116) in two passes over float64 lists, every sum with
    math.fsum -> (coef, xbar, ybar, sigma_x, sigma_y); NaN for an empty or constant side"""
    m = len(x)
    nan = float("nan")
    if m == 0:
        return nan, nan, nan, nan, nan
    xb, yb = math.fsum(x) / m, math.fsum(y) / m
    sxx = math.fsum((v - xb) ** 2 for v in x)
    syy = math.fsum((v - yb) ** 2 for v in y)
    sxy = math.fsum((v - xb) * (w - yb) for v, w in zip(x, y))
    den = math.sqrt(sxx * syy)
    return (sxy / den if den > 0.0 else nan), xb, yb, math.sqrt(sxx / m), math.sqrt(syy / m)


def tol_coef(length, xbar, ybar, sx, sy):
    """64 * len * 2^-53 * (1 + |xbar| / sigma_x)(1 + |ybar| / sigma_y): the first-order style and the constant of
    track_model.fit_tolerances -- len roundings of relative size 2^-53 in each of the sums, amplified by how far the means sit from
    zero in units of the spread; about 1e-9 at len = 144 000 on zero-mean material"""
    return 64.0 * length * EPS * (1.0 + abs(xbar) / sx) * (1.0 + abs(ybar) / sy)


def coef(source, sample, lag, a, b):
    """-> (coefficient over the pairs (source[u_n], sample[n]), n in V; |V|; its tolerance, NaN where the coefficient is)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    lo, hi = valid_range(n, lag, a, b)
    u = np.arange(lo, hi, dtype=np.int64) + int(lag) + shifts(n, a, b)[lo:hi]
    c, xb, yb, sx, sy = pearson(s[u].tolist(), t[lo:hi].tolist())
    return c, hi - lo, (tol_coef(hi - lo, xb, yb, sx, sy) if c == c else float("nan"))


def warp(source, sample, lag, a, b, h):
    """-> dict(r [2h + 1], tol [2h + 1], frac, coef, len, tol_coef) along the line (a, b) through `lag`"""
    assert 1 <= h <= NEAR_MAX and valid_line(np.asarray(sample).size, a, b)
    n = np.asarray(sample).size
    vals = [r_at(source, sample, lag, a, b, d) for d in range(-h, h + 1)]
    r = np.array([v for v, _ in vals])
    c, length, tc = coef(source, sample, lag, a, b)
    return dict(r=r, tol=np.array([tolerance(n, s) for _, s in vals]), frac=phat_sub_model.frac_of(r[h - 1], r[h], r[h + 1]),
                coef=c, len=length, tol_coef=tc)


def planted(n, l0, a, b):
    """white float32 noise of 2N frames and a sample that follows it along the line (a, b) through the lag l0: sample[n] =
    source[n + l0 + k_n] for n in V, fresh noise elsewhere"""
    rng = np.random.default_rng(200)
    src = rng.standard_normal(2 * n).astype(np.float32)
    smp = rng.standard_normal(n).astype(np.float32)
    lo, hi = valid_range(n, l0, a, b)
    smp[lo:hi] = src[np.arange(lo, hi, dtype=np.int64) + int(l0) + shifts(n, a, b)[lo:hi]]
    return src, smp


def planted_cases(n):
    """(l0, a, b) of the planted pairs at length n"""
    lines = [(12.0 / n, 0.25), (-12.0 / n, -0.75)] + ([(40.0 / n, 0.0)] if n == 144000 else [])
    return [(l0, a, b) for l0 in (n // 3 + 1, -(n // 4) - 3) for a, b in lines]
