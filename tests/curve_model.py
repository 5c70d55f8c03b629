"""float64 model of asx_xcorr_curve_f32_dev (include/audiosync/xcorr_hip.h): around a given lag, the time-domain sum
r[idx] = sum_{n<N} source[(n + idx) mod 2N] * sample[n] at the 2h + 1 neighbouring indices (circular over the 2N indices), summed with
math.fsum over the float64 products (exact for float32 inputs), the reference's Pearson coefficient at each index's lag
(lag_window_model.wrap, oracle.pearson_coefficient) and the parabolic vertex of the three centre values (phat_sub_model.frac_of)."""
import math

import numpy as np

import lag_window_model
import oracle
import phat_sub_model

NEAR_MAX = phat_sub_model.NEAR_MAX


def index_of(lag, n):
    """lag l >= 0 is index l, lag l < 0 index 2N + l"""
    assert -n <= lag <= n - 1
    return int(lag) if lag >= 0 else 2 * n + int(lag)


def r_at(source, sample, idx):
    """-> (r[idx] correctly rounded, sum of the |products| of its terms)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    prod = s[(np.arange(n) + int(idx)) % (2 * n)] * t
    return math.fsum(prod), float(math.fsum(np.abs(prod)))


def tolerance(n, sum_abs):
    """the first-order worst case of any float64 summation order over n exact products"""
    return n * 2.0 ** -53 * sum_abs


def coef_at(source, sample, idx):
    """the reference's coefficient at index idx: the wrap and the segments of src/cross_correlation.c:256-272; NaN for the empty one"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    _, (s0, s1), (t0, t1) = lag_window_model.wrap(int(idx), t.size)
    return oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")


def neighbours(lag, n, h):
    """the 2h + 1 indices around the lag's index, d = -h .. h"""
    assert 1 <= h <= NEAR_MAX
    return [(index_of(lag, n) + d) % (2 * n) for d in range(-h, h + 1)]


def lag_of(idx, n):
    """the lag of an index after the reference's wrap"""
    return lag_window_model.wrap(int(idx), n)[0]


def curve(source, sample, lag, h, coef=True):
    """-> (r [2h + 1], tol [2h + 1], coef [2h + 1] or None, frac) around `lag`"""
    n = np.asarray(sample).size
    idx = neighbours(lag, n, h)
    vals = [r_at(source, sample, i) for i in idx]
    r = np.array([v for v, _ in vals])
    tol = np.array([tolerance(n, a) for _, a in vals])
    c = np.array([coef_at(source, sample, i) for i in idx]) if coef else None
    return r, tol, c, phat_sub_model.frac_of(r[h - 1], r[h], r[h + 1])
