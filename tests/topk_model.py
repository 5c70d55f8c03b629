"""float64 model of the top-k rule of asx_xcorr_topk_f32_dev (include/audiosync/xcorr_hip.h), built from the oracle: entry j is the
reference's max_abs_index (src/cross_correlation.c:52-67) over A_j -- the pair's window minus the lags within min_separation of the
earlier entries -- in ascending index order, then the reference's lag wrap, segments (:256-271) and pearson_coefficient (:272)."""
import math

import numpy as np

import oracle
from lag_window_model import window_indices, wrap


def allowed(n, lo, hi, lags, sep):
    """A_j as ascending indices: the window [lo, hi] minus |l - lag_i| <= sep for every lag_i in lags"""
    idx = window_indices(n, lo, hi)
    lag = np.where(idx < n, idx, idx - 2 * n)
    keep = np.ones(idx.size, dtype=bool)
    for li in lags:
        keep &= np.abs(lag - int(li)) > sep
    return idx[keep]


def topk_peaks(r, n, k, sep, lo=None, hi=None):
    """-> list of k peak indices (None once A_j is empty)"""
    lo = -n if lo is None else lo
    hi = n - 1 if hi is None else hi
    r = np.asarray(r, dtype=np.float64)
    peaks, lags = [], []
    for _ in range(k):
        idx = allowed(n, lo, hi, lags, sep)
        if idx.size == 0:
            peaks.append(None)
            continue
        p = int(idx[oracle.max_abs_index(r[idx])])
        peaks.append(p)
        lags.append(wrap(p, n)[0])
    return peaks


def brute_peaks(r, n, k, sep, lo, hi):
    """the same rule written as a plain loop over every lag (the check of topk_peaks)"""
    r = [float(v) for v in r]
    peaks, lags = [], []
    for _ in range(k):
        best, bk = None, None
        for i in range(2 * n):
            l = i if i < n else i - 2 * n
            if not (lo <= l <= hi) or any(abs(l - m) <= sep for m in lags):
                continue
            if best is None:
                best, bk = i, r[i]           # the seed: signed
            elif abs(r[i]) > bk:
                best, bk = i, abs(r[i])
        peaks.append(best)
        if best is not None:
            lags.append(best if best < n else best - 2 * n)
    return peaks


def model(source, sample, k, sep, lo=None, hi=None, r=None):
    """-> list of k (ret, lag, coef) of the top-k rule; an empty A_j gives (-3, 0, nan)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    if r is None:
        r = oracle.cross_correlation(s, t, want_results=True)[3]
    out = []
    for p in topk_peaks(r, n, k, sep, lo, hi):
        if p is None:
            out.append((-3, 0, float("nan")))
            continue
        lag, (s0, s1), (t0, t1) = wrap(p, n)
        coef = oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")
        out.append(((-1 if math.isnan(coef) else 0), lag, coef))
    return out
