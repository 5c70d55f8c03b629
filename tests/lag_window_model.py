"""float64 model of the lag-window rule of asx_plan_set_lag_window (include/audiosync/xcorr_hip.h), built from the oracle:
the reference's max_abs_index (src/cross_correlation.c:52-67) run over the in-window elements of results[] in ascending index
order, then the reference's lag wrap, segments (:256-271) and pearson_coefficient (:272)."""
import math

import numpy as np

import oracle


def window_indices(n, lo, hi):
    """the in-window indices of r, ascending: lag l >= 0 is index l, lag l < 0 index 2N + l"""
    assert -n <= lo <= hi <= n - 1
    lags = np.arange(lo, hi + 1, dtype=np.int64)
    return np.sort(np.where(lags >= 0, lags, 2 * n + lags))


def window_peak(r, n, lo, hi):
    """index of the windowed peak: the first in-window element seeds the maximum signed, the rest compete with fabs"""
    idx = window_indices(n, lo, hi)
    return int(idx[oracle.max_abs_index(np.asarray(r, dtype=np.float64)[idx])])


def wrap(peak, n):
    """src/cross_correlation.c:256-271 -> (lag, source range, sample range)"""
    if peak >= n:
        lag = peak % n - n
        return lag, (0, lag + n), (-lag, n)
    return peak, (peak, peak + n), (0, n)


def model(source, sample, lo=None, hi=None, r=None):
    """-> (ret, lag, coef) of cross_correlation() with the peak searched only at lags lo..hi (default: every lag)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    lo = -n if lo is None else lo
    hi = n - 1 if hi is None else hi
    if r is None:
        r = oracle.cross_correlation(s, t, want_results=True)[3]
    lag, (s0, s1), (t0, t1) = wrap(window_peak(r, n, lo, hi), n)
    coef = oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")
    return (-1 if math.isnan(coef) else 0), lag, coef
