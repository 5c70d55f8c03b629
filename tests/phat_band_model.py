"""float64 model of asx_xcorr_phat_band_f32_dev (include/audiosync/xcorr_hip.h): tests/phat_model.py with the band's mask between
the division and the inverse transform, and the division by the number of bins that vote."""
import math

import numpy as np

import oracle
from lag_window_model import window_peak, wrap

LOWPASS_SEED, LOWPASS_N, LOWPASS_SHIFT, LOWPASS_NOISE = 77, 144000, 3, 1e-4


def votes(n, lo, hi):
    """V: the number of k in [0, 2N) whose frequency min(k, 2N - k) lies in [lo, hi]; bins 0 and N are their own mirrors"""
    assert 0 <= lo <= hi <= n
    return 2 * (hi - lo + 1) - (lo == 0) - (hi == n)


def r_phat_band(source, sample, lo, hi):
    """r_phat / V for all F = 2N lags: every bin m of X conj(Y) with lo <= m <= hi divided by its magnitude (a bin that is exactly
    zero stays zero), every other bin zero.  rfft holds bins 0..N, irfft supplies the mirrors.  N is half the source's length."""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    f = s.size
    assert f % 2 == 0 and t.size <= f
    q = np.fft.rfft(s) * np.conj(np.fft.rfft(t, f))
    mag = np.abs(q)
    unit = np.divide(q, mag, out=np.zeros_like(q), where=mag > 0)
    unit[:lo] = 0.0
    unit[hi + 1:] = 0.0
    return np.fft.irfft(unit, f) * (f / votes(f // 2, lo, hi))


def model(source, sample, bin_lo, bin_hi, lo=None, hi=None, r=None):
    """-> (ret, lag, coef, peak) with the peak searched at lags lo..hi of the banded r_phat (default: every lag)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    lo = -n if lo is None else lo
    hi = n - 1 if hi is None else hi
    if r is None:
        r = r_phat_band(s, t, bin_lo, bin_hi)
    idx = window_peak(r, n, lo, hi)
    lag, (s0, s1), (t0, t1) = wrap(idx, n)
    coef = oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")
    return (-1 if math.isnan(coef) else 0), lag, coef, abs(float(r[idx]))


def lowpass_pair(p, n=LOWPASS_N):
    """oracle.synth_pair(77, p, n, 3), both tracks low-passed at bin n/6 of the 2n-point transform (4 kHz at 48 kHz: a brick wall
    through rfft / irfft of each track at its own length, so the source's cut is its bin n/6 and the sample's its bin n/12), with
    independent white noise of amplitude 1e-4 (default_rng(5 + p): the source's 2n values, then the sample's n) added to both,
    rounded to float32 -> (source, sample, planted lag)"""
    src, smp, lag = oracle.synth_pair(LOWPASS_SEED, p, n, LOWPASS_SHIFT)
    rng = np.random.default_rng(5 + p)

    def low(x):
        z = np.fft.rfft(np.asarray(x, dtype=np.float64))
        z[x.size * (n // 6) // (2 * n) + 1:] = 0.0     # the same frequency in a track of x.size samples
        return np.fft.irfft(z, x.size)

    src = (low(src) + LOWPASS_NOISE * rng.standard_normal(2 * n)).astype(np.float32)
    smp = (low(smp) + LOWPASS_NOISE * rng.standard_normal(n)).astype(np.float32)
    return src, smp, lag
