"""float64 model of asx_xcorr_phat_f32_dev (include/audiosync/xcorr_hip.h): the GCC-PHAT curve at F = 2N through numpy's
rfft / irfft with the zero-bin rule, the windowed max_abs_index rule of tests/lag_window_model.py over it, then the reference's lag
wrap, segments and pearson_coefficient through the oracle."""
import math

import numpy as np

import oracle
from lag_window_model import window_peak, wrap

HUM_SEED, HUM_N = 11, 144000


def r_phat(source, sample):
    """r_phat / F for all F = 2N lags: every bin of X conj(Y) divided by its magnitude; a bin that is exactly zero stays zero.  The
    sample is zero-padded to the source's length (N samples as the library takes them; up to 2N for a circular test signal)."""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    f = s.size
    assert f % 2 == 0 and t.size <= f
    q = np.fft.rfft(s) * np.conj(np.fft.rfft(t, f))
    mag = np.abs(q)
    unit = np.divide(q, mag, out=np.zeros_like(q), where=mag > 0)
    return np.fft.irfft(unit, f)


def model(source, sample, lo=None, hi=None, r=None):
    """-> (ret, lag, coef, peak) with the peak searched at lags lo..hi of r_phat (default: every lag)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    lo = -n if lo is None else lo
    hi = n - 1 if hi is None else hi
    if r is None:
        r = r_phat(s, t)
    idx = window_peak(r, n, lo, hi)
    lag, (s0, s1), (t0, t1) = wrap(idx, n)
    coef = oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")
    return (-1 if math.isnan(coef) else 0), lag, coef, abs(float(r[idx]))


def hum_pair(p, n=HUM_N):
    """oracle.synth_pair(11, p, n, 1) with a 50 Hz tone of amplitude 0.5 in both tracks (48 kHz; the sample's phase is 1.0 + p): the
    tone carries the raw correlation's peak away from the planted lag -> (source, sample, planted lag)"""
    src, smp, lag = oracle.synth_pair(HUM_SEED, p, n, 1)
    w = 2.0 * np.pi * 50.0 / 48000.0
    src = (src.astype(np.float64) + 0.5 * np.sin(w * np.arange(2 * n))).astype(np.float32)
    smp = (smp.astype(np.float64) + 0.5 * np.sin(w * np.arange(n) + 1.0 + p)).astype(np.float32)
    return src, smp, lag
