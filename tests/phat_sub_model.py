"""float64 model of asx_xcorr_phat_sub_f32_dev (include/audiosync/xcorr_hip.h): the banded PHAT model of tests/phat_band_model.py,
then the 2h + 1 values of r_phat / V around the peak's index, circularly over the 2N indices, and the parabolic vertex through the
three centre values in the order the header states.  single_lag is the sum k_phat_near evaluates, over the real-column Q of
tests/model_fourstep.py."""
import math

import numpy as np

import phat_band_model

NEAR_MAX = 8


def frac_of(ym, y0, yp):
    """the header's rule, in float64 and in its order -> frac"""
    ym, y0, yp = float(ym), float(y0), float(yp)
    if math.isnan(ym) or math.isnan(y0) or math.isnan(yp):
        return float("nan")
    s = -1.0 if y0 < 0.0 else 1.0
    a, b, c = s * ym, s * y0, s * yp
    den = (a - 2.0 * b) + c
    if den >= 0.0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * (a - c) / den))


def den_of(ym, y0, yp):
    """the rule's denominator (negative at a peak), for the tests' conditioning checks"""
    s = -1.0 if y0 < 0.0 else 1.0
    return (s * ym - 2.0 * (s * y0)) + s * yp


def near_of(r, idx, h):
    """r[(idx + d) mod len(r)] for d = -h .. h"""
    assert 1 <= h <= NEAR_MAX
    return np.asarray(r, dtype=np.float64)[(idx + np.arange(-h, h + 1)) % len(r)].copy()


def model(source, sample, bin_lo, bin_hi, h, lo=None, hi=None, r=None):
    """-> (ret, lag, coef, peak, frac, near): phat_band_model.model's four, then the neighbourhood of the peak's index in r_phat / V
    (r: that curve, computed here when not given) and the fractional lag"""
    n = np.asarray(sample).size
    if r is None:
        r = phat_band_model.r_phat_band(source, sample, bin_lo, bin_hi)
    ret, lag, coef, peak = phat_band_model.model(source, sample, bin_lo, bin_hi, lo, hi, r=r)
    near = near_of(r, lag % (2 * n), h)
    return ret, lag, coef, peak, frac_of(near[h - 1], near[h], near[h + 1]), near


def single_lag(Q, M1, M2, idx):
    """one value of the real-column inverse from ONE column of Q (rows 0 .. M1 of M2 columns), idx = j1 * M2 + j2:
    Re Q[0][j2] + (-1)^j1 Re Q[M1][j2] + 2 sum_{0 < u < M1} Re(Q[u][j2] exp(+i pi u j1 / M1)), the twiddle from (u j1) mod 2 M1"""
    j1, j2 = divmod(int(idx), M2)
    assert 0 <= j1 < 2 * M1
    u = np.arange(1, M1)
    w = np.exp(1j * np.pi * ((u * j1) % (2 * M1)) / M1)
    return float(Q[0, j2].real + (-1.0) ** j1 * Q[M1, j2].real + 2.0 * np.sum((Q[1:M1, j2] * w).real))


def delayed_pair(n, p, delta, seed=5):
    """a source of 2n white samples and the same track circularly delayed so that r peaks at p + delta frames: the sample's spectrum
    is the source's times a phase ramp, in float64 -> (source, full-length sample)"""
    src = np.random.default_rng(seed).standard_normal(2 * n)
    k = np.arange(n + 1)
    ramp = np.exp(2j * np.pi * k * (p + delta) / (2 * n))
    if float(p + delta) != int(p + delta):
        ramp[n] = ramp[n].real          # bin N of a real track is real: a fractional delay keeps the cosine part
    return src, np.fft.irfft(np.fft.rfft(src) * ramp, 2 * n)
