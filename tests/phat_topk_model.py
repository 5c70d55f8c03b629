"""float64 model of asx_xcorr_phat_topk_f32_dev (include/audiosync/xcorr_hip.h): the banded GCC-PHAT curve of
tests/phat_band_model.py, the top-k rule of tests/topk_model.py over it -- entry j is the windowed max_abs_index rule over A_j, the
pair's window minus the lags within min_separation of the earlier entries -- then the reference's lag wrap, segments and
pearson_coefficient through the oracle, and the curve's height at the entry."""
import math

import numpy as np

import oracle
import phat_band_model
import topk_model
from lag_window_model import wrap

MULTIPATH_LAGS = (1200, -7000, 31000, 90, -52000)
MULTIPATH_GAINS = (1.0, 0.8, 0.65, 0.5, 0.4)
MULTIPATH_NOISE = 0.1


def model(source, sample, bin_lo, bin_hi, k, sep, lo=None, hi=None, r=None):
    """-> list of k (ret, lag, coef, peak); an empty A_j gives (-3, 0, nan, nan).  r: r_phat_band(source, sample, bin_lo, bin_hi)
    when the caller has it."""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    if r is None:
        r = phat_band_model.r_phat_band(s, t, bin_lo, bin_hi)
    out = []
    for p in topk_model.topk_peaks(r, n, k, sep, lo, hi):
        if p is None:
            out.append((-3, 0, float("nan"), float("nan")))
            continue
        lag, (s0, s1), (t0, t1) = wrap(p, n)
        coef = oracle.pearson_coefficient(s[s0:s1], t[t0:t1]) if s1 > s0 else float("nan")
        out.append(((-1 if math.isnan(coef) else 0), lag, coef, abs(float(r[p]))))
    return out


def margins(r, n, entries, sep, lo=None, hi=None):
    """how far each entry of `entries` (model()'s list) stands above the best lag its pass left: over A_j every element competes
    with |r| but the seed -- the smallest index -- which competes signed, and the margin is the winner's competing value minus the
    largest of the others' (infinite when A_j holds one lag, NaN for an empty entry) -> list of floats.  All of them large against
    the float32 resolution means no rounding can reorder the entries."""
    lo = -n if lo is None else lo
    hi = n - 1 if hi is None else hi
    r = np.asarray(r, dtype=np.float64)
    out, lags = [], []
    for ret, lag, _, _ in entries:
        if ret == -3:
            out.append(float("nan"))
            continue
        idx = topk_model.allowed(n, lo, hi, lags, sep)
        value = np.abs(r[idx])
        value[0] = r[idx[0]]
        w = int(np.flatnonzero(idx == lag % (2 * n))[0])
        rest = np.delete(value, w)
        out.append(float(value[w] - rest.max()) if rest.size else float("inf"))
        lags.append(lag)
    return out


E2E_N, E2E_K, E2E_SEP, E2E_TOL, E2E_SEED = 144000, 3, 64, 2, 20271
E2E_OFFSETS = (0, 20000, 45000, 70000)
E2E_ECHOES = ((9000, 0.6), (13000, 0.6), (5000, 0.6), (17000, 0.6))     # per clip: the echo's delay in frames and its gain


def e2e_clips(seed=E2E_SEED):
    """4 clips of 2N frames cut from one noise recording (default_rng(seed).standard_normal) at E2E_OFFSETS, so the lag of (a, b) is
    offset_b - offset_a.  Clip c also hears itself d_c frames late at gain g_c (E2E_ECHOES) -- in the pair (a, b) that plants the
    decoys T + d_a and T - d_b -- and carries the 50 Hz tone of phat_model.hum_pair at amplitude 0.5, its phase 1.0 + c."""
    n = E2E_N
    pad = max(d for d, _ in E2E_ECHOES)
    rec = np.random.default_rng(seed).standard_normal(pad + max(E2E_OFFSETS) + 2 * n)
    w = 2.0 * np.pi * 50.0 / 48000.0
    clips = []
    for c, (o, (d, g)) in enumerate(zip(E2E_OFFSETS, E2E_ECHOES)):
        at = pad + o
        clips.append(rec[at:at + 2 * n] + g * rec[at - d:at - d + 2 * n] + 0.5 * np.sin(w * np.arange(2 * n) + 1.0 + c))
    return np.stack(clips).astype(np.float32)


def e2e_tables(clips, band=None):
    """the model's [C, C, k] tables of the all-pairs call over e2e_clips() (a sample is a clip's first N frames) -> (lag, coef, peak, ret)"""
    C, n = len(clips), E2E_N
    lo, hi = (0, n) if band is None else band
    lag = np.zeros((C, C, E2E_K), dtype=np.int64)
    coef = np.zeros((C, C, E2E_K))
    peak = np.zeros((C, C, E2E_K))
    ret = np.zeros((C, C, E2E_K), dtype=np.int32)
    for a in range(C):
        for b in range(C):
            for j, e in enumerate(model(clips[a], clips[b, :n], lo, hi, E2E_K, E2E_SEP)):
                ret[a, b, j], lag[a, b, j], coef[a, b, j], peak[a, b, j] = e
    return lag, coef, peak, ret


def check_e2e(lag, ret, out):
    """tables of the four clips (the model's or the device's) and closure's outputs for them: every pair's first entry is its
    planted lag, an echo decoy of the source or of the sample is among the entries behind it, closure keeps the planted lags and
    places the clips"""
    o = np.array(E2E_OFFSETS, dtype=np.int64)
    true = o[None, :] - o[:, None]
    assert lag[:, :, 0].tobytes() == true.tobytes() and not ret.any(), (lag[:, :, 0], ret)
    for a in range(4):
        for b in range(4):
            decoys = {int(true[a, b]) + E2E_ECHOES[a][0], int(true[a, b]) - E2E_ECHOES[b][0]}
            assert decoys & set(lag[a, b, 1:].tolist()), (a, b, lag[a, b])
    assert out["best_lag"].tobytes() == true.tobytes() and not out["best_ret"].any() and not out["best_entry"].any()
    assert out["placed"].tolist() == [1] * 4
    assert (np.abs(out["offset"] - (o - o[out["root"]])) <= E2E_TOL).all(), (out["offset"], out["root"])


def multipath_pair(seed, n, lags=MULTIPATH_LAGS, gains=MULTIPATH_GAINS):
    """a sample that hears the source over several paths: source = 2n values of default_rng(seed).standard_normal rounded to float32;
    sample[m] = sum_i gains[i] * source[(m + lags[i]) mod 2n] + 0.1 * standard_normal(n), rounded to float32 -> (source, sample)"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n).astype(np.float32)
    s64 = src.astype(np.float64)
    m = np.arange(n)
    smp = np.zeros(n)
    for l, g in zip(lags, gains):
        smp += g * s64[(m + l) % (2 * n)]
    smp += MULTIPATH_NOISE * rng.standard_normal(n)
    return src, smp.astype(np.float32)
