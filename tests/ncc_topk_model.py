"""The top-k rule of the normalised cross-correlation (asx_xcorr_ncc_topk_f32_dev, asx_xcorr_pool_ncc_topk_f32_dev) over a given
curve, as include/audiosync/xcorr_hip.h states it, and fixture C: three copies of the sample in one source, the quietest of which no
raw search returns.  Builds on tests/ncc_model.py.  Plain module: no fixtures, nothing happens on import."""
import numpy as np

import ncc_model

GAINS = (0.3, 1.0, 0.6)   # fixture C: the copies at lags N/10 + 17p, N/2 + 5p, 8N/10 - 3p


def keys_of(c, vx, vy, min_energy=ncc_model.DEFAULT_ENERGY):
    """|float32(c)| per lag, NaN where the lag does not compete: what the device keeps of the curve (the debug call's d_c, in
    absolute value)"""
    ok = ncc_model.competing(c, vx, vy, min_energy)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(ok, np.abs(c.astype(np.float32)), np.float32("nan")).astype(np.float32)


def topk_of_keys(keys, k, min_separation, row=None):
    """The rule over keys[l] = |c32[l]| (NaN: lag l does not compete), l = 0..N-1.  -> k entries (status, lag, peak): status 0 for an
    entry with a lag (its ret is then 0, or -1 for a NaN coefficient), -3 when A_j is empty, -2 for a row that is not a row of the
    call; lag 0 and a NaN peak with -2 and -3."""
    n = keys.size
    lo, hi = (0, n - 1) if row is None else (int(row[0]), int(row[1]))
    nan = float("nan")
    if not ncc_model.row_ok(lo, hi, n):
        return [(-2, 0, nan)] * k
    left = np.zeros(n, dtype=bool)          # A_j
    left[lo:hi + 1] = True
    out = []
    for _ in range(k):
        if not left.any():
            out.append((-3, 0, nan))
            continue
        cand = left & ~np.isnan(keys)
        if cand.any():
            best = np.where(cand, keys, np.float32(-1.0))
            lag = int(np.argmax(best))      # the first of equal maxima
            peak = float(best[lag])
        else:
            lag, peak = int(np.flatnonzero(left)[0]), 0.0
        out.append((0, lag, peak))
        left[max(0, lag - min_separation):min(n - 1, lag + min_separation) + 1] = False
    return out


def topk(c, vx, vy, k, min_separation, row=None, min_energy=ncc_model.DEFAULT_ENERGY):
    """the rule over the float64 model's curve (ncc_model.curve's result)"""
    return topk_of_keys(keys_of(c, vx, vy, min_energy), k, min_separation, row)


def fixture_c(n, p):
    """-> (source float32 [2N], sample float32 [N], the three planted lags in gain order).  sample = unit noise + 0.25 DC; source =
    unit noise plus 0.3 / 1.0 / 0.6 times the sample at lags N/10 + 17p, N/2 + 5p and 8N/10 - 3p, and +2.0 from frame 1.3 N on."""
    rng = np.random.default_rng(3000 + p)
    smp = rng.standard_normal(n) + 0.25
    src = rng.standard_normal(2 * n)
    lags = (n // 10 + 17 * p, n // 2 + 5 * p, max(0, (8 * n) // 10 - 3 * p))
    for gain, lag in zip(GAINS, lags):
        room = max(0, min(n, 2 * n - lag))   # (all of the sample but at lengths of a few frames, where 17 p lies past the source)
        src[lag:lag + room] += gain * smp[:room]
    src[(13 * n) // 10:] += 2.0
    order = sorted(range(3), key=lambda i: -GAINS[i])
    return src.astype(np.float32), smp.astype(np.float32), tuple(lags[i] for i in order)
