"""float64 model of asx_xcorr_track_f32_dev (include/audiosync/xcorr_hip.h): the curve call's sum kept apart per time segment,
r_s[d] = sum_{b_s <= n < b_{s+1}} source[(n + p + d) mod 2N] * sample[n] with b_s = floor(s N / S), summed with math.fsum over the
float64 products (exact for float32 inputs); each segment's peak, offset and weight by the header's rule (phat_sub_model.frac_of for the
parabola); and the weighted least-squares line through (t_s, off_s) of the used segments, its sums with math.fsum.  The tolerance
functions are first-order worst cases of any float64 evaluation order, with or without fused multiply-add."""
import math

import numpy as np

import curve_model
import phat_sub_model

HALF_MAX = 64
SEG_MAX = 64
EPS = 2.0 ** -53


def bounds(n, segments):
    """b_0 .. b_S: segment s is the sample's frames [b_s, b_{s+1}), b_s = floor(s N / S) in integers"""
    assert 1 <= segments <= min(SEG_MAX, n)
    return [s * int(n) // int(segments) for s in range(segments + 1)]


def times(n, segments):
    """t_s = (b_s + b_{s+1} - 1) / 2, the mean frame index of segment s"""
    b = bounds(n, segments)
    return [(b[s] + b[s + 1] - 1) / 2 for s in range(segments)]


def offsets(h):
    return list(range(-h, h + 1))


def indices(lag, n, h):
    """the 2h + 1 indices around the lag's index, d = -h .. h, circular over 2N"""
    assert 1 <= h <= HALF_MAX
    return [(curve_model.index_of(lag, n) + d) % (2 * n) for d in offsets(h)]


def r_seg(source, sample, idx, b0, b1):
    """-> (r_s at index idx over the frames [b0, b1) correctly rounded, sum of the |products| of its terms)"""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(sample, dtype=np.float64)
    n = t.size
    prod = s[(np.arange(b0, b1) + int(idx)) % (2 * n)] * t[b0:b1]
    return math.fsum(prod), float(math.fsum(np.abs(prod)))


def tol_r(length, sum_abs):
    """len_s * 2^-53 * sum |products|"""
    return length * EPS * sum_abs


def track_r(source, sample, lag, h, segments):
    """-> (r [S, 2h + 1], tol [S, 2h + 1]) around `lag`"""
    n = np.asarray(sample).size
    b = bounds(n, segments)
    idx = indices(lag, n, h)
    r = np.zeros((segments, 2 * h + 1))
    tol = np.zeros_like(r)
    for s in range(segments):
        for j, i in enumerate(idx):
            v, a = r_seg(source, sample, i, b[s], b[s + 1])
            r[s, j] = v
            tol[s, j] = tol_r(b[s + 1] - b[s], a)
    return r, tol


def seg_rule(r_s, h):
    """one segment's 2h + 1 values -> (off, w, used): the peak m is the d with the largest |r_s[d]| scanned from -h upwards with a
    strict > (the smallest d wins ties, an all-zero segment gives -h), w = |r_s[m]|, off = m + frac at an interior peak and m at an
    edge; used: an interior peak and every value finite"""
    y = [float(v) for v in r_s]
    assert len(y) == 2 * h + 1
    m, best = 0, abs(y[0])
    for j in range(1, len(y)):
        if abs(y[j]) > best:
            m, best = j, abs(y[j])
    interior = 0 < m < 2 * h
    off = float(m - h)
    if interior:
        off = float(m - h) + phat_sub_model.frac_of(y[m - 1], y[m], y[m + 1])
    return off, abs(y[m]), bool(interior and all(math.isfinite(v) for v in y))


def seg_of(r, h):
    """r [S, 2h + 1] -> (seg [S, 2] = {off, w}, used [S] of bool)"""
    rows = [seg_rule(row, h) for row in np.asarray(r, dtype=np.float64)]
    return np.array([[o, w] for o, w, _ in rows]), np.array([u for _, _, u in rows], dtype=bool)


def fit(t, off, w, used):
    """the weighted line through (t_s, off_s) over the used segments, ascending s -> dict(drift, lag0, rms, rms2, tbar, ybar, Stt, W);
    the first three NaN with fewer than two used segments"""
    k = [s for s in range(len(t)) if used[s]]
    nan = float("nan")
    if len(k) < 2:
        return dict(drift=nan, lag0=nan, rms=nan, rms2=nan, tbar=nan, ybar=nan, Stt=nan, W=nan, count=len(k))
    t = [float(t[s]) for s in k]
    y = [float(off[s]) for s in k]
    w = [float(w[s]) for s in k]
    W = math.fsum(w)
    tbar = math.fsum(a * b for a, b in zip(w, t)) / W
    ybar = math.fsum(a * b for a, b in zip(w, y)) / W
    Stt = math.fsum(a * (b - tbar) ** 2 for a, b in zip(w, t))
    Sty = math.fsum(a * (b - tbar) * (c - ybar) for a, b, c in zip(w, t, y))
    drift = Sty / Stt
    lag0 = ybar - drift * tbar
    rms2 = math.fsum(a * (c - (lag0 + drift * b)) ** 2 for a, b, c in zip(w, t, y)) / W
    return dict(drift=drift, lag0=lag0, rms=math.sqrt(rms2), rms2=rms2, tbar=tbar, ybar=ybar, Stt=Stt, W=W, count=len(k))


def fit_tolerances(t, off, w, used, f, segments):
    """-> (tol_drift, tol_lag0, tol_rms2) for the fit f of these segments, S = segments:
    tol_drift = 64 S 2^-53 sum w (|t| + |tbar|)(|off| + |ybar|) / Stt
    tol_lag0  = 2 |tbar| tol_drift + 64 S 2^-53 (|ybar| + |drift tbar|)
    tol_rms2  = 64 S 2^-53 max (|off| + |lag0| + |drift t|)^2"""
    k = [s for s in range(len(t)) if used[s]]
    c = 64.0 * segments * EPS
    tbar, ybar, drift, lag0 = f["tbar"], f["ybar"], f["drift"], f["lag0"]
    td = c * math.fsum(float(w[s]) * (abs(float(t[s])) + abs(tbar)) * (abs(float(off[s])) + abs(ybar)) for s in k) / f["Stt"]
    tl = 2.0 * abs(tbar) * td + c * (abs(ybar) + abs(drift * tbar))
    tr = c * max((abs(float(off[s])) + abs(lag0) + abs(drift * float(t[s]))) ** 2 for s in k)
    return td, tl, tr


def track(source, sample, lag, h, segments):
    """-> (r [S, 2h + 1], tol, seg [S, 2], used [S], fit dict) around `lag`"""
    n = np.asarray(sample).size
    r, tol = track_r(source, sample, lag, h, segments)
    seg, used = seg_of(r, h)
    return r, tol, seg, used, fit(times(n, segments), seg[:, 0], seg[:, 1], used)
