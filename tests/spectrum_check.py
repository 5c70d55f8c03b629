"""Bin-by-bin check of a device correlation against a float64 reference spectrum (test helper, not a conftest).

The time-domain comparisons elsewhere in the suite (max|r_dev - r_ref| / max|r_ref|) average an error over all 2N lags:
an error confined to one frequency bin moves that metric by about 1/2N of its size and passes.  Here the device's r goes
back to the frequency domain in float64 and every bin k = 0 .. F/2 is held against its own error scale:

    z_k = |R_k - P_k| / (u log2 F (eX_k |Y_k| + |X_k| eY_k + eP_k)),   u = 2^-24,
    eX_k = max(rms|X|, rms of |X| over the row of k) + |X_k|   (eY_k the same for Y),
    eP_k = max(rms|P|, rms of |P| over the row of k),

with X = rfft(x), Y = rfft(y zero-padded to F), P = X conj(Y) and R = rfft(r) in float64.  eX_k and eY_k are the forward
transforms' errors at bin k, carried through the product; eP_k is the inverse transform's own error.  A transform's
rounding errors are spread about evenly over the bins (rms over all F bins) -- except where energy is concentrated:
a bin's own value is rounded on its way through every stage (|X_k|), and a row transform's errors scale with the row's
norm (rms over the row).  The last two matter for inputs with a large DC component: the column stage gathers the offset
into row 0, whose bins then carry errors far above the global rms on any float32 FFT (torch's CPU FFT included).  The
row terms come from the float64 reference, never from the device's r: a broken row cannot raise its own limit.

R = X conj(Y) holds only when the plan is not embedded in a longer transform (F == 2N); the helper refuses other plans.

Coordinates of a bin in the plan's split (the message of a failure names them):
  real-column (csrc/rlayout.hip)   k = k1 + 2 M1 k2, k1 < 2 M1, k2 < M2.  Rows k1 = 0 .. M1 are stored; a bin of row
                                   k1 > M1 is the mirror image of bin F - k, row 2 M1 - k1, column M2 - 1 - k2.
  packed (csrc/xcorr_kernels.hip)  k mod M = k1 + M1 k2 (M = F/2, k1 < M1, k2 < M2) of the packed complex transform.
"""
import math

import numpy as np

U = 2.0 ** -24
# Largest z a correct device transform may show at any bin.  Measured on an MI355X: at most 0.52 on white noise, impulse
# pairs and chirps (both layouts, every length and split in test_gpu_transform_spectrum.py), 2.24 on tracks with large DC
# offsets (row M1 of the real-column split: the columns' Nyquist bin, a difference of two sums of the offset).  The
# run-time-schedule kernels (test_gpu_schedule_cover.py): at most 0.44 on white noise (split 125x75x2) and 0.25 on impulse
# pairs (12x400x2) over the 59 forced splits of schedule_cover.CASES, 0.42 over the four longest lengths (N = 4 000 000,
# split 3200x1250x2; 0.40 at 1 953 125, 0.41 at 2 097 152; the embedded 3 999 971 is held in the time domain, 3.1e-7 of
# max |r|).  torch's float32 CPU FFT reaches 0.6 on white noise.  One bin off by 1e-3 relative reaches 19 and more
# (test_spectrum_check.py).
Z_MAX = 8.0


def _rms(S, F):
    """sqrt(mean |S_k|^2) over all F bins of a real sequence's spectrum, from its F/2 + 1 stored bins"""
    w = _weights(S.size, F)
    return math.sqrt(float(np.sum(w * (S.real ** 2 + S.imag ** 2))) / F)


def _weights(size, F):
    """multiplicity of the F/2 + 1 stored bins of a real sequence's spectrum among its F bins"""
    w = np.full(size, 2.0)
    w[0] = 1.0
    if F % 2 == 0:
        w[-1] = 1.0
    return w


def _row_rms(a, rows, F):
    """per bin: rms of a over the bins of its row"""
    w = _weights(a.size, F)
    num = np.bincount(rows, weights=w * a * a)
    den = np.bincount(rows, weights=w)
    return np.sqrt(num / np.maximum(den, 1.0))[rows]


class Reference:
    """the float64 spectra of one input pair: X, Y, P = X conj(Y) (computed once, reused for every r of the same pair)"""

    def __init__(self, x, y):
        x = np.asarray(x)
        y = np.asarray(y)
        assert x.dtype == np.float32 and y.dtype == np.float32, (x.dtype, y.dtype)
        F, N = x.size, y.size
        if F != 2 * N:
            raise ValueError("per-bin check needs F == 2N (got F = %d, N = %d): an embedded plan's r is not X conj(Y)" % (F, N))
        self.F, self.N = F, N
        yp = np.zeros(F, dtype=np.float64)
        yp[:N] = y
        self.X = np.fft.rfft(x.astype(np.float64))
        self.Y = np.fft.rfft(yp)
        self.P = self.X * np.conj(self.Y)
        self._scales = {}

    def scale(self, M1, layout):
        """the denominator of z for every bin, for a plan with M1 rows (of the layout's kind)"""
        key = (M1, layout)
        if key not in self._scales:
            F = self.F
            rows = stored_rows(np.arange(F // 2 + 1), F, M1, layout)
            aX, aY = np.abs(self.X), np.abs(self.Y)
            eX = np.maximum(_rms(self.X, F), _row_rms(aX, rows, F)) + aX
            eY = np.maximum(_rms(self.Y, F), _row_rms(aY, rows, F)) + aY
            aP = np.abs(self.P)
            eP = np.maximum(_rms(self.P, F), _row_rms(aP, rows, F))
            self._scales[key] = U * math.log2(F) * (eX * aY + aX * eY + eP)
        return self._scales[key]

    def r_plain(self):
        """the exact correlation in float64: r[p] = sum_j x[(j + p) mod F] y[j]"""
        return np.fft.irfft(self.P, n=self.F)


def stored_rows(k, F, M1, layout):
    """the stored row (the row kernels' unit of work) that computes bin k (an int or an array)"""
    if layout == "real-column":
        k1 = k % (2 * M1)
        return np.where(k1 <= M1, k1, 2 * M1 - k1)
    if layout == "packed":
        return (k % (F // 2)) % M1
    raise ValueError(layout)


def coords(k, F, M1, M2, layout):
    """(k1, k2) of bin k in the plan's split, and the stored row that computes it"""
    if layout == "real-column":
        k1, k2 = k % (2 * M1), k // (2 * M1)
        return k1, k2, (k1 if k1 <= M1 else 2 * M1 - k1)
    if layout == "packed":
        kk = k % (F // 2)
        return kk % M1, kk // M1, kk % M1
    raise ValueError(layout)


class Result:
    def __init__(self, z, F, M1, M2, layout, label):
        self.z, self.F, self.M1, self.M2, self.layout, self.label = z, F, M1, M2, layout, label
        self.k = int(np.argmax(z))
        self.zmax = float(z[self.k])
        self.k1, self.k2, self.row = coords(self.k, F, M1, M2, layout)
        self.p9999 = float(np.percentile(z, 99.99))
        self.median = float(np.median(z))

    def rows_over(self, limit=Z_MAX, most=16):
        """stored rows (the row kernels' unit of work) holding a bin with z > limit, worst first"""
        ks = np.nonzero(self.z > limit)[0]
        worst = {}
        for k in ks[np.argsort(-self.z[ks])]:
            row = coords(int(k), self.F, self.M1, self.M2, self.layout)[2]
            worst.setdefault(row, float(self.z[k]))
        return sorted(worst, key=lambda r: -worst[r])[:most]

    def summary(self):
        return ("spectrum N=%d F=%d split=%dx%d layout=%s input=%s  max z=%.3f at bin %d (k1=%d, k2=%d)  p99.99=%.3f  median=%.4f"
                % (self.F // 2, self.F, self.M1, self.M2, self.layout, self.label, self.zmax, self.k, self.k1, self.k2,
                   self.p9999, self.median))

    def message(self, limit=Z_MAX):
        mirror = "" if self.k1 == self.row else " (mirror of stored row %d)" % self.row
        return ("%s [%s, split %dx%d]: bin %d of %d, (k1, k2) = (%d, %d)%s has z = %.2f > Z_MAX = %g; "
                "rows with z > %g: %s; 99.99th percentile %.3f, median %.4f"
                % (self.label, self.layout, self.M1, self.M2, self.k, self.F // 2, self.k1, self.k2, mirror, self.zmax,
                   limit, limit, self.rows_over(limit), self.p9999, self.median))


def inputs(kind, n, seed=5, a=None, b=None):
    """float32 (x[2n], y[n]) of one input family:
    W  the production shape (oracle.synth_pair: uniform white noise, the sample a delayed, scaled copy plus noise)
    I  an impulse pair x = e_a, y = e_b (|X_k| = |Y_k| = 1: every twiddle path weighs the same); a = 2n - 1, b = 0 by default
    C  a linear chirp from 0 to Nyquist, the sample its first n values
    D  white noise with offsets +30 (source) and +20 (sample): the DC bin dominates"""
    import oracle
    F = 2 * n
    if kind == "W":
        x, y, _ = oracle.synth_pair(seed, 1, n, 1)
        return x, y
    if kind == "I":
        x = np.zeros(F, dtype=np.float32)
        y = np.zeros(n, dtype=np.float32)
        x[F - 1 if a is None else a] = 1.0
        y[0 if b is None else b] = 1.0
        return x, y
    if kind == "C":
        t = np.arange(F, dtype=np.float64)
        x = np.cos(np.pi * t * t / (2.0 * F)).astype(np.float32)   # instantaneous frequency t / (2F) cycles per sample
        return x, x[:n].copy()
    if kind == "D":
        rng = np.random.default_rng(seed)
        x = (rng.uniform(-1.0, 1.0, F) + 30.0).astype(np.float32)
        y = (rng.uniform(-1.0, 1.0, n) + 20.0).astype(np.float32)
        return x, y
    raise ValueError(kind)


def check(ref, r_plain, M1, M2, layout, label=""):
    """z of every bin of r_plain (the plain sum of products, length F) against `ref` (a Reference of the same inputs)"""
    r = np.asarray(r_plain, dtype=np.float64)
    assert r.size == ref.F, (r.size, ref.F)
    assert M1 * M2 * 2 == ref.F, (M1, M2, ref.F)
    R = np.fft.rfft(r)
    z = np.abs(R - ref.P) / ref.scale(M1, layout)
    return Result(z, ref.F, M1, M2, layout, label)
