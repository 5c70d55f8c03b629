"""The per-bin spectrum check (tests/spectrum_check.py) on the CPU: torch's float32 FFT stands in for the device pipeline.

Calibration: a correct float32 pipeline stays far below Z_MAX.  Power: one bin of X conj(Y) off by 1e-3 relative, at each
place of the real-column decomposition that has code of its own (csrc/rlayout.hip), is caught -- and the time-domain metric
of test_gpu_parity.py::test_raw_correlation_matches_oracle, on the same r, is not.  No GPU needed."""
import functools

import numpy as np
import pytest

import spectrum_check as sc
from util import asx

LENGTHS = [144000, 1440000]
DELTA = 1e-3
TIME_DOMAIN_TOL = 2e-5   # test_raw_correlation_matches_oracle's limit on max|r - r_ref| / max|r_ref|


def standin_r(x, y):
    """the device pipeline's stand-in: float32 rfft of both tracks, X conj(Y), float32 irfft (the plain sum of products)"""
    import torch
    F = x.size
    yp = np.zeros(F, dtype=np.float32)
    yp[: y.size] = y
    X = torch.fft.rfft(torch.from_numpy(x))
    Y = torch.fft.rfft(torch.from_numpy(yp))
    return torch.fft.irfft(X * torch.conj(Y), n=F).numpy().astype(np.float64)


def split_of(n):
    d = asx().planmath_describe(n)   # host-only
    assert d["F"] == 2 * n
    return d


@functools.lru_cache(maxsize=None)
def white_baseline(n):
    """(reference spectra, stand-in r, its float32 error) of the production-shaped pair, once per length"""
    x, y = sc.inputs("W", n)
    ref = sc.Reference(x, y)
    r = standin_r(x, y)
    return ref, r, r - ref.r_plain()


def probe_bins(d):
    """half-spectrum bins at the places of the real-column split with code of their own (k = k1 + 2 M1 k2, folded)"""
    F, M1, M2 = d["F"], d["M1"], d["M2"]
    MB = M1 // d["radix1"][-1]   # the innermost column stage's butterflies: u_b = MB/2 pairs with itself

    def fold(k1, k2):
        k = k1 + 2 * M1 * k2
        return k if k <= F // 2 else F - k

    bins = {
        "DC": 0,
        "Nyquist": F // 2,
        "k = M1 (row M1, k2 = 0)": M1,
        "k = 2 M1 (row 0, k2 = 1)": 2 * M1,
        "row MB/2 = %d, k2 = 7 (u_b = MB/2)" % (MB // 2): fold(MB // 2, 7),
        "last bin of row M1 - 1": fold(M1 - 1, M2 - 1),
    }
    if M2 == 2400:   # two 1200-point halves: even k2 from one, odd k2 from the other (k_rows_r, TWO = true)
        bins["row 7, k2 = 100 (even half)"] = fold(7, 100)
        bins["row 7, k2 = 101 (odd half)"] = fold(7, 101)
    return bins


def perturbed_r(ref, err32, k, delta):
    """float64 irfft of X conj(Y) with bin k scaled by (1 + delta), plus the stand-in's float32 error"""
    P = ref.P.copy()
    P[k] *= 1.0 + delta
    return np.fft.irfft(P, n=ref.F) + err32


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", ["W", "I", "C"])
def test_calibration_float32_pipeline_stays_below_a_quarter_of_the_limit(n, kind):
    d = split_of(n)
    if kind == "W":
        ref, r, _ = white_baseline(n)
    else:
        x, y = sc.inputs(kind, n, a=2 * n - 1, b=d["M2"] - 1)
        ref = sc.Reference(x, y)
        r = standin_r(x, y)
    res = sc.check(ref, r, d["M1"], d["M2"], "real-column", kind)
    print(res.summary())
    assert res.zmax <= sc.Z_MAX / 4, res.message(sc.Z_MAX / 4)


@pytest.mark.parametrize("n", LENGTHS)
def test_one_bin_off_by_1e3_is_caught_and_the_time_domain_metric_misses_it(n):
    d = split_of(n)
    ref, r0, err32 = white_baseline(n)
    r_exact = ref.r_plain()
    bins = probe_bins(d)
    assert len(set(bins.values())) == len(bins), bins
    for name, k in bins.items():
        r = perturbed_r(ref, err32, k, DELTA)
        res = sc.check(ref, r, d["M1"], d["M2"], "real-column", "W + bin %d x (1 + %g)" % (k, DELTA))
        assert res.k == k and res.zmax > sc.Z_MAX, (name, res.summary())
        k1, k2, row = sc.coords(k, d["F"], d["M1"], d["M2"], "real-column")
        assert res.rows_over(sc.Z_MAX) == [row], (name, res.message())
        # the known blind spot this check exists for: the old metric passes the same r
        td = np.abs(r - r_exact).max() / np.abs(r_exact).max()
        assert td < TIME_DOMAIN_TOL, (name, td)
        print("%-40s bin %7d (k1=%4d, k2=%4d): z = %7.1f, time-domain metric %.2e" % (name, k, k1, k2, res.zmax, td))


def test_coordinates_of_the_two_layouts():
    F, M1, M2 = 288000, 300, 480
    assert sc.coords(0, F, M1, M2, "real-column") == (0, 0, 0)
    assert sc.coords(M1, F, M1, M2, "real-column") == (M1, 0, M1)
    assert sc.coords(2 * M1 + 30, F, M1, M2, "real-column") == (30, 1, 30)
    assert sc.coords(M1 + 1, F, M1, M2, "real-column") == (M1 + 1, 0, M1 - 1)   # mirror of row M1 - 1
    assert sc.coords(F // 2, F, M1, M2, "real-column") == (0, M2 // 2, 0)
    assert sc.coords(F // 2, F, M1, M2, "packed") == (0, 0, 0)                   # Nyquist comes from packed bin 0
    assert sc.coords(M1 + 5, F, M1, M2, "packed") == (5, 1, 5)


def test_refuses_embedded_plans():
    x = np.zeros(2002, dtype=np.float32)
    y = np.zeros(1000, dtype=np.float32)
    with pytest.raises(ValueError):
        sc.Reference(x, y)
