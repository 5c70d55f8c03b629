"""Band-limited GCC-PHAT without a GPU: the float64 model of tests/phat_band_model.py on inputs whose answer is known (pure delays pin
the vote count V, low-passed pairs show what the band is for), asx_band_bins, which needs no device, and the census and budgets of the
banded row kernels in the built library (k_rows_rb: a name of its own next to the k_rows_r and k_rows_rp instances)."""
import ctypes
import re

import numpy as np
import pytest

import phat_band_model
import phat_model
from test_kernel_resources import demangled, kernels  # noqa: F401  (the fixture)
from util import asx

N = 6000
LAGS = (0, 1, 777, N - 1, -1, -2500, -N)


def delayed(lag):
    src = np.random.default_rng(5).standard_normal(2 * N)
    return src, np.roll(src, -lag)                      # full[j] = src[j + lag], circular: all 2N samples, nothing is cut off


@pytest.mark.parametrize("band", [(0, N), (1, N), (0, N - 1), (100, 2000)])
def test_a_pure_circular_delay_has_peak_one_whatever_the_band(band):
    """|r| = 1 at the delay only when the divisor is the number of bins that voted: both ends of the band, either end, neither"""
    for lag in LAGS:
        src, full = delayed(lag)
        r = phat_band_model.r_phat_band(src, full, *band)
        ret, got, _, peak = phat_band_model.model(src, full[:N], *band, r=r)
        assert got == lag and abs(peak - 1.0) < 1e-12, (band, lag, got, peak)
        assert abs(r[lag % (2 * N)] - 1.0) < 1e-12
    assert phat_band_model.votes(N, *band) == {(0, N): 2 * N, (1, N): 2 * N - 1, (0, N - 1): 2 * N - 1, (100, 2000): 3802}[band]


def test_a_pure_delay_in_the_single_frequency_bands():
    """One frequency m gives the cosine r[l] = cos(2 pi m (l - lag) / F), whose magnitude is 1 at more lags than one, so the rule,
    which ranks magnitudes, cannot name the lag (rounding decides among the ties); the divisor is pinned all the same: the curve is +1
    at the delay.  [1, 1]: two voters, +1 at the lag, -1 at lag + N, smaller everywhere else.  [N, N]: one voter, +1 and -1 in turn.
    [0, 0]: one voter, a constant curve of magnitude 1."""
    for lag in LAGS:
        src, full = delayed(lag)
        r = phat_band_model.r_phat_band(src, full, 1, 1)
        assert phat_band_model.votes(N, 1, 1) == 2
        assert np.max(np.abs(r - np.cos(np.pi * (np.arange(2 * N) - lag) / N))) < 1e-12
        assert int(np.argmax(r)) == lag % (2 * N) and abs(r[lag % (2 * N)] - 1.0) < 1e-12
        ret, got, _, peak = phat_band_model.model(src, full[:N], 1, 1, r=r)
        assert abs(peak - 1.0) < 1e-12 and got % N == lag % N, (lag, got, peak)
        r = phat_band_model.r_phat_band(src, full, N, N)
        assert phat_band_model.votes(N, N, N) == 1
        assert np.max(np.abs(np.abs(r) - 1.0)) < 1e-12
        want = np.where((np.arange(2 * N) - lag) % 2 == 0, 1.0, -1.0)
        assert np.max(np.abs(r - want)) < 1e-12, lag
        assert abs(phat_band_model.model(src, full[:N], N, N, r=r)[3] - 1.0) < 1e-12
        r = phat_band_model.r_phat_band(src, full, 0, 0)
        assert phat_band_model.votes(N, 0, 0) == 1
        assert np.max(np.abs(np.abs(r) - 1.0)) < 1e-12 and np.max(np.abs(r - r[0])) < 1e-12


def test_the_full_band_is_the_phat_model():
    src, full = delayed(777)
    smp = full[:N] + 0.3 * np.random.default_rng(6).standard_normal(N)
    assert np.max(np.abs(phat_band_model.r_phat_band(src, smp, 0, N) - phat_model.r_phat(src, smp))) < 1e-15
    assert phat_band_model.model(src, smp, 0, N)[:2] == phat_model.model(src, smp)[:2]


def test_low_passed_pairs_need_the_band():
    """three pairs low-passed at bin N/6 over noise of 1e-4, N = 144 000.  Measured: every bin voting 0.041 / 0.027 / 0.096 and pair 0
    one lag off; bins [1, N/6] voting 0.248 / 0.148 / 0.570, every lag the planted one, 0.0103 / 0.0068 / 0.0250 above the runner-up,
    which is the adjacent lag."""
    n = phat_band_model.LOWPASS_N
    wrong = 0
    for p in range(3):
        src, smp, planted = phat_band_model.lowpass_pair(p)
        full = phat_model.model(src, smp)
        r = phat_band_model.r_phat_band(src, smp, 1, n // 6)
        ret, lag, coef, peak = phat_band_model.model(src, smp, 1, n // 6, r=r)
        rest = np.abs(r)
        rest[planted % (2 * n)] = 0.0
        runner = int(np.argmax(rest))
        print("low-passed pair", p, "planted", planted, "full band", full[1], full[3], "banded", lag, peak, "above the rest",
              peak - rest[runner], "runner-up at", runner - planted % (2 * n))
        wrong += full[1] != planted
        assert (ret, lag) == (0, planted), (p, lag, planted)
        assert peak > 4.0 * full[3], (p, peak, full[3])
        assert peak - rest[runner] >= 0.005, (p, peak, rest[runner])
        assert abs(runner - planted % (2 * n)) == 1
    assert wrong == 1


def band_bins_raw(*args):
    lo, hi = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = asx().lib().asx_band_bins(*args, ctypes.byref(lo), ctypes.byref(hi))
    return rc, lo.value, hi.value


def test_band_bins():
    mod = asx()
    assert mod.band_bins(144000, 48000, 0, 4000) == (0, 24000)
    assert mod.band_bins(144000, 48000, 300, 3400) == (1800, 20400)
    assert mod.band_bins(144000, 48000, 300, 24000) == (1800, 144000)      # the Nyquist frequency itself
    assert mod.band_bins(144000, 48000, 300, 30000) == (1800, 144000)      # above it: clamped to N
    assert mod.band_bins(144000, 48000, 0, float("inf")) == (0, 144000)
    assert mod.band_bins(144000, 48000, 100.001, 100.17) == (601, 601)     # ceil below, floor above
    nan = float("nan")
    refused = [(144000, 0.0, 0.0, 4000.0), (144000, -48000.0, 0.0, 4000.0), (144000, 48000.0, -1.0, 4000.0),
               (144000, 48000.0, 4000.0, 300.0), (144000, nan, 0.0, 4000.0), (144000, 48000.0, nan, 4000.0),
               (144000, 48000.0, 0.0, nan), (100, 48000.0, 10.0, 20.0),    # between bins 0 and 1: no bin inside
               (144000, 48000.0, 24000.5, 30000.0)]                        # all of it above the Nyquist frequency
    for args in refused:
        assert band_bins_raw(*args) == (-1, -7, -7), args
        with pytest.raises(ValueError):
            mod.band_bins(*args)
    assert band_bins_raw(144000, 48000.0, 300.0, 3400.0) == (0, 1800, 20400)


def test_banded_row_kernels_census_and_budgets(kernels):  # noqa: F811
    names = {demangled(k): v for k, v in kernels.items()}
    rows = [(n, r) for n, r in names.items() if n.startswith("void k_rows_rb<")]
    assert len(rows) == 12, sorted(n for n, _ in rows)
    forms = set()
    for n, r in rows:
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
        m = re.match(r"void k_rows_rb<(Sched<[^>]*>, \d+), (true|false), (\d)>", n)
        forms.add((m.group(1), m.group(2) == "true", int(m.group(3))))
        # the plain instance of the same form: the same static LDS
        plain = names[next(p for p in names if p.startswith(n.replace("k_rows_rb<", "k_rows_r<").split("(")[0] + "("))]
        assert r["group_segment_fixed_size"] == plain["group_segment_fixed_size"], (n, r, plain)
    assert len({f[:2] for f in forms}) == 3 and {f[2] for f in forms} == {0, 1, 2, 3}, forms
    assert len([n for n in names if n.startswith("void k_rows_rp<")]) == 12
    assert len([n for n in names if n.startswith("void k_rows_r<")]) == 12
    assert len([n for n in names if n.startswith("void k_phat_finalize<")]) == 2


def test_the_python_surface_names_the_three_calls():
    mod = asx()
    from audiosync_amd import hipxcorr
    calls = ("asx_xcorr_phat_band_f32_dev", "asx_xcorr_phat_band_debug_r_dev", "asx_band_bins")
    assert set(calls) <= set(hipxcorr.ABI_SYMBOLS)
    for name in ("xcorr_phat_band_dev", "phat_band_debug_r_dev", "xcorr_phat_band_f32"):
        assert callable(getattr(mod.Plan, name)), name
    assert callable(mod.band_bins)
    assert all(hasattr(mod.lib(), name) for name in calls)
    assert mod.abi_version() == 2
