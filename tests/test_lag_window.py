"""Lag window of the peak search (asx_plan_set_lag_window), the parts that need no GPU: the C-ABI and the host library export
the new calls, the windowed inverse column kernels are built and keep their budgets, and the float64 model of the rule that
tests/test_gpu_lag_window.py checks the device against is the reference's own answer for the full window."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from lag_window_model import model, window_indices, window_peak
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft, kernel_forms

NEW_ABI = ("asx_plan_set_lag_window", "asx_plan_lag_window", "asx_stream_set_lag_window")


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in NEW_ABI:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert m.lib().asx_abi_version() == 2
    host = open(os.path.join(ROOT, "include", "audiosync", "audiosync.h")).read()
    H = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync.so"))
    for name in ("audiosync_set_max_lag_ms", "audiosync_get_max_lag_ms"):
        assert re.search(r"\b%s\s*\(" % name, host), name
        assert hasattr(H, name), name


def test_max_lag_setting_round_trips_on_the_host():
    H = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync.so"))
    H.audiosync_set_max_lag_ms.argtypes = [ctypes.c_long]
    H.audiosync_get_max_lag_ms.restype = ctypes.c_long
    assert H.audiosync_get_max_lag_ms() == 0
    H.audiosync_set_max_lag_ms(2500)
    assert H.audiosync_get_max_lag_ms() == 2500
    H.audiosync_set_max_lag_ms(0)
    assert H.audiosync_get_max_lag_ms() == 0


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def test_windowed_inverse_kernels_exist_and_keep_the_budgets_of_their_unwindowed_forms(kernels):
    """the window form beside every plain instance of k_inv_cols_r (<..., AsxWin> beside <..., AsxSelAll>) and of k_inv_cols
    (the same two selections), same template arguments: same LDS (so the same blocks per CU by tile), <= 128 VGPRs, no scratch"""
    pairs = 0
    for family in ("k_inv_cols_r", "k_inv_cols"):
        base = kernel_forms(kernels, family, "all")
        wind = kernel_forms(kernels, family, "window")
        assert base and set(base) == set(wind), (family, sorted(base), sorted(wind))
        for k, rs in wind.items():
            ((_, r),), ((_, b),) = rs, base[k]
            assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (family, k, r)
            assert r["group_segment_fixed_size"] == b["group_segment_fixed_size"], (family, k, r, b)
            pairs += 1
    assert pairs == 3 + 8, pairs


def brute_peak(r, n, lo, hi):
    """the rule written out as the reference's loop (src/cross_correlation.c:52-67) over the in-window indices"""
    idx = window_indices(n, lo, hi)
    best, at = r[idx[0]], idx[0]
    for i in idx[1:]:
        if abs(r[i]) > best:
            best, at = abs(r[i]), i
    return int(at)


def test_full_window_model_is_the_reference_at_the_known_answer_lengths(kat):
    for case in kat["cross_correlation"]:
        src, smp = np.asarray(case["source"], dtype=np.float64), np.asarray(case["sample"], dtype=np.float64)
        ret, lag, coef = oracle.cross_correlation(src, smp)
        mret, mlag, mcoef = model(src, smp)
        assert (mret, mlag) == (ret, lag), case["name"]
        assert (mcoef == coef) or (mcoef != mcoef and coef != coef), case["name"]


@pytest.mark.parametrize("n", [7, 64, 1000, 4801])
def test_window_model_follows_the_rule(n):
    rng = np.random.default_rng(n)
    src, smp, _ = oracle.synth_pair(77, 0, n, 1)
    r = oracle.cross_correlation(src, smp, want_results=True)[3]
    assert window_peak(r, n, -n, n - 1) == oracle.max_abs_index(r)
    for _ in range(20):
        lo, hi = sorted(int(v) for v in rng.integers(-n, n, 2))
        assert window_peak(r, n, lo, hi) == brute_peak(r, n, lo, hi), (lo, hi)
    # the seed is signed: a large negative value there loses to a smaller |r| later in the window
    rr = np.zeros(2 * n)
    rr[3], rr[5] = -10.0, 1.0
    assert window_peak(rr, n, 3, 5) == 5 and window_peak(rr, n, 4, 5) == 5 and window_peak(rr, n, 3, 4) == 4
    # silent: the seed; a window that straddles 0 starts at index 0
    z = np.zeros(2 * n)
    assert window_peak(z, n, 2, 5) == 2 and window_peak(z, n, -3, -1) == 2 * n - 3 and window_peak(z, n, -3, 2) == 0
