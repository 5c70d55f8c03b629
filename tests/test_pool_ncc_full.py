"""Full-range normalised cross-correlation over track pools (asx_xcorr_pool_ncc_full_f32_dev and its top-k form), the parts that need
no GPU: on fixture F of tests/ncc_pool_full_model.py the float64 models alone show what the call buys -- the full-range tables hold
every true lag and triangle closure places all four clips, while the raw top-k tables and the NCC tables of the lags 0..N-1 do not --,
the library exports the calls, the host checks raise before anything is uploaded, and the built code object holds the new kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import closure_model
import ncc_pool_full_model as pm
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_pool_ncc_full_f32_dev", "asx_xcorr_pool_ncc_full_topk_f32_dev")
KERNELS = ("k_nccfp_peak",)


# ---- A. the references alone meet the premise -----------------------------------------------------------------------------------------

def test_the_full_range_tables_hold_every_true_lag_and_closure_places_every_clip():
    t = pm.full_tables()
    pm.check_premise(t)
    # the figures DESIGN.md quotes: (decoy lag, decoy peak, true lag, true peak) to three decimals
    want = {(0, 1): (50000, 0.429, 20000, 0.302), (0, 3): (60000, 0.402, 70000, 0.205), (3, 0): (-60000, 0.763, -70000, 0.215)}
    for (a, b), row in want.items():
        got = (int(t["lag"][a, b, 0]), round(float(t["peak"][a, b, 0]), 3), int(t["lag"][a, b, 1]), round(float(t["peak"][a, b, 1]), 3))
        assert got == row, (a, b, got)
    off = ~np.eye(pm.C, dtype=bool)
    others = [(a, b) for a in range(pm.C) for b in range(pm.C) if a != b and (a, b) not in pm.DECOYS]
    assert min(t["peak"][a, b, 0] for a, b in others) >= 0.26
    noise = [t["peak"][a, b, j] for a in range(pm.C) for b in range(pm.C) for j in range(pm.K)
             if t["lag"][a, b, j] != pm.true_lags()[a, b] and not ((a, b) in pm.DECOYS and j == 0)]
    assert max(noise) <= 0.021
    c = pm.close(t)
    assert pm.right_picks(c) == 16 and np.array_equal(c["best_lag"], pm.true_lags())
    entry = np.zeros((pm.C, pm.C), dtype=np.int32)
    for a, b in pm.DECOYS:
        entry[a, b] = 1
    assert np.array_equal(c["best_entry"], entry)
    assert np.array_equal(c["confirm"], np.where(off, 3, 0))
    assert c["root"] == 0 and c["offset"].tolist() == list(pm.OFFSETS) and c["support"].tolist() == [0, 6, 6, 6]
    assert c["placed"].tolist() == [1] * pm.C
    # the coefficient alone takes entry 0 everywhere: wrong in exactly the three decoy pairs
    by_coef = closure_model.by_coefficient(t["coef"], t["ret"])
    assert not by_coef.any()
    wrong = np.take_along_axis(t["lag"], by_coef[:, :, None].astype(np.int64), axis=2)[:, :, 0] != pm.true_lags()
    assert sorted(zip(*np.nonzero(wrong))) == sorted(pm.DECOYS)


def test_the_raw_tables_lose_every_true_lag_to_the_level_step():
    t = pm.raw_tables()
    want = pm.true_lags()
    for a in range(pm.C):
        for b in range(pm.C):
            if a != b:
                assert want[a, b] not in t["lag"][a, b].tolist(), (a, b, t["lag"][a, b])
    c = pm.close(t)
    assert pm.right_picks(c) == 3
    assert c["placed"][3] == 1 and int(c["offset"][3]) == 60000          # clip 3 sits on the decoy


def test_the_ncc_tables_of_the_lags_from_zero_miss_every_negative_true_lag():
    t = pm.half_tables()
    want = pm.true_lags()
    negative = [(a, b) for a in range(pm.C) for b in range(pm.C) if want[a, b] < 0]
    assert len(negative) == 6
    for a, b in negative:
        assert (t["lag"][a, b] >= 0).all() and want[a, b] not in t["lag"][a, b].tolist()
    c = pm.close(t)
    assert pm.right_picks(c) == 9
    assert c["placed"][2] == 0 and c["root"] != 0                         # clip 2 is not placed, and the root is not clip 0


# ---- B. surface -------------------------------------------------------------------------------------------------------------------

def test_the_calls_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS and name in hipxcorr.SIGNATURES, name
        assert hasattr(L, name), name
    assert hasattr(L, "asx_plan_debug_ncc_full") and "asx_plan_debug_ncc_full" in hipxcorr.SIGNATURES
    assert "asx_plan_debug_ncc_full" not in hipxcorr.ABI_SYMBOLS
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_pool_ncc_full_dev", "xcorr_pool_ncc_full_topk_dev", "xcorr_pool_ncc_full_f32", "xcorr_pool_ncc_full_topk_f32",
                 "debug_ncc_full"):
        assert callable(getattr(m.Plan, name)), name
    assert m.pool_ncc_full_args is hipxcorr.pool_ncc_full_args and m.pool_ncc_full_topk_args is hipxcorr.pool_ncc_full_topk_args
    assert m.Plan.NCC_POOL_TABLE_SETS == {"pool_full": 3} and "pool_full" not in m.Plan.NCC_TABLE_SETS
    vp = ctypes.c_void_p
    a = hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_full_f32_dev"][1]
    assert a[:11] == hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_f32_dev"][1][:11]
    assert a[11:13] == [ctypes.c_double, ctypes.c_int64] and a[13:] == [vp] * 5
    a = hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_full_topk_f32_dev"][1]
    assert a[:11] == hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_f32_dev"][1][:11]
    assert a[11:15] == [ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_int64] and a[15:] == [vp] * 5
    flat = re.sub(r"[\s*]+", " ", hdr)
    for phrase in ("Not offered: pools in this call (asx_xcorr_pool_ncc_full_f32_dev",
                   "or those of asx_xcorr_pool_ncc_full_topk_f32_dev",
                   "The tables for closure come from asx_xcorr_pool_ncc_full_topk_f32_dev",
                   "min(asx_plan_group(), 2^30 / 72N) pairs"):
        assert re.sub(r"[\s*]+", " ", phrase) in flat, phrase
    assert "no pool form yet" not in flat


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_pool_ncc_full_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_pool_ncc_full_topk_dev(self, *a, **kw):
        raise AssertionError("called")


def test_the_checks_come_before_anything_is_uploaded():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((3, 32), np.float32), samples=np.zeros((2, 16), np.float32))
    bad = [dict(sources=np.zeros(32, np.float32)), dict(sources=np.zeros((3, 31), np.float32)), dict(samples=np.zeros((2, 15), np.float32)),
           dict(samples=np.zeros((0, 16), np.float32)), dict(pairs=np.zeros((4, 3), np.int32)), dict(pairs=np.zeros((0, 2), np.int32)),
           dict(pairs=np.zeros((4, 2), np.float32)), dict(pairs=np.array([[0, 2 ** 31]])), dict(pairs=[0, 1]),
           dict(min_energy=0), dict(min_energy=1e-7), dict(min_energy=1.5), dict(min_energy=float("nan")), dict(min_energy=True),
           dict(min_energy="1e-3"), dict(min_overlap=0), dict(min_overlap=17), dict(min_overlap=-1), dict(min_overlap=2.0),
           dict(min_overlap=True), dict(min_overlap="8"), dict(windows=np.zeros(3, np.int64)), dict(windows=np.zeros((5, 2), np.int64)),
           dict(windows=np.zeros((6, 2), np.float64))]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_pool_ncc_full_f32(NoDevice(), **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.pool_ncc_full_args(16, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_pool_ncc_full_topk_f32(NoDevice(), k=2, min_separation=1, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.pool_ncc_full_topk_args(16, k=2, min_separation=1, **args)
    for k, sep in ((0, 1), (9, 1), (2, -1), (True, 1), (2, 1.5), (2.0, 1)):
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.pool_ncc_full_topk_args(16, k=k, min_separation=sep, **good)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_pool_ncc_full_topk_f32(NoDevice(), k=k, min_separation=sep, **good)
    out = hipxcorr.pool_ncc_full_args(16, good["sources"], good["samples"], [[2, 1], [0, 0]], [[-15, 3], [2, 15]], np.float32(0.5),
                                      np.int64(16))
    assert out[4:] == (2, 1, 0.5, 16) and type(out[7]) is int and out[2].dtype == np.int32 and out[3].dtype == np.int64
    out = hipxcorr.pool_ncc_full_args(16, np.zeros((3, 32)), np.zeros((2, 16)))
    assert out[2:] == (None, None, 6, 0, 1e-3, 8) and out[0].dtype == np.float32
    assert hipxcorr.pool_ncc_full_args(15, np.zeros((1, 30)), np.zeros((1, 15)))[7] == 8          # None: (N + 1) // 2
    assert hipxcorr.pool_ncc_full_topk_args(16, good["sources"], good["samples"], 8, 0, min_overlap=1)[4:] == (6, 0, 1e-3, 1, 8, 0)


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_the_pool_full_range_kernel_is_built_within_its_budget():
    """k_nccfp_peak is the family's one kernel: the staging, prefix, finalize, scan, step and invalid kernels of a pool group are the
    strided call's (k_nccfull_*), which read a track through pointers the launcher offsets, or no track at all"""
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_nccfp_", n)}
    assert sorted(re.match(r"(?:void )?(k_nccfp_\w+)", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    # the strided kernel it shares its body with keeps the resources it had
    full = [r for n, r in names.items() if re.match(r"(void )?k_nccfull_peak", n)]
    assert len(full) == 1 and full[0]["private_segment_fixed_size"] == 0 and full[0]["vgpr_count"] <= 128
