"""Full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev, its top-k form and its debug call), the parts that need no
GPU: the float64 model of tests/ncc_full_model.py is the reference's coefficient at every lag -(N-1)..N-1, fixture D hides a negative
lag from the raw search and from the NCC model of the lags >= 0 but not from the full-range model, fixture E's two copies stand clear
of everything else, the host checks raise before anything is uploaded, the library exports the three calls, and the built code object
holds the k_nccfull_* kernels within the budget of the k_ncc family."""
import ctypes
import os
import re

import numpy as np
import pytest

import ncc_full_model as fm
import ncc_model
import oracle
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_ncc_full_f32_dev", "asx_xcorr_ncc_full_topk_f32_dev", "asx_xcorr_ncc_full_debug_c_dev")
KERNELS = ("k_nccfull_stage", "k_nccfull_prefix", "k_nccfull_peak", "k_nccfull_finalize", "k_nccfull_invalid", "k_nccfull_scan",
           "k_nccfull_step")
MARGIN = 0.2


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 16, 300])
def test_the_models_curve_is_the_references_coefficient_at_every_lag(n):
    """c[l] against pearson_coefficient() of the reference's segments (src/cross_correlation.c:256-271) at every lag -(N-1)..N-1,
    within 1e-11 (a two-frame overlap divides by an energy of two frames); the lags >= 0 are tests/ncc_model.py's in every bit"""
    src, smp, _ = oracle.synth_pair(23, 4, n, 1)
    cv = fm.curve(src, smp)
    c = cv[0]
    assert c.shape == (2 * n - 1,) and c[n - 1:].tobytes() == ncc_model.curve(src, smp)[0].tobytes()
    worst = 0.0
    for lag in range(-(n - 1), n):
        want = fm.coefficient(src, smp, lag)
        got = c[lag + n - 1]
        if want != want:                        # (an overlap of one frame: 0 / 0)
            continue
        worst = max(worst, abs(got - want))
    print("ncc full model N", n, "worst |c - pearson_coefficient|", worst)
    assert worst <= 1e-11


def test_the_models_rules_at_the_edges():
    n = 16
    src, smp, _ = oracle.synth_pair(23, 5, n, 1)
    cv = fm.curve(src, smp)
    ok = fm.competing(cv, min_overlap=4)
    assert not ok[:3].any() and ok[3:].all()                      # overlaps 1..3 are below min_overlap = 4
    assert fm.competing(cv, min_overlap=n)[:n - 1].sum() == 0     # min_overlap = N: no negative lag
    full = fm.model(src, smp, min_overlap=4, cv=cv)
    assert fm.model(src, smp, row=(full[1], full[1]), min_overlap=4, cv=cv) == full
    assert fm.model(src, smp, row=(-(n - 1), n - 1), min_overlap=4, cv=cv) == full
    for row in ((-n, 5), (0, n), (7, 3)):
        got = fm.model(src, smp, row=row)
        assert got[:2] == (-2, 0) and got[2] != got[2] and got[3] != got[3]
    # a row inside [0, N-1] is the NCC model's answer
    assert fm.model(src, smp, row=(2, 9), cv=cv) == ncc_model.model(src, smp, row=(2, 9))
    # no lag competes: a constant sample, a silent source, one frame
    flat = fm.model(src, np.full(n, 0.25, np.float32), row=(-3, 9))
    assert flat[:2] == (-1, -3) and flat[3] == 0.0 and flat[2] != flat[2]
    silent = fm.model(np.zeros(2 * n, np.float32), smp)
    assert silent[1] == -(n - 1) and silent[3] == 0.0
    one = fm.model(np.array([1.0, 2.0], np.float32), np.array([3.0], np.float32))
    assert one[1] == 0 and one[3] == 0.0
    # a source whose first N frames are silent: no negative lag competes, the others do
    quiet = src.copy()
    quiet[:n] = 0.0
    ok = fm.competing(fm.curve(quiet, smp), min_overlap=1)
    assert not ok[:n - 1].any() and ok[n:].all()
    # top-k: zones do not wrap between N-1 and -(N-1), -3 behind an empty A_j
    tk = fm.topk(src, smp, 3, 2 * n, min_overlap=1, cv=cv)
    assert tk[0][0] == 0 and [e[0] for e in tk[1:]] == [-3, -3]
    tk = fm.topk(src, smp, 3, 2, row=(n - 3, n - 1), min_overlap=1, cv=cv)
    assert tk[0][0] == 0 and all(n - 3 <= e[1] <= n - 1 for e in tk if e[0] == 0)


@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("n", [1000, 2049, 5000])
def test_fixture_d_needs_the_negative_lags(n, p):
    src, smp, planted = fm.fixture_d(n, p)
    assert planted == -(n // 5 + 7 * p)
    cv = fm.curve(src, smp)
    for mo in (n // 2, n // 4):
        ok = fm.competing(cv, min_overlap=mo)
        ret, lag, coef, peak = fm.model(src, smp, min_overlap=mo, cv=cv)
        second = fm.runner_up(cv, ok, lag)
        print("fixture d", n, p, "min_overlap", mo, "planted", planted, "full", lag, "|c|", peak, "next best", second)
        assert (ret, lag) == (0, planted) and peak - second >= MARGIN
        assert abs(coef - cv[0][lag + n - 1]) <= 1e-9
    # the model of the lags >= 0 finds nothing to speak of
    assert ncc_model.model(src, smp)[3] < 0.2
    # the float64 raw argmax over the circular r is fooled by the level step
    r = np.asarray(oracle.cross_correlation(src, smp, want_results=True)[3], dtype=np.float64)
    raw = int(np.argmax(np.abs(r)))
    raw = raw if raw < n else raw - 2 * n
    print("fixture d", n, p, "raw argmax", raw)
    assert raw != planted


@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("n", [1000, 2049, 5000])
def test_fixture_e_holds_a_copy_on_each_side_of_zero(n, p):
    src, smp, lags = fm.fixture_e(n, p)
    assert lags[0] < 0 < lags[1]
    cv = fm.curve(src, smp)
    sep = 50
    tk = fm.topk(src, smp, 2, sep, min_overlap=n // 2, cv=cv)
    assert [e[:2] for e in tk] == [(0, lags[0]), (0, lags[1])], tk
    ok = fm.competing(cv, min_overlap=n // 2)
    for lag in lags:
        ok[lag + n - 1 - sep:lag + n + sep] = False
    rest = float(np.max(np.where(ok, np.abs(cv[0]), -1.0)))
    print("fixture e", n, p, "entries", [e[3] for e in tk], "best outside the zones", rest)
    assert min(e[3] for e in tk) - rest >= MARGIN


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
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_ncc_full_dev", "xcorr_ncc_full_topk_dev", "ncc_full_debug_c_dev", "xcorr_ncc_full_f32", "xcorr_ncc_full_topk_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert m.ncc_full_args is hipxcorr.ncc_full_args and m.ncc_full_topk_args is hipxcorr.ncc_full_topk_args
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_full_f32_dev"][1]
    assert a[8:10] == [ctypes.c_double, ctypes.c_int64] and a[10:] == [ctypes.c_void_p] * 5
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_full_topk_f32_dev"][1]
    assert a[8:12] == [ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    assert hipxcorr.SIGNATURES["asx_xcorr_ncc_full_debug_c_dev"][1][3:5] == [ctypes.c_double, ctypes.c_int64]
    flat = re.sub(r"[\s*]+", " ", hdr)
    for phrase in ("-(N-1) <= l <= N-1", "Lag -N has no overlap", "rlo32[2N + l]", "m >= min_overlap",
                   "Vx[l] * Vy[l] >= min_energy * Vmax * Vy", "1 <= min_overlap <= N", "-(N-1) <= lag_min <= lag_max <= N-1",
                   "the smallest (most negative) lag", "no wrap between N-1 and -(N-1)", "72N bytes", "Not offered: pools"):
        assert re.sub(r"[\s*]+", " ", phrase) in flat, phrase


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_ncc_full_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_ncc_full_topk_dev(self, *a, **kw):
        raise AssertionError("called")


def test_the_checks_come_before_anything_is_uploaded():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32))
    bad = [dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
           dict(min_energy=0), dict(min_energy=1e-7), dict(min_energy=1.5), dict(min_energy=float("nan")), dict(min_energy=True),
           dict(min_overlap=0), dict(min_overlap=17), dict(min_overlap=-1), dict(min_overlap=2.0), dict(min_overlap=True),
           dict(min_overlap="8"), dict(windows=np.zeros(3, np.int64)), dict(windows=np.zeros((3, 2), np.int64)),
           dict(windows=np.zeros((2, 2), np.float64))]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_full_f32(NoDevice(), **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_full_args(16, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_full_topk_f32(NoDevice(), k=2, min_separation=1, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_full_topk_args(16, k=2, min_separation=1, **args)
    for k, sep in ((0, 1), (9, 1), (2, -1), (True, 1), (2, 1.5)):
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_full_topk_args(16, k=k, min_separation=sep, **good)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_full_topk_f32(NoDevice(), k=k, min_separation=sep, **good)
    out = hipxcorr.ncc_full_args(16, good["source"], np.zeros(16), [[-15, 3], [2, 15]], np.float32(0.5), np.int64(16))
    assert out[3:] == (2, 32, 0, 1, 0.5, 16) and type(out[8]) is int and out[2].dtype == np.int64
    assert hipxcorr.ncc_full_args(16, np.zeros(32), np.zeros(16))[2:] == (None, 1, 0, 0, 0, 1e-3, 8)
    assert hipxcorr.ncc_full_args(15, np.zeros(30), np.zeros(15))[8] == 8          # None: (N + 1) // 2
    assert hipxcorr.ncc_full_topk_args(16, good["source"], good["sample"], 8, 0, min_overlap=1)[7:] == (1e-3, 1, 8, 0)


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_the_full_range_kernels_are_built_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_nccfull_", n)}
    assert sorted(re.match(r"(?:void )?(k_nccfull_\w+)", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
