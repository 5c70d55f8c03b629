"""Ragged normalised cross-correlation (asx_xcorr_ncc_ragged_f32_dev, its top-k form and its debug call), the parts that need no GPU:
the float64 model of tests/ncc_ragged_model.py is the reference's coefficient over the frames two tracks of differing lengths share,
at every lag that exists; with the lengths (2N, N) it is the full-range model; fixture G's premises -- zero padding sends the
full-range model to another lag, the lengths bring the planted one back with a margin --; the host checks raise before anything is
uploaded; the library exports the three calls; the built code object holds the k_nccrag_* kernels within the budget of the k_ncc
family."""
import ctypes
import os
import re

import numpy as np
import pytest

import ncc_full_model as fm
import ncc_ragged_model as rm
import oracle
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_ncc_ragged_f32_dev", "asx_xcorr_ncc_ragged_topk_f32_dev", "asx_xcorr_ncc_ragged_debug_c_dev")
KERNELS = ("k_nccrag_stage", "k_nccrag_moments", "k_nccrag_prefix", "k_nccrag_vmax", "k_nccrag_peak", "k_nccrag_finalize",
           "k_nccrag_seg", "k_nccrag_invalid")
MARGIN = 0.2


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

def lengths_of(n):
    """(Ls, Lm) worth telling apart: the plan's shape, Ls < Lm, Lm = 1, Ls = 1, Ls <= N, both short"""
    return sorted({(2 * n, n), (max(1, n // 2), n), (2 * n, 1), (1, n), (n, max(1, n - 1)), (max(1, (3 * n) // 2), max(1, (2 * n) // 3)),
                   (max(1, 2 * n - 1), max(1, n // 3))})


@pytest.mark.parametrize("n", [1, 2, 3, 16, 300])
def test_the_models_curve_is_the_references_coefficient_of_the_shared_frames(n):
    """c[l] against pearson_coefficient() of source[n0 + l, n1 + l) and sample[n0, n1) at every lag that exists, within 1e-11; the
    lags with m <= 0 are NaN; frames beyond the lengths are never read (they hold NaN)"""
    src, smp, _ = oracle.synth_pair(29, 4, n, 1)
    worst = 0.0
    for ls, lm in lengths_of(n):
        s, t = src.copy(), smp.copy()
        s[ls:] = np.nan
        t[lm:] = np.nan
        cv = rm.curve(s, t, ls, lm)
        c, m = cv[0], cv[4]
        assert c.shape == (2 * n - 1,)
        for lag in range(-(n - 1), n):
            got = c[lag + n - 1]
            n0, n1 = max(0, -lag), min(lm, ls - lag)
            assert m[lag + n - 1] == n1 - n0
            if n1 <= n0:
                assert got != got, (n, ls, lm, lag)
                continue
            want = rm.coefficient(s, t, lag, ls, lm)
            if want != want or n1 - n0 < 2:                  # (a constant or one-frame segment: 0 / 0)
                continue
            worst = max(worst, abs(got - want))
    print("ncc ragged model N", n, "worst |c - pearson_coefficient|", worst)
    assert worst <= 1e-11


@pytest.mark.parametrize("n", [3, 16, 300, 2049])
def test_at_the_plans_shape_the_model_is_the_full_range_model(n):
    for k in range(3):
        src, smp, _ = oracle.synth_pair(29, 5 + k, n, 1)
        for mo in (1, fm.default_overlap(n), n):
            want = fm.model(src, smp, min_overlap=mo)
            got = rm.model(src, smp, 2 * n, n, min_overlap=mo)
            assert got[:2] == want[:2] and abs(got[3] - want[3]) <= 1e-9, (n, k, mo, got, want)
            assert got[2] == want[2] or (got[2] != got[2] and want[2] != want[2])
    d_src, d_smp, planted = fm.fixture_d(max(n, 300), 0)
    m = d_smp.size
    got, want = rm.model(d_src, d_smp, 2 * m, m), fm.model(d_src, d_smp)
    assert got[1] == want[1] == planted and abs(got[3] - want[3]) <= 1e-9


def test_the_models_rules_at_the_edges():
    n = 16
    src, smp, _ = oracle.synth_pair(29, 9, n, 1)
    nan = float("nan")
    for ls, lm in ((0, n), (2 * n + 1, n), (2 * n, n + 1), (2 * n, 0), (-1, 3)):
        assert not rm.lens_ok(ls, lm, n)
        got = rm.topk(src, smp, ls, lm, 2, 1, row=(-99, 99))            # -5 over -2
        assert [e[:2] for e in got] == [(-5, 0)] * 2 and all(e[2] != e[2] and e[3] != e[3] for e in got)
    # a short sample under the default min_overlap: only the lags of full overlap compete (template matching)
    ls, lm = 2 * n, 5
    cv = rm.curve(src, smp, ls, lm)
    ok = rm.competing(cv, ls, lm)
    assert ok[n - 1:].all() and not ok[:n - 1].any() and (cv[4][n - 1:] == lm).all()
    assert rm.competing(cv, ls, lm, min_overlap=2)[n - 1 - 3:].all() and not rm.competing(cv, ls, lm, min_overlap=2)[:n - 1 - 3].any()
    # a short source: the lags at and beyond Ls do not exist; a returned lag that does not exist has an empty segment
    ls, lm = 6, n
    cv = rm.curve(src, smp, ls, lm)
    assert np.isnan(cv[0][ls + n - 1:]).all() and (cv[4][ls + n - 1:] <= 0).all()
    got = rm.model(src, smp, ls, lm, row=(ls, n - 1), cv=cv)
    assert got[:2] == (-1, ls) and got[2] != got[2] and got[3] == 0.0
    # rows, top-k and -3 as in the full-range model
    full = rm.model(src, smp, 20, 9, min_overlap=3)
    assert rm.model(src, smp, 20, 9, row=(full[1], full[1]), min_overlap=3) == full
    assert rm.model(src, smp, 20, 9, row=(-n, 3))[:2] == (-2, 0)
    tk = rm.topk(src, smp, 20, 9, 3, 2 * n, min_overlap=3)
    assert tk[0] == full and [e[0] for e in tk[1:]] == [-3, -3] and nan != tk[1][3]
    # Lm = 1: no energy, nothing competes
    one = rm.model(src, smp, 2 * n, 1)
    assert one[1] == -(n - 1) and one[3] == 0.0


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("n", [64, 1000, 2049, 5000])
def test_fixture_g_needs_the_lengths(n, p):
    src, smp, ls, lm, planted = rm.fixture_g(n, p)
    assert (ls, lm, planted) == (2 * n, n // 4, n // 3 + 5 * p) and not smp[lm:].any()
    # zero-padded, as a caller without lengths hands the pair over: the full-range model goes elsewhere
    fcv = fm.curve(src, smp)
    ret, lag, coef, peak = fm.model(src, smp, cv=fcv)
    at_planted = abs(float(fcv[0][planted + n - 1]))
    print("fixture g", n, p, "planted", planted, "padded: lag", lag, "|c|", peak, "|c| at the planted lag", at_planted)
    assert lag != planted and peak - at_planted >= 0.1
    # with the lengths: the planted lag, clear of every other
    cv = rm.curve(src, smp, ls, lm)
    ok = rm.competing(cv, ls, lm)
    ret, lag, coef, peak = rm.model(src, smp, ls, lm, cv=cv)
    second = rm.runner_up(cv, ok, lag)
    print("fixture g", n, p, "ragged: lag", lag, "|c|", peak, "next best", second)
    assert (ret, lag) == (0, planted) and peak - second >= MARGIN
    assert abs(coef - cv[0][lag + n - 1]) <= 1e-9


@pytest.mark.parametrize("p", [0, 1])
@pytest.mark.parametrize("n", [1000, 2049, 5000])
def test_fixture_h_a_negative_lag_and_fixture_k_two_copies(n, p):
    src, smp, ls, lm, planted = rm.fixture_h(n, p)
    assert (ls, lm, planted) == ((3 * n) // 2, (7 * n) // 10, -(n // 5)) and np.isnan(src[ls:]).all() and np.isnan(smp[lm:]).all()
    mo = n // 4
    cv = rm.curve(src, smp, ls, lm)
    ok = rm.competing(cv, ls, lm, min_overlap=mo)
    ret, lag, coef, peak = rm.model(src, smp, ls, lm, min_overlap=mo, cv=cv)
    assert (ret, lag) == (0, planted) and peak - rm.runner_up(cv, ok, lag) >= MARGIN
    ps, pt = rm.padded(src, smp, ls, lm)
    far = fm.model(ps, pt, min_overlap=mo)
    print("fixture h", n, p, "planted", planted, "ragged |c|", peak, "padded: lag", far[1], "|c|", far[3])
    assert far[1] != planted
    src, smp, ls, lm, lags = rm.fixture_k(n, p)
    cv = rm.curve(src, smp, ls, lm)
    sep = 20
    tk = rm.topk(src, smp, ls, lm, 2, sep, cv=cv)
    assert [e[:2] for e in tk] == [(0, lags[0]), (0, lags[1])], tk
    ok = rm.competing(cv, ls, lm)
    for lag in lags:
        ok[lag + n - 1 - sep:lag + n + sep] = False
    rest = float(np.max(np.where(ok, np.abs(cv[0]), -1.0)))
    print("fixture k", n, p, "entries", [e[3] for e in tk], "best outside the zones", rest)
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
    for name in ("xcorr_ncc_ragged_dev", "xcorr_ncc_ragged_topk_dev", "ncc_ragged_debug_c_dev", "xcorr_ncc_ragged_f32",
                 "xcorr_ncc_ragged_topk_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert m.ncc_ragged_args is hipxcorr.ncc_ragged_args and m.ncc_ragged_topk_args is hipxcorr.ncc_ragged_topk_args
    assert m.ragged_pack is hipxcorr.ragged_pack
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_ragged_f32_dev"][1]
    assert a[:10] == [vp, vp, sz, vp, sz, vp, sz, vp, sz, sz] and a[10:12] == [ctypes.c_double, ctypes.c_int64] and a[12:] == [vp] * 5
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_ragged_topk_f32_dev"][1]
    assert a[:10] == [vp, vp, sz, vp, sz, vp, sz, vp, sz, sz] and a[10:14] == [ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    assert a[14:] == [vp] * 5
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_ragged_debug_c_dev"][1]
    assert a[3:7] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int64] and a[7:] == [vp] * 6
    flat = re.sub(r"[\s*]+", " ", hdr)
    for phrase in ("(0, NaN, NaN, -5)", "takes precedence over -2 and -3", "m >= min(min_overlap, Ls, Lm)", "1 <= Ls <= 2N and 1 <= Lm <= N",
                   "d_lengths == NULL means (2N, N)", "a length_stride of 0 means one row for all pairs", "NaN included",
                   "n1 = min(Lm, Ls - l)", "rlo32[2N + l] for l < 0", "nothing wraps", "at most 2N - 2", "the zero half of x_lo'",
                   "Vx[l] * Vy[l] >= min_energy * Vmax * Vy", "w = min(Ls, Lm)", "template matching", "84N bytes",
                   "staged and summed per pair", "ret is never 1", "Not offered: pools", "lags >= N", "the double ABI; streams"):
        assert re.sub(r"[\s*]+", " ", phrase) in flat, phrase
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    for name in CALLS[:2]:
        assert name in top[top.index("ret = -5"):], name


def test_ragged_pack():
    asx()
    from audiosync_amd import hipxcorr
    tracks = [np.arange(1, 4), np.ones(8, np.float64), [2.5]]
    out, lens = hipxcorr.ragged_pack(tracks, 8)
    assert out.dtype == np.float32 and out.shape == (3, 8) and lens.dtype == np.int64 and lens.tolist() == [3, 8, 1]
    assert out[0].tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and out[1].tolist() == [1] * 8 and out[2].tolist() == [2.5] + [0] * 7
    for bad in ([], [np.zeros(9)], [np.zeros(0)], [np.zeros((2, 2))]):
        with pytest.raises(ValueError):
            hipxcorr.ragged_pack(bad, 8)


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_ncc_ragged_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_ncc_ragged_topk_dev(self, *a, **kw):
        raise AssertionError("called")


def test_the_checks_come_before_anything_is_uploaded():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32))
    bad = [dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
           dict(min_energy=0), dict(min_energy=1e-7), dict(min_energy=1.5), dict(min_energy=float("nan")), dict(min_energy=True),
           dict(min_overlap=0), dict(min_overlap=17), dict(min_overlap=-1), dict(min_overlap=2.0), dict(min_overlap=True),
           dict(windows=np.zeros(3, np.int64)), dict(windows=np.zeros((3, 2), np.int64)), dict(windows=np.zeros((2, 2), np.float64)),
           dict(lengths=np.zeros(3, np.int64)), dict(lengths=np.zeros((3, 2), np.int64)), dict(lengths=np.zeros((2, 2), np.float64)),
           dict(lengths=np.zeros((2, 3), np.int64)), dict(lengths=[[32.0, 16.0]] * 2)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_ragged_f32(NoDevice(), **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_ragged_args(16, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_ragged_topk_f32(NoDevice(), k=2, min_separation=1, **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_ragged_topk_args(16, k=2, min_separation=1, **args)
    for k, sep in ((0, 1), (9, 1), (2, -1), (True, 1), (2, 1.5)):
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_ragged_topk_args(16, k=k, min_separation=sep, **good)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_ragged_topk_f32(NoDevice(), k=k, min_separation=sep, **good)
    out = hipxcorr.ncc_ragged_args(16, good["source"], np.zeros(16), [[30, 3], [2, 16]], [[-15, 3], [2, 15]], np.float32(0.5), np.int64(16))
    assert out[4:] == (2, 32, 0, 1, 1, 0.5, 16) and type(out[10]) is int and out[2].dtype == np.int64 and out[3].dtype == np.int64
    # the rows' values are the device's to judge: (0, 99) passes the host checks
    assert hipxcorr.ncc_ragged_args(16, np.zeros(32), np.zeros(16), [0, 99])[4:] == (1, 0, 0, 0, 0, 1e-3, 8)
    assert hipxcorr.ncc_ragged_args(16, np.zeros(32), np.zeros(16))[2:] == (None, None, 1, 0, 0, 0, 0, 1e-3, 8)
    # a 2-D lengths array alone makes the batch: one shared pair cut three ways
    assert hipxcorr.ncc_ragged_args(16, np.zeros(32), np.zeros(16), np.ones((3, 2), np.int64))[4:9] == (3, 0, 0, 1, 0)
    assert hipxcorr.ncc_ragged_topk_args(16, good["source"], good["sample"], 8, 0, min_overlap=1)[9:] == (1e-3, 1, 8, 0)


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_the_ragged_kernels_are_built_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_nccrag_", n)}
    assert sorted(re.match(r"(?:void )?(k_nccrag_\w+)", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
