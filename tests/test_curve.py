"""The curve around given lags (asx_xcorr_curve_f32_dev, asx_xcorr_pool_curve_f32_dev), the parts that need no GPU: the float64 model of
tests/curve_model.py is the oracle's r at every index and takes its neighbours circularly, the header says what the calls promise, the
C-ABI and the built library export both calls, the host checks of the Plan methods raise before anything is uploaded, and the built
code object holds two k_curve_dots within their budget while the pinned families keep their counts."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import curve_model
import oracle
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft, kernel_forms

CALLS = ("asx_xcorr_curve_f32_dev", "asx_xcorr_pool_curve_f32_dev")


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 1000])
def test_the_models_r_is_the_oracles_at_every_index(n):
    """the time-domain sum against the oracle's float64 transforms, whose inverse is unnormalised as the reference's is (2N times the
    plain sum): within the transforms' own error, 1e-10 of |source| |sample|"""
    src, smp, _ = oracle.synth_pair(11, 2, n, 1)
    want = np.asarray(oracle.cross_correlation(src, smp, want_results=True)[3], dtype=np.float64) / (2 * n)
    assert want.size == 2 * n
    got = np.array([curve_model.r_at(src, smp, i)[0] for i in range(2 * n)])
    scale = float(np.linalg.norm(src.astype(np.float64)) * np.linalg.norm(smp.astype(np.float64)))
    err = float(np.max(np.abs(got - want))) / scale
    print("curve model N", n, "worst |model - oracle| / (|source| |sample|)", err)
    assert err < 1e-10


def test_neighbours_are_circular_in_index_space():
    n = 16
    assert curve_model.neighbours(0, n, 2) == [30, 31, 0, 1, 2]              # index 2N - 1 (lag -1) sits beside index 0
    assert curve_model.neighbours(-1, n, 1) == [30, 31, 0]
    assert curve_model.neighbours(n - 1, n, 1) == [14, 15, 16]               # index N (lag -N) beside index N - 1
    assert curve_model.neighbours(-n, n, 1) == [15, 16, 17]
    assert [curve_model.lag_of(i, n) for i in (30, 31, 0, 15, 16, 17)] == [-2, -1, 0, 15, -16, -15]
    src, smp, _ = oracle.synth_pair(5, 0, n, 1)
    for lag in (0, -1, n - 1, -n):
        r, tol, coef, frac = curve_model.curve(src, smp, lag, 1)
        idx = curve_model.neighbours(lag, n, 1)
        assert r.tolist() == [curve_model.r_at(src, smp, i)[0] for i in idx]
        assert all(t > 0.0 for t in tol)
        for i, c in zip(idx, coef):
            assert math.isnan(c) == (i in (n, n + 1)), (lag, i, c)           # lag -N: empty; lag -N + 1: one frame, constant
        assert frac == curve_model.phat_sub_model.frac_of(*r)
    with pytest.raises(AssertionError):
        curve_model.index_of(n, n)


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
    assert re.search(r"^#define\s+ASX_NEAR_MAX\s+8\s*$", hdr, flags=re.M)
    assert hipxcorr.NEAR_MAX == 8 == curve_model.NEAR_MAX
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_curve_dev", "xcorr_pool_curve_dev", "xcorr_curve_f32", "xcorr_pool_curve_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert callable(hipxcorr.curve_args) and callable(hipxcorr.pool_curve_args)
    # (batch, entries, d_center, half_width) then four float64 / int32 outputs and the stream, in both
    for name in CALLS:
        a = hipxcorr.SIGNATURES[name][1]
        assert a[-9:-5] == [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] and a[-5:] == [ctypes.c_void_p] * 5, name


def test_the_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("The exact correlation curve and a fractional lag around given lags")
    text = flat[at:flat.index("int asx_xcorr_pool_curve_f32_dev", at)]
    for phrase in ("r[idx] = sum_{n<N} source[(n + idx) mod 2N] * sample[n]", "packed ones included", "a stride of 0 broadcasts",
                   "1 <= entries <= ASX_TOPK_MAX", "1 <= half_width <= ASX_NEAR_MAX", "e = i * entries + j",
                   "d_r[e * n + (d + h)] = r[(p + d) mod 2N]", "index 2N - 1 (lag -1) sits beside index 0",
                   "index N (lag -N) beside index N - 1", "unnormalised and signed", "always in the direct form", "bit for bit",
                   "row [l, l]", "d_coef may be NULL", "den = (a - 2 b) + c", "clamped to [-0.5, 0.5]", "-2 for a centre outside [-N, N-1]",
                   "-4 for an entry", "over -2", "allocates nothing", "never synchronises the host", "touches no counter",
                   "one direct Pearson pass per neighbour", "never touches, fills or grows the bank", "batch == 0 returns 0",
                   "independent of the batch size"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    top =flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    minus2 = top[top.index("ret[i] = -2"):top.index("ret = -3")]
    minus4 = top[top.index("ret = -4"):]
    for name in CALLS:
        assert name in minus2 and (name in minus4) == name.startswith("asx_xcorr_pool"), name
    sentence = flat[flat.index("Not offered with PHAT:"):]
    sentence = sentence[:sentence.index(".")]
    assert "top-k" in sentence and "double ABI" in sentence, sentence


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_curve_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_pool_curve_dev(self, *a, **kw):
        raise AssertionError("called")


BAD_OPTIONS = [dict(half_width=0), dict(half_width=9), dict(half_width=1.5), dict(half_width=True), dict(half_width=-1),
               dict(half_width=None), dict(entries=0), dict(entries=9), dict(entries=2.0), dict(entries=True), dict(entries=None)]


def test_the_strided_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32), centers=np.zeros(2, np.int64))
    bad = BAD_OPTIONS + [
        dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
        dict(centers=np.zeros(3, np.int64)), dict(centers=np.zeros((2, 2), np.int64)), dict(centers=np.zeros(2, np.float64)),
        dict(centers=np.zeros((2, 3), np.int64), entries=2), dict(centers=np.zeros(2, np.int64), entries=2),
        dict(centers=np.zeros((2, 1, 1), np.int64)), dict(centers=[True, False]), dict(centers=np.int64(0)),
        dict(source=np.zeros(32, np.float32), sample=np.zeros(16, np.float32), centers=np.zeros(0, np.int64)),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_curve_f32(NoDevice(), **args)
    s, t, c, batch, ss, ts, h, entries = hipxcorr.curve_args(16, good["source"], np.zeros(16), [[3, -4, 5], [0, 1, -16]], np.int32(8), np.int64(3))
    assert (batch, ss, ts, h, entries) == (2, 32, 0, 8, 3) and c.dtype == np.int64 and c.shape == (2, 3) and t.dtype == np.float32
    assert type(h) is int and type(entries) is int
    # both operands 1-D: the centres set the batch; [B] and [B, 1] are both one entry per pair
    assert hipxcorr.curve_args(16, np.zeros(32), np.zeros(16), [1, 2, 3])[3:] == (3, 0, 0, 1, 1)
    assert hipxcorr.curve_args(16, np.zeros(32), np.zeros(16), [[1], [2]])[2].shape == (2, 1)


def test_the_pool_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((3, 16), np.float32), centers=np.zeros((2, 3), np.int64))
    bad = BAD_OPTIONS + [
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(centers=np.zeros(6, np.int64)), dict(centers=np.zeros((3, 2), np.int64)), dict(centers=np.zeros((2, 3), np.float32)),
        dict(pairs=[[0, 1]] * 4, centers=np.zeros((2, 3), np.int64)), dict(centers=np.zeros((2, 3, 2), np.int64)),
        dict(centers=np.zeros((2, 3), np.int64), entries=2),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_curve_f32(NoDevice(), **args)
    out = hipxcorr.pool_curve_args(16, good["sources"], good["samples"], [[5, 6], [7, 8]], [[0, 1], [7, -1]], 3, 2)
    assert out[4:] == (2, 3, 2) and out[2].tolist() == [[0, 1], [7, -1]] and out[3].tolist() == [[5, 6], [7, 8]]
    assert hipxcorr.pool_curve_args(16, good["sources"], good["samples"], np.zeros((2, 3, 4), np.int32), entries=4)[4:] == (6, 1, 4)
    assert hipxcorr.pool_curve_args(16, good["sources"], good["samples"], good["centers"])[2] is None


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_two_curve_kernels_within_their_budget_and_the_pinned_families_unchanged():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = sorted((n, r) for n, r in names.items() if re.match(r"(void )?k_curve_dots\b", n))
    assert len(mine) == 2 and "AsxAtList" in mine[0][0] and "AsxAtPitch" in mine[1][0], [n for n, _ in mine]
    for n, r in mine:
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    prep = [n for n in names if re.match(r"(void )?k_pearson_prep\b", n)]
    aux = [n for n in names if re.match(r"(void )?k_bcast_aux\b", n)]
    dots = [r for rs in kernel_forms(names, "k_refine_dots", inputs="pitched").values() for r in rs]
    listed = [r for rs in kernel_forms(names, "k_refine_dots", inputs="listed").values() for r in rs]
    assert (len(prep), len(dots), len(listed), len(aux)) == (2, 2, 1, 1), (prep, aux)
    assert len([n for n in names if re.match(r"(void )?k_phat_near\b", n)]) == 1
