"""GCC-PHAT over track pools (asx_xcorr_pool_phat_f32_dev), the parts that need no GPU: the C-ABI and the built library export the
call, the header no longer lists pools among what PHAT does not offer, the host checks of Plan.xcorr_pool_phat_f32 raise before
anything is uploaded, the listed PHAT row kernels are built beside the k_rows_rl instances within their budgets, and the float64
model the GPU test compares against gives, over a pool of delayed copies of one track, the delays' differences."""
import ctypes
import os
import re

import numpy as np
import pytest

import phat_band_model
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

NEW = "asx_xcorr_pool_phat_f32_dev"


def test_the_call_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    assert re.search(r"\b%s\s*\(" % NEW, hdr)
    assert NEW in hipxcorr.ABI_SYMBOLS and NEW in hipxcorr.SIGNATURES
    assert hasattr(L, NEW)
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    # the per-pair result convention at the top of the header names the call at -4
    top = hdr[:hdr.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    at = top.index("ret = -4")
    assert NEW in top[at:]
    assert callable(m.Plan.xcorr_pool_phat_dev) and callable(m.Plan.xcorr_pool_phat_f32)


def test_the_header_no_longer_lists_pools_among_what_phat_lacks():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("Not offered with PHAT:")
    sentence = flat[at:flat.index(".", at)]
    assert "pool" not in sentence, sentence
    assert "top-k" in sentence and "double ABI" in sentence, sentence


def test_host_checks_return_the_checked_arguments():
    asx()
    from audiosync_amd.hipxcorr import pool_phat_args
    n = 16
    src3, smp2 = np.zeros((3, 2 * n), np.float32), np.zeros((2, n), np.float64)
    s, t, p, w, batch, ws, lo, hi = pool_phat_args(n, src3, smp2)
    assert p is None and w is None and (batch, ws, lo, hi) == (6, 0, 0, n) and s.dtype == t.dtype == np.float32
    s, t, p, w, batch, ws, lo, hi = pool_phat_args(n, src3, smp2, [[0, 1], [7, -1]], (-3, 3), (np.int64(2), 5))
    assert p.tolist() == [[0, 1], [7, -1]] and w.tolist() == [-3, 3] and (batch, ws, lo, hi) == (2, 0, 2, 5)
    assert type(lo) is int and type(hi) is int


def test_plan_method_checks_before_it_uploads():
    """Plan.xcorr_pool_phat_f32 raises ValueError before it touches the plan's device state (a stand-in plan with no handle)"""
    asx()
    from audiosync_amd import hipxcorr

    class NoDevice:
        sample_len = 16

        @property
        def device(self):
            raise AssertionError("uploaded")

        def xcorr_pool_phat_dev(self, *a, **kw):
            raise AssertionError("called")

    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((2, 16), np.float32))
    bad = [
        dict(band=(-1, 5)), dict(band=(0, 17)), dict(band=(5, 4)), dict(band=(1.0, 4)), dict(band=(True, 4)), dict(band=(1, 2, 3)),
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(windows=(1.5, 2)), dict(windows=(0, 1, 2)), dict(windows=[[0, 1]] * 3), dict(pairs=[[0, 1]] * 3, windows=[[0, 1]] * 2),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_phat_f32(NoDevice(), **args)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def _family(kernels, name):
    """template arguments -> resources of every instance of the kernel template `name`"""
    prefix = "void %s<" % name
    return {k[len(prefix):].split(">(")[0]: r for k, r in kernels.items() if k.startswith(prefix)}


@pytest.mark.parametrize("name", ["k_rows_rlp", "k_rows_rlb"])
def test_a_listed_phat_row_kernel_sits_beside_every_listed_row_kernel(kernels, name):
    """one instance per k_rows_rl instance with the same template arguments: <= 128 VGPRs, no scratch, its twin's static LDS"""
    twins, mine = _family(kernels, "k_rows_rl"), _family(kernels, name)
    assert len(twins) >= 1 and sorted(mine) == sorted(twins), (sorted(mine), sorted(twins))
    for args, r in mine.items():
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (name, args, r)
        assert r["group_segment_fixed_size"] == twins[args]["group_segment_fixed_size"], (name, args, r, twins[args])


@pytest.mark.parametrize("band", [None, (100, 2000)])
def test_the_model_over_a_pool_of_delayed_copies(band):
    """three circular delays of one noise track as both pools: every pair's lag is the difference of the delays, its peak 1, and
    the lags close every triangle.  The noise lies inside the first N frames of every clip, so that a clip's first N frames, which
    are the sample, are the whole clip once the transform pads them: each pair is a pure circular delay.  (Only the model runs: this
    pins what the GPU test compares against.)"""
    n = 6000
    lo, hi = (0, n) if band is None else band
    base = np.zeros(2 * n)
    base[1500:1500 + 3000] = np.random.default_rng(11).standard_normal(3000)
    delays = [0, 37, -1213]
    clips = [np.roll(base, d) for d in delays]
    assert all(not c[n:].any() for c in clips)
    lag = np.zeros((3, 3), dtype=np.int64)
    for a in range(3):
        for b in range(3):
            # r[k] = sum over m of source[m + k] sample[m] peaks at k = (delay of a) - (delay of b)
            ret, lag[a, b], coef, peak = phat_band_model.model(clips[a], clips[b][:n], lo, hi)
            assert lag[a, b] == delays[a] - delays[b], (a, b, lag[a, b])
            assert abs(peak - 1.0) <= 1e-12, (a, b, peak)
            assert ret == 0
    for a in range(3):
        for b in range(3):
            for c in range(3):
                assert lag[a, b] + lag[b, c] == lag[a, c], (a, b, c)
