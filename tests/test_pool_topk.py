"""Top-k over pools (asx_xcorr_pool_topk_f32_dev) and the best-entry consumer (asx_topk_best_dev), the parts that need no GPU: the
C-ABI and the host library export both calls, the header names the new call at ret = -3 and -4 and no longer says that top-k over
pools is not offered, the host checks of Plan.xcorr_pool_topk_f32 raise before anything is uploaded, and the new kernels are built
beside the instances they mirror within their budgets."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

NEW = ("asx_xcorr_pool_topk_f32_dev", "asx_topk_best_dev")


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert m.lib().asx_abi_version() == 2
    # the per-pair result convention at the top of the header names the new call at -3 and at -4
    top = hdr[:hdr.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    for code in ("ret = -3", "ret = -4"):
        at = top.index(code)
        nxt = top.find("ret = -", at + 1)
        assert "asx_xcorr_pool_topk_f32_dev" in top[at:nxt if nxt > 0 else len(top)], code
    for path in (os.path.join("include", "audiosync", "xcorr_hip.h"), "INTEGRATION.md"):
        assert "Top-k over pools is not offered" not in open(os.path.join(ROOT, path)).read(), path
    assert callable(m.topk_best_dev) and hasattr(m.Plan, "xcorr_pool_topk_dev") and hasattr(m.Plan, "xcorr_pool_topk_f32")


def test_host_checks_return_the_checked_arguments():
    asx()
    from audiosync_amd.hipxcorr import TOPK_MAX, pool_topk_args
    n = 16
    src3, smp2 = np.zeros((3, 2 * n), np.float32), np.zeros((2, n), np.float64)
    s, t, p, w, batch, ws, k, sep = pool_topk_args(n, src3, smp2, np.int64(TOPK_MAX), 0)
    assert p is None and w is None and (batch, ws, k, sep) == (6, 0, TOPK_MAX, 0) and s.dtype == t.dtype == np.float32
    assert type(k) is int and type(sep) is int
    s, t, p, w, batch, ws, k, sep = pool_topk_args(n, src3, smp2, 2, 5, [[0, 1], [7, -1]], (-3, 3))
    assert p.tolist() == [[0, 1], [7, -1]] and w.tolist() == [-3, 3] and (batch, ws, k, sep) == (2, 0, 2, 5)


def test_plan_method_checks_before_it_uploads():
    """Plan.xcorr_pool_topk_f32 raises ValueError before it touches the plan's device state (a stand-in plan with no handle)"""
    asx()
    from audiosync_amd import hipxcorr

    class NoDevice:
        sample_len = 16

        @property
        def device(self):
            raise AssertionError("uploaded")

        def xcorr_pool_topk_dev(self, *a, **kw):
            raise AssertionError("called")

        def xcorr_pool_dev(self, *a, **kw):
            raise AssertionError("called")

    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((2, 16), np.float32), k=2, min_separation=10)
    bad = [
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(windows=(1.5, 2)), dict(windows=(0, 1, 2)), dict(windows=[[0, 1]] * 3), dict(pairs=[[0, 1]] * 3, windows=[[0, 1]] * 2),
        dict(k=0), dict(k=9), dict(k=2.0), dict(k=True), dict(min_separation=-1), dict(min_separation=1.0),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_topk_f32(NoDevice(), **args)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def _args(k, prefix):
    return k[len(prefix):].split(">(")[0]


def test_listed_topk_prep_kernel_sits_beside_every_prep_kernel(kernels):
    """k_pearson_prep_xl<NTP, NB>: exactly the instances and the LDS of k_pearson_prep<NTP, NB>, <= 128 VGPRs, no scratch"""
    lds = {k: r["group_segment_fixed_size"] for k, r in kernels.items()}
    prep = {_args(k, "void k_pearson_prep<"): v for k, v in lds.items() if k.startswith("void k_pearson_prep<")}
    mine = {_args(k, "void k_pearson_prep_xl<"): v for k, v in lds.items() if k.startswith("void k_pearson_prep_xl<")}
    assert len(prep) == 2 and mine == prep, (mine, prep)
    for k, r in kernels.items():
        if k.startswith("void k_pearson_prep_xl<"):
            assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (k, r)


def test_the_other_new_kernels_meet_the_budgets(kernels):
    """the k-entry writer for pairs outside their pools and the best-entry consumer: one instance each, plain kernels without LDS"""
    found = {}
    for k, r in kernels.items():
        m = re.match(r"(?:void )?(k_invalid_pairs_k|k_topk_best)\b", k)
        if m:
            found.setdefault(m.group(1), []).append((k, r))
    assert {k: len(v) for k, v in found.items()} == {"k_invalid_pairs_k": 1, "k_topk_best": 1}, found
    for ks in found.values():
        for k, r in ks:
            assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
