"""Pool calls (asx_xcorr_pool_f32_dev), the parts that need no GPU: the C-ABI and the host library export the new call, ret = -4 is
documented, the host checks of Plan.xcorr_pool_f32 raise before anything is uploaded, and the listed kernels are built beside the
instances they mirror within their budgets."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft, kernel_forms


def test_new_symbol_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    assert re.search(r"\basx_xcorr_pool_f32_dev\s*\(", hdr)
    assert "asx_xcorr_pool_f32_dev" in hipxcorr.ABI_SYMBOLS
    assert hasattr(L, "asx_xcorr_pool_f32_dev")
    assert m.lib().asx_abi_version() == 2
    # ret = -4 is documented beside the per-pair result convention at the top of the header
    top = hdr[:hdr.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    assert "ret = -4" in top and "asx_xcorr_pool_f32_dev" in top


def test_pool_host_checks_raise_before_any_device_call():
    from audiosync_amd.hipxcorr import pool_args
    asx()
    n = 16
    src3, smp2 = np.zeros((3, 2 * n), np.float32), np.zeros((2, n), np.float64)
    s, t, p, w, batch, ws = pool_args(n, src3, smp2)
    assert p is None and w is None and (batch, ws) == (6, 0) and s.dtype == t.dtype == np.float32
    s, t, p, w, batch, ws = pool_args(n, src3, smp2, [[0, 1], [2, 0], [7, -1]], [[-1, 1]] * 3)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1], [2, 0], [7, -1]] and w.dtype == np.int64 and (batch, ws) == (3, 1)
    s, t, p, w, batch, ws = pool_args(n, src3, smp2, np.array([[2 ** 31 - 1, -2 ** 31]]), (0, 3))
    assert (batch, ws) == (1, 0) and p.tolist() == [[2 ** 31 - 1, -2 ** 31]]      # indices are not checked: -4 stays reachable
    bad = [
        dict(sources=np.zeros(2 * n, np.float32)), dict(samples=np.zeros(n, np.float32)),
        dict(sources=np.zeros((3, 2 * n + 1), np.float32)), dict(samples=np.zeros((2, n - 1), np.float32)),
        dict(sources=np.zeros((0, 2 * n), np.float32)), dict(samples=np.zeros((0, n), np.float32)),
        dict(pairs=[[0.0, 1.0]]), dict(pairs=[0, 1]), dict(pairs=[[0, 1, 2]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(pairs=[[2 ** 31, 0]]), dict(pairs=[[0, -2 ** 31 - 1]]),
        dict(windows=(0.5, 1.0)), dict(windows=(0, 1, 2)), dict(windows=[[0, 1]] * 2),
        dict(pairs=[[0, 1]] * 3, windows=[[0, 1]] * 2),
    ]
    for kw in bad:
        args = dict(sources=src3, samples=smp2, pairs=None, windows=None)
        args.update(kw)
        with pytest.raises(ValueError):
            pool_args(n, args["sources"], args["samples"], args["pairs"], args["windows"])


def test_plan_method_checks_before_it_uploads():
    """Plan.xcorr_pool_f32 raises from pool_args before it touches the plan's device state (a stand-in plan with no handle)"""
    m = asx()
    from audiosync_amd import hipxcorr

    class NoDevice:
        sample_len = 16

        @property
        def device(self):
            raise AssertionError("uploaded")

        def xcorr_pool_dev(self, *a, **kw):
            raise AssertionError("called")

    for kw in (dict(pairs=[[0, 1, 2]]), dict(windows=(1.5, 2)), dict(pairs=[[0.0, 0.0]])):
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_f32(NoDevice(), np.zeros((2, 32), np.float32), np.zeros((2, 16), np.float32), **kw)
    with pytest.raises(ValueError):
        hipxcorr.Plan.xcorr_pool_f32(NoDevice(), np.zeros((2, 32), np.float32), np.zeros((2, 15), np.float32))
    assert m is not None


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def _args(k, prefix):
    return k[len(prefix):].split(">(")[0]


def test_listed_row_kernel_sits_beside_every_row_kernel(kernels):
    """k_rows_rl<S, NT, TWO> beside k_rows_r<S, NT, TWO, BC>: the same LDS, <= 128 VGPRs, no scratch"""
    base = {}
    for k, r in kernels.items():
        if k.startswith("void k_rows_r<"):
            base.setdefault(_args(k, "void k_rows_r<").rsplit(", ", 1)[0], []).append(r)
    mine = {_args(k, "void k_rows_rl<"): r for k, r in kernels.items() if k.startswith("void k_rows_rl<")}
    assert base and set(base) == set(mine), (sorted(base), sorted(mine))
    for args, r in mine.items():
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (args, r)
        assert {b["group_segment_fixed_size"] for b in base[args]} == {r["group_segment_fixed_size"]}, (args, r)


def test_listed_tail_kernels_meet_the_budgets(kernels):
    """the listed forms of the tail kernels that read inputs, beside the forms they mirror, with the same LDS"""
    found = {}
    for k, r in kernels.items():
        m = re.match(r"(?:void )?(k_pool_resolve|k_invalid_pairs)\b", k)
        if m:
            found.setdefault(m.group(1), []).append((k, r))
    listed = {name: kernel_forms(kernels, family, selection, "listed")
              for name, family, selection in (("k_refine_dots listed", "k_refine_dots", None), ("k_pearson_partial listed", "k_pearson_partial", None),
                                              ("k_pearson_prep seed listed", "k_pearson_prep", "seed"), ("k_pearson_prep rows listed", "k_pearson_prep", "rows"))}
    listed_dots = listed["k_refine_dots listed"]
    for name, forms in listed.items():
        found[name] = [(name + " " + k, r) for k, rs in forms.items() for _, r in rs]
    assert {k: len(v) for k, v in found.items()} == {"k_pool_resolve": 1, "k_invalid_pairs": 1, "k_refine_dots listed": 1,
                                                     "k_pearson_partial listed": 2, "k_pearson_prep seed listed": 2, "k_pearson_prep rows listed": 2}, found
    for name, ks in found.items():
        for k, r in ks:
            assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (k, r)

    def lds_of(forms):
        return {k: [r["group_segment_fixed_size"] for _, r in rs] for k, rs in forms.items()}

    prep = lds_of(kernel_forms(kernels, "k_pearson_prep", "seed", "pitched"))
    for name in ("k_pearson_prep seed listed", "k_pearson_prep rows listed"):
        assert lds_of(listed[name]) == prep, (name, lds_of(listed[name]), prep)
    dots = [r["group_segment_fixed_size"] for _, r in kernel_forms(kernels, "k_refine_dots", inputs="pitched")["float"]]
    assert dots and [r["group_segment_fixed_size"] for _, r in listed_dots["float"]] == dots
