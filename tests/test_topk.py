"""Top-k peaks (asx_xcorr_topk_f32_dev), the parts that need no GPU: the C-ABI and the host library export the new call, the float64
model of the rule (tests/topk_model.py) agrees with a plain loop, the host checks of Plan.xcorr_topk_f32 raise before anything is
uploaded, and the new kernels are built beside the windowed ones within their budgets."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from test_kernel_resources import READELF, demangled, kernels_of
from topk_model import allowed, brute_peaks, topk_peaks
from util import ROOT, asx, graft, kernel_forms


def test_new_symbol_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    assert re.search(r"\basx_xcorr_topk_f32_dev\s*\(", hdr)
    assert "asx_xcorr_topk_f32_dev" in hipxcorr.ABI_SYMBOLS
    assert hasattr(L, "asx_xcorr_topk_f32_dev")
    assert m.lib().asx_abi_version() == 2
    assert re.search(r"#define ASX_TOPK_MAX 8\b", hdr) and hipxcorr.TOPK_MAX == 8
    # ret = -3 is documented beside the per-pair result convention at the top of the header
    top = hdr[:hdr.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    assert "ret = -3" in top and "asx_xcorr_topk_f32_dev" in top


def test_model_is_a_greedy_search_over_the_allowed_lags():
    """topk_peaks (numpy, built on oracle.max_abs_index) against a plain loop over every lag, on small r with many exact ties"""
    rng = np.random.default_rng(7)
    seen = {"empty": 0, "seed_moved": 0, "straddle0": 0, "ties": 0}
    for trial in range(300):
        n = int(rng.integers(3, 24))
        r = rng.integers(-4, 5, 2 * n).astype(np.float64)          # few values: exact ties everywhere
        if trial % 5 == 0:
            r = rng.standard_normal(2 * n)
        lo = int(rng.integers(-n, n))
        hi = int(rng.integers(lo, n))
        if trial % 7 == 0:
            lo, hi = -n, n - 1
        k = int(rng.integers(1, 9))
        sep = int(rng.choice([0, 1, 2, 3, n // 2, n, 2 * n, 10 ** 9]))
        got = topk_peaks(r, n, k, sep, lo, hi)
        want = brute_peaks(r, n, k, sep, lo, hi)
        assert got == want, (n, lo, hi, k, sep, r.tolist(), got, want)
        seen["empty"] += None in got
        lags = [p if p < n else p - 2 * n for p in got if p is not None]
        seen["straddle0"] += any(l - sep < 0 <= l + sep for l in lags[:-1])
        seen["ties"] += len(set(np.abs(r).tolist())) < 2 * n
        first = allowed(n, lo, hi, [], sep)[0]
        if len(lags) >= 2 and allowed(n, lo, hi, lags[:1], sep).size and allowed(n, lo, hi, lags[:1], sep)[0] != first:
            seen["seed_moved"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_model_rules_by_hand():
    n = 8
    r = np.zeros(2 * n)
    # ties: the smallest index wins, and the zone of the winner takes its neighbours out
    r[[2, 5, 9]] = [3.0, -3.0, 3.0]                               # lags 2, 5, -7
    assert topk_peaks(r, n, 4, 0) == [2, 5, 9, 0]
    assert topk_peaks(r, n, 3, 3) == [2, 9, 6]                    # |5 - 2| <= 3: lag 5 is out; then lag -7; the seed of what is left
    # the seed competes signed: a negative value at the seed loses to a zero elsewhere
    r = np.zeros(2 * n)
    r[0] = 5.0
    r[1] = -1.0
    assert topk_peaks(r, n, 2, 0) == [0, 2]                       # seed of A_2 is index 1 (lag 1): -1 signed, the |0| at index 2 beats it
    r[1] = 1.0
    assert topk_peaks(r, n, 2, 0) == [0, 1]                       # +1 at the seed: nothing beats it
    # linear lag distance: lags -N and N-1 are far apart; exhaustion gives None for this entry and every later one
    r = np.zeros(2 * n)
    r[n - 1] = 2.0                                                # lag N-1
    assert topk_peaks(r, n, 2, 1, -n, n - 1)[1] == 0
    assert topk_peaks(r, n, 3, 2 * n) == [n - 1, None, None]
    assert topk_peaks(r, n, 3, 0, n - 2, n - 1) == [n - 1, n - 2, None]


def test_topk_host_checks_raise_before_any_device_call():
    from audiosync_amd.hipxcorr import topk_args
    asx()
    n = 16
    src1, smp1 = np.zeros(2 * n, np.float32), np.zeros(n, np.float32)
    src3, smp3 = np.zeros((3, 2 * n), np.float32), np.zeros((3, n), np.float32)
    s, t, w, batch, ss, ts, ws, k, sep = topk_args(n, src3, smp1, 4, 100)
    assert w is None and (batch, ss, ts, ws, k, sep) == (3, 2 * n, 0, 0, 4, 100)
    s, t, w, batch, ss, ts, ws, k, sep = topk_args(n, src1, smp3, 1, 0, [[-1, 1]] * 3)
    assert w.dtype == np.int64 and (batch, ss, ts, ws, k, sep) == (3, 0, n, 1, 1, 0)
    assert topk_args(n, src1, smp1, np.int32(8), np.int64(0), (0, 3))[3:] == (1, 0, 0, 0, 8, 0)
    bad = [
        dict(k=0, min_separation=0), dict(k=9, min_separation=0), dict(k=2.0, min_separation=0), dict(k=True, min_separation=0),
        dict(k=2, min_separation=-1), dict(k=2, min_separation=1.5), dict(k=2, min_separation=None),
        dict(k=2, min_separation=0, windows=(0, 1, 2)), dict(k=2, min_separation=0, windows=(0.5, 1.0)),
        dict(k=2, min_separation=0, windows=[[0, 1]] * 2),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            topk_args(n, src3, smp3, **kw)
    for s_, t_ in ((np.zeros(2 * n + 1, np.float32), smp1), (src1, np.zeros(n - 1, np.float32)), (src3, np.zeros((2, n), np.float32))):
        with pytest.raises(ValueError):
            topk_args(n, s_, t_, 2, 0)


def test_plan_method_checks_before_it_uploads():
    """Plan.xcorr_topk_f32 raises from topk_args before it touches the plan's device state (a stand-in plan with no handle)"""
    m = asx()
    from audiosync_amd import hipxcorr

    class NoDevice:
        sample_len = 16

        def _staged(self, *a, **kw):
            raise AssertionError("uploaded")

    for k, sep in ((0, 0), (9, 0), (2, -1)):
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_topk_f32(NoDevice(), np.zeros(32, np.float32), np.zeros(16, np.float32), k, sep)
    assert m is not None


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def test_topk_inverse_kernels_sit_beside_the_per_pair_ones(kernels):
    """the top-k form beside every per-pair form, same template arguments: k_inv_cols_r<..., AsxSelTopk<ZC>> in three zone
    capacities beside <..., AsxWinRows>, k_inv_cols<..., AsxSelTopk<7>> (the packed kernels' one capacity) beside every
    k_inv_cols<..., AsxWinRows>: same LDS, <= 128 VGPRs, no scratch"""
    n = 0
    for family, caps in (("k_inv_cols_r", ["1", "3", "7"]), ("k_inv_cols", ["7"])):
        base = kernel_forms(kernels, family, "rows")
        mine = kernel_forms(kernels, family, "topk")
        assert base and set(base) == set(mine), (family, sorted(base), sorted(mine))
        for args, rs in mine.items():
            assert sorted(str(zc) for zc, _ in rs) == [str(c) for c in caps], (family, args)
            ((_, b),) = base[args]
            for _, r in rs:
                assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (family, args, r)
                assert r["group_segment_fixed_size"] == b["group_segment_fixed_size"], (family, args, r)
                n += 1
    assert n == 3 * 3 + 8, n


def test_topk_tail_kernels_meet_the_budgets(kernels):
    found = {f: [(f + " " + k, r) for k, rs in kernel_forms(kernels, f, "topk").items() for _, r in rs]
             for f in ("k_finalize", "k_refine_pick", "k_pearson_prep")}
    found["k_topk_step"] = [(k, r) for k, r in kernels.items() if k.startswith("k_topk_step(")]
    assert {k: len(v) for k, v in found.items()} == {"k_finalize": 1, "k_refine_pick": 1, "k_pearson_prep": 2,
                                                     "k_topk_step": 1}, found
    for k, r in itertools.chain.from_iterable(found.values()):
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (k, r)
