"""Per-pair lag windows (asx_xcorr_windowed_f32_dev), the parts that need no GPU: the C-ABI and the host library export the new
call, the per-pair kernels are built beside the windowed ones and keep their budgets, the positions -> rows arithmetic of
Plan.xcorr_windows_f32 agrees with a loop, and the host checks of Plan.xcorr_windowed_f32 raise before anything is uploaded."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft, kernel_forms

NEW_ABI = ("asx_xcorr_windowed_f32_dev",)


def test_new_symbol_is_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in NEW_ABI:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert m.lib().asx_abi_version() == 2
    # ret = -2 is documented beside the per-pair result convention at the top of the header
    top = hdr[:hdr.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    assert "ret[i] = -2" in top and "asx_xcorr_windowed_f32_dev" in top


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    return {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}


def test_per_pair_inverse_kernels_sit_beside_the_windowed_ones(kernels):
    """the per-pair form beside every window form of k_inv_cols_r (<..., AsxWinRows> beside <..., AsxWin>) and of k_inv_cols
    (the same two selections), same template arguments: same LDS, <= 128 VGPRs, no scratch"""
    pairs = 0
    for family in ("k_inv_cols_r", "k_inv_cols"):
        base = kernel_forms(kernels, family, "window")
        mine = kernel_forms(kernels, family, "rows")
        assert base and set(base) == set(mine), (family, sorted(base), sorted(mine))
        for k, rs in mine.items():
            ((_, r),), ((_, b),) = rs, base[k]
            assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (family, k, r)
            assert r["group_segment_fixed_size"] == b["group_segment_fixed_size"], (family, k, r, b)
            pairs += 1
    assert pairs == 3 + 8, pairs


def test_per_pair_tail_kernels_meet_the_budgets(kernels):
    found = {f: [(f + " " + k, r) for k, rs in kernel_forms(kernels, f, "rows").items() for _, r in rs]
             for f in ("k_finalize", "k_refine_pick", "k_pearson_prep")}
    found["k_invalid_rows"] = [(n, r) for n, r in kernels.items() if n.startswith("k_invalid_rows(")]
    assert {k: len(v) for k, v in found.items()} == {"k_finalize": 1, "k_refine_pick": 1, "k_pearson_prep": 2,
                                                     "k_invalid_rows": 1}, found
    for n, r in sum(found.values(), []):
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)


def brute_rows(n, hop, batch, p_lo, p_hi):
    out = []
    for k in range(batch):
        lo, hi = max(p_lo - k * hop, -n), min(p_hi - k * hop, n - 1)
        if lo <= hi:
            out.append((k, lo, hi))
    return out


def test_position_rows_agree_with_a_loop():
    from audiosync_amd.hipxcorr import position_rows
    asx()
    cases = itertools.product((5, 8, 100, 144000), (1, 3, 4, 7, 64, 250, 36000), (1, 4, 13),
                              (-10 ** 6, -400, -7, 0, 3, 55, 300, 1000, 500000), (0, 2, 9, 60, 310, 2000, 10 ** 6))
    seen_empty = seen_partial = 0
    for n, hop, batch, p_lo, p_hi in cases:
        if p_lo > p_hi:
            continue
        k0, k1, rows = position_rows(n, hop, batch, p_lo, p_hi)
        want = brute_rows(n, hop, batch, p_lo, p_hi)
        got = [(k0 + i, int(lo), int(hi)) for i, (lo, hi) in enumerate(rows)]
        assert got == want, (n, hop, batch, p_lo, p_hi)
        assert rows.dtype == np.int64 and rows.shape == (k1 - k0, 2)
        assert all(-n <= lo <= hi <= n - 1 for _, lo, hi in got)
        seen_empty += k0 == k1
        seen_partial += 0 < k1 - k0 < batch
    assert seen_empty and seen_partial
    # ranges that start before the recording, hops that do not divide the range, ranges beyond the last window
    assert position_rows(100, 30, 10, -250, -201)[:2] == (0, 0)
    k0, k1, rows = position_rows(100, 30, 10, -60, 45)
    assert (k0, k1) == (0, 5) and rows[0].tolist() == [-60, 45] and rows[-1].tolist() == [-100, -75]
    assert position_rows(100, 30, 10, 10 ** 6, 10 ** 6 + 5)[:2] == (0, 0)
    with pytest.raises(ValueError):
        position_rows(100, 30, 10, 5, 4)
    with pytest.raises(ValueError):
        position_rows(100, 0, 10, 0, 4)


def test_windowed_host_checks_raise_before_any_device_call():
    from audiosync_amd.hipxcorr import windowed_args
    asx()
    n = 16
    src1, smp1 = np.zeros(2 * n, np.float32), np.zeros(n, np.float32)
    src3, smp3 = np.zeros((3, 2 * n), np.float32), np.zeros((3, n), np.float32)
    s, t, w, batch, ss, ts, ws = windowed_args(n, src3, smp1, [[-1, 1]] * 3)
    assert (batch, ss, ts, ws) == (3, 2 * n, 0, 1) and w.dtype == np.int64
    assert windowed_args(n, src1, smp3, (-n, n - 1))[3:] == (3, 0, n, 0)
    assert windowed_args(n, src1, smp1, np.array([0, 0], np.int32))[3:] == (1, 0, 0, 0)
    # a row that is not a window is the caller's to send: it comes back as (0, NaN, -2), it is not refused here
    assert windowed_args(n, src1, smp1, (5, 4))[3] == 1
    bad = [
        (np.zeros(2 * n + 1, np.float32), smp1, (0, 1)),     # source length
        (src1, np.zeros(n - 1, np.float32), (0, 1)),         # sample length
        (src1, smp1, (0, 1, 2)),                             # a row of three
        (src1, smp1, np.zeros((2, 2, 2), np.int64)),         # windows of rank 3
        (src1, smp1, (0.5, 1.0)),                            # not integers
        (src3, smp3, [[0, 1]] * 2),                          # batch sizes differ
        (src3, np.zeros((2, n), np.float32), (0, 1)),
        (np.zeros((0, 2 * n), np.float32), smp1, (0, 1)),    # empty batch
        (np.zeros((1, 1, 2 * n), np.float32), smp1, (0, 1)),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            windowed_args(n, *args)
