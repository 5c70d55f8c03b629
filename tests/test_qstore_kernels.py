"""The kernels of partial storing (csrc/rlayout.hip: k_rows_rm, k_q_predict, k_qstore_takeback), read from the built library without a
GPU: the budgets of the row kernels beside k_rows_rm (tests/test_prune_kernels.py) -- at most 128 VGPRs, no scratch, and static plus
dynamic LDS that lets four 256-thread blocks of the two-half form share a compute unit."""
import os
import re

import pytest

import test_kernel_resources as res
from util import asx, graft


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(res.READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    found = res.kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    return {res.demangled(k): v for k, v in found.items()}


def test_the_partial_store_row_kernel_keeps_the_row_budgets(kernels):
    rows = [(n, r) for n, r in kernels.items() if n.startswith("void k_rows_rm<")]
    assert len(rows) == 1, sorted(n for n, _ in rows)  # the two-half form (N = 960 000 and 1 440 000)
    (n, r), = rows
    assert re.match(r"void k_rows_rm<Sched<1200, [^>]*>, 128, true>", n), n
    assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    assert 4 * (2400 * 16 + r["group_segment_fixed_size"]) <= 160 * 1024, (n, r)


def test_the_small_kernels_are_there_and_spill_nothing(kernels):
    for name in ("k_q_predict", "k_qstore_takeback"):
        (n, r), = [(n, r) for n, r in kernels.items() if n.startswith(name + "(")]
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)


def test_the_row_kernels_beside_it_are_still_there(kernels):
    assert len([n for n in kernels if n.startswith("void k_rows_r<")]) == 12
    assert len([n for n in kernels if n.startswith("void k_rows_re<")]) == 3
