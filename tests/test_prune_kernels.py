"""The kernels of the pruned inverse column pass (csrc/rlayout.hip), read from the built library without a GPU: the budgets of the
kernels beside them (tests/test_kernel_resources.py) and, for the two-half row form, the load order tests/test_kernel_isa_order.py
pins for k_rows_r -- the tile energies are summed through LDS and stored, nothing is loaded for them."""
import os
import re

import pytest

import test_kernel_isa_order as order
import test_kernel_resources as res
from util import asx, graft, kernel_forms


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(res.READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    found = res.kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    return {res.demangled(k): v for k, v in found.items()}


def test_row_kernels_with_tile_energies_keep_the_row_budgets(kernels):
    """three instances (480-point rows, 1200-point rows, the two-half form): <= 128 VGPRs, no scratch, LDS such that four two-half
    blocks or eight one-row blocks fit on a CU -- the energies use the free upper halves of the slots, no LDS of their own"""
    rows = [(n, r) for n, r in kernels.items() if n.startswith("void k_rows_re<")]
    assert len(rows) == 3, sorted(n for n, _ in rows)
    for n, r in rows:
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
        two = re.match(r"void k_rows_re<Sched<[^>]*>, \d+, (true|false)>", n).group(1) == "true"
        m2 = int(re.search(r"Sched<(\d+)", n).group(1)) * (2 if two else 1)
        assert (4 if two else 8) * (m2 * 16 + r["group_segment_fixed_size"]) <= 160 * 1024, (n, r)


def test_pruned_inverse_kernels_keep_the_column_budgets(kernels):
    cols = [(args + " " + first, r) for args, rs in kernel_forms(kernels, "k_inv_cols_r", "prune").items() for first, r in rs]
    assert len(cols) == 6 and sorted(n.split()[-1] for n, _ in cols) == ["false"] * 3 + ["true"] * 3, sorted(n for n, _ in cols)  # three column schedules x {first two tiles, the rest}
    for n, r in cols:
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
        m1 = int(re.search(r"Sched<(\d+)", n).group(1))
        assert 2 * (m1 * 16 * 8 + r["group_segment_fixed_size"]) <= 160 * 1024, (n, r)
    for name in ("k_tile_bounds", "k_prune_select"):
        (n, r), = [(n, r) for n, r in kernels.items() if n.startswith(name + "(")]
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)


def test_the_existing_row_and_inverse_kernels_are_still_there(kernels):
    assert len([n for n in kernels if n.startswith("void k_rows_r<")]) == 12
    assert len(kernel_forms(kernels, "k_inv_cols_r", "all")) == 3


def test_two_half_row_kernel_with_energies_issues_no_load_behind_a_barrier():
    if not os.path.exists(order.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    if not order.rocm_version().startswith(order.PINNED_ROCM):
        pytest.skip("instruction orders are pinned to ROCm %s" % order.PINNED_ROCM)
    asx()
    import subprocess
    d = order.disassembly(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    names = subprocess.run(["c++filt"], input="\n".join(d), capture_output=True, text=True).stdout.split("\n")
    isa = {nm: d[k] for nm, k in zip(names, d)}
    ins = order.one(isa, "void k_rows_re<Sched<1200, 12, 10, 10>, 128, true>")
    barriers = order.positions(ins, lambda s: s.startswith("s_barrier"))
    loads = order.positions(ins, lambda s: s.startswith("global_load"))
    assert len(barriers) >= 5 and loads, (len(barriers), len(loads))  # k_rows_r's four and the one in front of the tile sums
    late = [i for i in loads if i > barriers[0]]
    assert not late, [ins[i] for i in late][:4]
