"""What the tile energies cost the row pass in instructions (csrc/rlayout.hip: rows_r_body<..., ENG = true>), read from the
disassembly of the built libaudiosync_hip.so without a GPU.

Round 7's k_rows_re was 9.5 % slower than k_rows_r: +397 instructions on the two waves of the store phase, the tail of a block's life,
eight of every eleven of them integer arithmetic for the LDS address of one |Q|^2.  Round 8 writes column c's value into slot c
itself: one address per thread, the column in the store's offset field.  A refactoring that brings per-value address arithmetic
back (a layout the compiler cannot fold into offsets) shows here as a longer kernel and as stores off several address registers."""
import os
import re
import subprocess

import pytest

import test_kernel_isa_order as order
from util import asx, graft

PARENT_EXTRA = 397  # k_rows_re<two-half> over k_rows_r<two-half, 0> at round 7 (2982 against 2585 instructions)
ROWS_R = "void k_rows_r<Sched<1200, 12, 10, 10>, 128, true, 0>"
ROWS_RE = "void k_rows_re<Sched<1200, 12, 10, 10>, 128, true>"


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(order.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    if not order.rocm_version().startswith(order.PINNED_ROCM):
        pytest.skip("instruction counts are pinned to ROCm %s (found %r)" % (order.PINNED_ROCM, order.rocm_version()))
    asx()
    d = order.disassembly(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    names = subprocess.run(["c++filt"], input="\n".join(d), capture_output=True, text=True).stdout.split("\n")
    return {nm: d[k] for nm, k in zip(names, d)}


def body(ins):
    """the kernel without the alignment padding behind its last instruction"""
    ins = list(ins)
    while ins and (ins[-1].startswith("s_nop") or ins[-1].startswith("s_code_end")):
        ins.pop()
    return ins


def test_tile_energies_cost_the_two_half_row_kernel_at_most_half_of_what_they_did(isa):
    plain, eng = body(order.one(isa, ROWS_R)), body(order.one(isa, ROWS_RE))
    extra = len(eng) - len(plain)
    print("k_rows_r %d instructions, k_rows_re %d: +%d (round 7: +%d)" % (len(plain), len(eng), extra, PARENT_EXTRA))
    assert 0 < extra <= PARENT_EXTRA // 2, (len(plain), len(eng))


def test_energy_stores_share_one_address_register(isa):
    """between the fourth and the fifth barrier (the store phase): 24 four-byte LDS stores -- twelve legs, two halves -- and nothing
    else written to LDS, all of them off ONE address register, each with an offset of its own"""
    ins = body(order.one(isa, ROWS_RE))
    barriers = order.positions(ins, lambda s: s.startswith("s_barrier"))
    assert len(barriers) >= 5, barriers
    phase = ins[barriers[3] + 1:barriers[4]]
    lds_writes = [s for s in phase if s.startswith("ds_write") or s.startswith("ds_store")]
    stores = [s for s in lds_writes if s.startswith("ds_write_b32 ")]
    assert len(stores) == 24 and len(lds_writes) == 24, lds_writes
    addr = {s.split()[1].rstrip(",") for s in stores}
    assert len(addr) == 1, addr
    offsets = [int(m.group(1)) if m else 0 for m in (re.search(r"offset:(\d+)", s) for s in stores)]
    assert len(set(offsets)) == 24 and max(offsets) < 65536, offsets
    # nothing writes that register inside the phase: the address is the thread's, computed once in front of its first store
    reg = int(addr.pop()[1:])
    first = phase.index(stores[0])

    def writes_reg(s):
        op = s.split()
        if len(op) < 2 or op[0].startswith(("ds_write", "global_store", "s_")):
            return False
        m = re.match(r"^v(\d+),?$|^v\[(\d+):(\d+)\],?$", op[1])
        if not m:
            return False
        lo, hi = (int(m.group(1)),) * 2 if m.group(1) else (int(m.group(2)), int(m.group(3)))
        return lo <= reg <= hi

    redefined = [s for s in phase[first + 1:] if writes_reg(s)]
    assert not redefined, redefined


def test_tile_bounds_hand_over_is_the_instruction_sequence_it_rests_on(isa):
    """k_tile_bounds hands a slice's sums to the pair's last block without an agent-scope release (csrc/rlayout.hip says why): that
    is sound on the gfx942 family because of the instructions the atomics become, so each of them is pinned here -- the sums stored
    through (sc1), every wave drained (vmcnt(0)) in front of the barrier behind which the ticket is drawn, the last arriver's cache
    invalidate (buffer_inv sc1) behind the ticket and in front of the barrier behind which the sums are loaded (sc1), and no L2
    write-back anywhere."""
    ins = body(order.one(isa, "k_tile_bounds("))
    barriers = order.positions(ins, lambda s: s.startswith("s_barrier"))
    assert len(barriers) == 3, barriers
    b1, b2 = barriers[0], barriers[1]
    assert not [s for s in ins if s.startswith("buffer_wbl2")]
    # the slice's sums: one eight-byte store, written through, and nothing else stored in front of the first barrier
    stores = order.positions(ins[:b1], lambda s: s.startswith(("global_store", "global_atomic", "flat_store", "flat_atomic")))
    assert len(stores) == 1 and re.match(r"global_store_dwordx2 .* sc1$", ins[stores[0]]), [ins[i] for i in stores]
    drained = [s for s in ins[stores[0] + 1:b1] if s.startswith("s_waitcnt") and "vmcnt(0)" in s]
    assert drained, ins[stores[0]:b1 + 1]
    # the ticket, the last arriver's invalidate behind it, no load of the sums in between
    between = ins[b1 + 1:b2]
    ticket = order.positions(between, lambda s: s.startswith("global_atomic_add"))
    inv = order.positions(between, lambda s: s.startswith("buffer_inv") and s.endswith("sc1"))
    assert len(ticket) == 1 and len(inv) == 1 and ticket[0] < inv[0], between
    assert not [s for s in between if s.startswith(("global_load", "flat_load"))], between
    assert [s for s in between[inv[0] + 1:] if s.startswith("s_waitcnt") and "vmcnt(0)" in s], between[inv[0]:]
    # the sums as the last block reads them: eight-byte loads at agent scope, every one of them
    loads = [s for s in ins[b2 + 1:] if s.startswith(("global_load", "flat_load"))]
    assert loads and all(re.match(r"global_load_dwordx2 .* sc1$", s) for s in loads), loads
