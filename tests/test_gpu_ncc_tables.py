"""The float64 tables behind the normalised cross-correlation on the MI355X, read through Plan.debug_ncc_tables and held to the exact
integer reference of tests/ncc_exact.py: the per-lag table {Sx', Vx} of k_ncc_table, the track's Vmax, Sy and Vy of the sample, the
prefix and suffix tables of k_nccfull_prefix -- for the strided call, the full-range call and the pool call.  Every sum is the exact
integer, every variance within TABLE_TOL of the exact rational; Vmax is reset between calls; a track's tables do not depend on its
place; and the competing set is the exact rule's at every lag, with no band around the threshold left out."""
import numpy as np
import pytest

import ncc_exact as ex
from util import asx

pytestmark = pytest.mark.gpu

# The variance figures of ncc_exact.compare(): |V_dev - V_exact| over the scale sum (x - mean)^2 -- the loudest window's for the
# sliding table, the prefix's or suffix's own for the full-range tables, the sample's for Vy -- and, for inputs A and B, over Vx
# itself.  Every test prints its figures per table, input and length (pytest -s).
# Measured on an MI355X, with the assertions at the hard cap, the largest value over the inputs A to E and the three calls:
#   per table   sliding Vx 5.95e-16 (over Vx itself: input A 4.31e-16, input B 5.96e-16 -- the offset costs no digits), Vmax 4.66e-16,
#               Vy 2.15e-16, the prefix table 9.95e-16, the suffix table 9.17e-16
#   per length  N = 1 and 2: 0, 3: 2.1e-16, 1023: 8.9e-16, 1024: 3.9e-16, 1025: 8.3e-16, 2047: 9.95e-16, 2048: 5.4e-16, 2049: 8.1e-16,
#               4096: 5.2e-16, 5000: 7.7e-16, 144 000: 9.8e-16, 960 000: 9.2e-16 (sliding Vx there 3.97e-16)
# a few ulps of float64 at every length, K = 468 chunk sums per window included.  Asserted at four times the largest value seen,
# 3.98e-15, rounded up to one significant digit.  The hard cap, 1e-9, stays 150 times below what one wrong frame of input A moves a
# window's variance by at N = 960 000; four times a measurement above it would be a finding about the kernel, not a reason to raise
# it.  The sums and the means are not under a tolerance at all: ncc_exact.compare() asserts the exact integers and the exact bits.
TABLE_TOL = 4e-15
assert TABLE_TOL <= 1e-9

# Packed plans at the lengths the chunk arithmetic tells apart (2048 frames per chunk, 2048 lags per block): 1, 2 and 3 (no, one and
# two negative lags), 1023 / 1024 / 1025 (the source's 2N frames straddle a chunk edge while N does not), 2047 / 2048 / 2049 (the
# edge of the sample and of the lag blocks), 4096 (two lag blocks and no remainder frames), 5000 (three blocks, two whole chunks per
# window).  Real-column plans: 144 000, and 960 000 -- K = 468 whole chunks per window, a prefix that starts from up to 468 chunk
# sums: the one length at which ncc_sum_arrays takes more than one element per thread.
PACKED = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 5000)
BIG = 144000
LONGEST = 960000

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tracks(kind, n, prefix):
    """the float32 tracks of an input"""
    return cached(("f32", kind, n, prefix), lambda: tuple(ex.f32(x) for x in ex.pair(kind, n, prefix)))


def exact_of(kind, n, prefix):
    """the exact reference of an input, computed once (with the full-range entries for the prefix variant) and never written to"""
    return cached(("exact", kind, n, prefix), lambda: ex.exact(*ex.pair(kind, n, prefix), full=prefix))


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    assert t.cuda.is_available()
    return t


def call(plan, which, src, smp):
    """one call of the kind that fills the set `which`; src, smp: one pair's tracks or stacked ones"""
    if which == "strided":
        return plan.xcorr_ncc_f32(src, smp)
    if which == "full":
        return plan.xcorr_ncc_full_f32(src, smp)
    src, smp = np.atleast_2d(src), np.atleast_2d(smp)
    return plan.xcorr_pool_ncc_f32(src, smp, np.array([(k, k) for k in range(src.shape[0])], dtype=np.int32))


def check(plan, which, kind, n):
    """a call on input `kind`, then its tables against the exact reference.  -> the tables"""
    prefix = which == "full"
    src, smp = tracks(kind, n, prefix)
    call(plan, which, src, smp)
    dev = plan.debug_ncc_tables(which)
    fig = ex.compare(dev, exact_of(kind, n, prefix), relative=kind in "AB")
    print("ncc tables", which, kind, n, " ".join("%s %.3g" % kv for kv in sorted(fig.items())))
    assert all(v <= TABLE_TOL for v in fig.values()), (which, kind, n, fig)
    return dev


@pytest.mark.parametrize("n", PACKED)
def test_tables_on_packed_plans(mod, n):
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "packed"
        for kind in ex.KINDS if n >= 1000 else "ABC":
            check(plan, "strided", kind, n)
            check(plan, "full", kind, n)


def test_tables_on_a_real_column_plan(mod):
    with mod.Plan(BIG, 1, 0) as plan:
        assert plan.layout == "real-column"
        for kind in ex.KINDS:
            one = check(plan, "strided", kind, BIG)
            check(plan, "full", kind, BIG)
            pool = check(plan, "pool", kind, BIG)
            assert same_tables(one, pool), kind          # the pool call's tables: the strided call's for the same track


def test_tables_at_the_longest_length(mod):
    """K = 468 whole chunks per window and up to 468 chunk sums in front of a prefix: ncc_sum_arrays loops.  Inputs A and C."""
    with mod.Plan(LONGEST, 1, 0) as plan:
        assert plan.layout == "real-column"
        for kind in "AC":
            check(plan, "strided", kind, LONGEST)
            check(plan, "full", kind, LONGEST)


def same_tables(a, b):
    """bit for bit (the full-range tables from index 1 on: index 0 is never written)"""
    if sorted(a) != sorted(b):
        return False
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if key in ("ptab", "ttab"):
            x, y = x[1:], y[1:]
        if x.tobytes() != y.tobytes():
            return False
    return True


@pytest.mark.parametrize("n", [2049, BIG])
def test_vmax_is_reset_between_calls(mod, n):
    """the same plan and slot: a call with input A, then one with input B, whose Vmax is thousands of times smaller"""
    with mod.Plan(n, 1, 0) as plan:
        for which in ("strided", "full") + (("pool",) if plan.layout == "real-column" else ()):
            loud = check(plan, which, "A", n)["vmax"]
            dev = check(plan, which, "B", n)
            want = exact_of("B", n, which == "full")["Vx"].max()
            print("ncc tables vmax", which, n, "A", loud, "then B", dev["vmax"], "exact", want)
            assert dev["vmax"] == dev["table"][:, 1].max() and dev["vmax"] < loud / 1000, (which, loud, dev["vmax"])
            assert abs(dev["vmax"] - want) <= TABLE_TOL * want


@pytest.mark.parametrize("n", [2049, BIG])
def test_places(mod, n):
    """inputs A, B and C as the three pairs of one group: each one's tables are, bit for bit, those of a call on that pair alone,
    and the pool call's for a track the strided call's"""
    with mod.Plan(n, 3, 0) as plan:
        assert plan.group >= 3
        sets = ("strided", "full") + (("pool",) if plan.layout == "real-column" else ())
        together = {}
        for which in sets:
            pairs = [tracks(kind, n, which == "full") for kind in "ABC"]
            call(plan, which, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            together[which] = [plan.debug_ncc_tables(which, k, k) for k in range(3)]
            for k, kind in enumerate("ABC"):
                fig = ex.compare(together[which][k], exact_of(kind, n, which == "full"), relative=kind in "AB")
                assert all(v <= TABLE_TOL for v in fig.values()), (which, kind, fig)
            # a sample track against another pair's source: the tables are the tracks', not the pairs'
            mixed = plan.debug_ncc_tables(which, 0, 2)
            assert mixed["vy"] == together[which][2]["vy"] and mixed["vmax"] == together[which][0]["vmax"]
        for which in sets:
            for k, kind in enumerate("ABC"):
                call(plan, which, *tracks(kind, n, which == "full"))
                assert same_tables(plan.debug_ncc_tables(which), together[which][k]), (which, kind)
        if "pool" in sets:
            for k in range(3):
                assert same_tables(together["pool"][k], together["strided"][k]), k


def curve(plan, torch, src, smp, min_energy, min_overlap=None):
    """the debug call's d_c: N floats, or the 2N - 1 of the full-range call where min_overlap is given"""
    n = smp.size
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    d_c = torch.full((n if min_overlap is None else 2 * n - 1,), 7.0, dtype=torch.float32, device="cuda")
    out = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    if min_overlap is None:
        plan.ncc_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), min_energy, d_c.data_ptr(), *(a.data_ptr() for a in out))
    else:
        plan.ncc_full_debug_c_dev(d_src.data_ptr(), d_smp.data_ptr(), min_energy, min_overlap, d_c.data_ptr(),
                                  *(a.data_ptr() for a in out))
    plan.sync()
    return d_c.cpu().numpy()


@pytest.mark.parametrize("n", ex.COMPETE_LENGTHS)
@pytest.mark.parametrize("kind", ex.COMPETE_KINDS)
def test_the_competing_set_exactly(mod, torch, kind, n):
    """Inputs D and E: the NaN pattern of d_c is the exact rule's at every lag.  tests/test_ncc_exact.py shows that no lag's exact
    energy lies within 1e-9 of a threshold, and the tables are within TABLE_TOL <= 1e-9 of the exact ones (the tests above), so
    nothing is left to the last bits."""
    with mod.Plan(n, 1, 0) as plan:
        src, smp = tracks(kind, n, False)
        e = exact_of(kind, n, False)
        for me in ex.ENERGIES:
            ok = ~np.isnan(curve(plan, torch, src, smp, me))
            want = ex.competing(e, me)
            print("ncc competing", kind, n, me, int(ok.sum()), "of", n)
            assert np.array_equal(ok, want), (kind, n, me, np.flatnonzero(ok != want)[:8])
            if me == 1.0:
                dev = plan.debug_ncc_tables("strided")
                assert ok.sum() >= 1 and np.array_equal(ok, dev["table"][:, 1] == dev["vmax"])
        src, smp = tracks(kind, n, True)
        e = exact_of(kind, n, True)
        for me in ex.ENERGIES:
            for mo in ex.overlaps(n):
                ok = ~np.isnan(curve(plan, torch, src, smp, me, mo))
                want = ex.competing_low(e, me, mo)
                print("ncc competing l < 0", kind, n, me, mo, int(ok[:n - 1].sum()), "of", n - 1)
                assert np.array_equal(ok[:n - 1], want), (kind, n, me, mo, np.flatnonzero(ok[:n - 1] != want)[:8])
                assert np.array_equal(ok[n - 1:], ex.competing(e, me)), (kind, n, me, mo)
            if me == 1.0:
                dev = plan.debug_ncc_tables("full")
                assert np.array_equal(ok[n - 1:], dev["table"][:, 1] == dev["vmax"]) and ok[n - 1:].sum() >= 1


def test_refusals(mod):
    n = 2049
    src, smp = tracks("A", n, False)
    with mod.Plan(n, 2, 0) as plan:
        for which in ("strided", "pool", "full"):
            with pytest.raises(mod.AsxError, match="no such set"):
                plan.debug_ncc_tables(which)
        plan.xcorr_ncc_f32(src, smp)
        before = plan.debug_ncc()
        plan.debug_ncc_tables("strided", plan.group - 1, plan.group - 1)     # inside the set
        for s, t in ((plan.group, 0), (0, plan.group)):
            with pytest.raises(mod.AsxError, match="outside"):
                plan.debug_ncc_tables("strided", s, t)
        with pytest.raises(mod.AsxError, match="no such set"):
            plan.debug_ncc_tables("full")
        assert mod.lib().asx_plan_debug_ncc_tables(plan._h, 3, 0, 0, None, None, None, None, None) == -1
        assert mod.lib().asx_plan_debug_ncc_tables(None, 0, 0, 0, None, None, None, None, None) == -1
        assert plan.debug_ncc() == before
