"""Triangle closure over a clip pool (asx_pool_closure_dev), the parts that need no GPU: what the rule of tests/closure_model.py does
on planted pools -- it finds the true lag where the coefficient alone takes a decoy, every pair it still gets wrong is flagged by
confirm 0, and the clips land on their offsets; the edges of the rule on hand-written tables; the header, the C-ABI and the binding;
the host checks of closure_args; the four kernels within their budget; and, at N = 144 000, that the float64 references alone
(tests/topk_model.py, then the closure model) meet the premise of the end-to-end GPU test: a planted private event is entry 0 of
its pair and closure picks the true lag behind it.

Two things the issue's wording does not fit, stated here and held as written:
  * k = 1 makes the pick the identity, so at (C, k) = (3, 1) closure is right exactly as often as the coefficient alone (5 of 6);
    "above the by-coefficient count" is asserted for every k > 1 and "equal" there.
  * with periodic decoys a wrong pick CAN be confirmed by another wrong pick one period off: of the seeds 1, 2, 3 at (8, 3) with
    period 2400, seed 3 has every wrong pair at confirm 0 (the case asserted); seeds 1 and 2 each have a wrong pair with confirm 1."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import closure_model as cm
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALL = "asx_pool_closure_dev"
OUTPUTS = ("best_lag", "best_coef", "best_ret", "best_entry", "confirm", "offset", "support", "placed")


def take(table, entry):
    return np.take_along_axis(table, entry[:, :, None].astype(np.int64), axis=2)[:, :, 0]


def right_pairs(p, lag, ret):
    """the pairs off the diagonal whose kept lag is within one frame of the planted one"""
    C = lag.shape[0]
    return (np.abs(lag - p["true_lag"]) <= 1) & (ret == 0) & ~np.eye(C, dtype=bool)


# ---- A. the model on planted pools ------------------------------------------------------------------------------------------------
# (C, k, seed): (pairs that hold the true lag, right by closure, right by coefficient), as the model gives them
FACTS = {(2, 2, 1): (2, 2, 1), (3, 1, 1): (5, 5, 5), (6, 3, 1): (28, 28, 0), (9, 4, 1): (70, 70, 0), (5, 8, 1): (18, 18, 0),
         (16, 4, 1): (238, 238, 0)}


@pytest.mark.parametrize("C,k,seed", sorted(FACTS))
def test_closure_finds_what_the_coefficient_misses(C, k, seed):
    p = cm.planted(C, k, seed)
    out = cm.closure(p["lag"], p["coef"], p["ret"], 2)
    e = cm.by_coefficient(p["coef"], p["ret"])
    by_closure = right_pairs(p, out["best_lag"], out["best_ret"])
    by_coef = right_pairs(p, take(p["lag"], e), take(p["ret"], e))
    holds = p["true_entry"] >= 0
    print((C, k, seed), "hold", int(holds.sum()), "closure", int(by_closure.sum()), "coefficient", int(by_coef.sum()))
    assert (int(holds.sum()), int(by_closure.sum()), int(by_coef.sum())) == FACTS[(C, k, seed)]
    assert int(holds.sum()) == C * (C - 1) - cm.bad_count(C, 2)
    # the two legs' jitter is at most 2 frames, the tolerance: every pair that holds the true lag is picked right
    assert (by_closure | ~holds).all()
    assert by_closure.sum() > by_coef.sum() if k > 1 else by_closure.sum() == by_coef.sum()
    wrong = ~by_closure & ~np.eye(C, dtype=bool)
    assert (out["confirm"][wrong] == 0).all()
    assert out["placed"].tolist() == [1] * C
    assert (np.abs(out["offset"] - (p["T"] - p["T"][out["root"]])) <= 1).all()
    # the (0, NaN, -3) entry is there, got no vote and was not picked
    nan = np.argwhere(p["ret"] == -3)
    assert len(nan) == 1 and out["votes"][tuple(nan[0])] == 0
    if k > 1:
        assert out["best_entry"][nan[0][0], nan[0][1]] != nan[0][2]


def test_periodic_decoys_leave_wrong_pairs_and_flag_them():
    p = cm.planted(8, 3, 3, period=2400)
    out = cm.closure(p["lag"], p["coef"], p["ret"], 2)
    ok = right_pairs(p, out["best_lag"], out["best_ret"])
    wrong = ~ok & ~np.eye(8, dtype=bool)
    assert int(ok.sum()) == 53 and int(wrong.sum()) == 3
    assert (out["confirm"][wrong] == 0).all()
    assert (np.abs(out["offset"] - (p["T"] - p["T"][out["root"]])) <= 1).all() and out["placed"].all()


def test_decoys_at_plus_minus_p_in_every_pair_tie_and_fall_back_to_the_coefficient():
    """the stated ambiguity: shifting one clip by P closes every triangle, so lags alone cannot decide"""
    C, P = 5, 2400
    rng = np.random.default_rng(7)
    T = rng.integers(0, 50000, size=C)
    true = (T[None, :] - T[:, None]).astype(np.int64)
    lag = np.stack([true, true + P, true - P], axis=2)
    coef = np.stack([np.full((C, C), 0.4), rng.uniform(0.6, 0.9, (C, C)), rng.uniform(0.6, 0.9, (C, C))], axis=2)
    ret = np.zeros((C, C, 3), dtype=np.int32)
    for tol in (0, 2):
        out = cm.closure(lag, coef, ret, tol)
        off = ~np.eye(C, dtype=bool)
        assert (out["votes"][off] == C - 1).all()                       # the true entry and both decoys: every clip supports each
        assert (out["best_entry"] == cm.by_coefficient(coef, ret)).all()
        assert (out["best_entry"][off] != 0).all()


# ---- B. the edges of the rule -----------------------------------------------------------------------------------------------------
def empty(C, k):
    """a table in which no pair was computed: (0, NaN, -3) everywhere, the diagonal as the pool call returns it"""
    lag = np.zeros((C, C, k), dtype=np.int64)
    coef = np.full((C, C, k), np.nan)
    ret = np.full((C, C, k), -3, dtype=np.int32)
    for a in range(C):
        lag[a, a, 0], coef[a, a, 0], ret[a, a, 0] = 0, 1.0, 0
    return lag, coef, ret


def put(t, a, b, entries):
    for j, (l, c) in enumerate(entries):
        t[0][a, b, j], t[1][a, b, j], t[2][a, b, j] = l, c, 0


def test_ties_go_to_the_coefficient_and_then_to_the_smaller_j():
    t = empty(2, 3)
    put(t, 0, 1, [(100, 0.5), (200, 0.7), (300, 0.7)])
    put(t, 1, 0, [(-100, 0.2), (-200, 0.2), (-300, 0.2)])
    out = cm.closure(*t, 0)
    assert out["votes"][0, 1].tolist() == [1, 1, 1] and out["best_entry"][0, 1] == 1 and out["best_lag"][0, 1] == 200
    assert out["best_entry"][1, 0] == 0                                    # all equal: the smallest j
    t[2][1, 0, 1:] = -1                                                    # only -100 is left to support: votes beat coefficients
    out = cm.closure(*t, 0)
    assert out["votes"][0, 1].tolist() == [1, 0, 0] and out["best_entry"][0, 1] == 0 and out["confirm"][0, 1] == 1


def test_a_nan_coefficient_never_displaces_an_entry():
    t = empty(2, 3)
    put(t, 0, 1, [(100, 0.1), (200, np.nan), (300, -0.5)])
    put(t, 1, 0, [(-100, 0.2), (-200, 0.2), (-300, 0.2)])
    out = cm.closure(*t, 0)
    assert out["votes"][0, 1].tolist() == [1, 1, 1] and out["best_entry"][0, 1] == 0
    t[2][1, 0, 0] = -1                                                     # ... but more votes do, NaN or not
    out = cm.closure(*t, 0)
    assert out["votes"][0, 1].tolist() == [0, 1, 1] and out["best_entry"][0, 1] == 1 and np.isnan(out["best_coef"][0, 1])


def test_a_lag_past_the_limit_is_not_valid():
    t = empty(2, 2)
    put(t, 0, 1, [(cm.LAG_MAX + 1, 0.9), (5, 0.1)])
    put(t, 1, 0, [(-cm.LAG_MAX - 1, 0.9), (-cm.LAG_MAX, 0.8)])
    out = cm.closure(*t, 2)
    assert out["best_entry"][0, 1] == 1 and out["best_lag"][0, 1] == 5 and out["votes"][0, 1].tolist() == [0, 0]
    assert out["best_entry"][1, 0] == 1 and out["best_lag"][1, 0] == -cm.LAG_MAX          # 2^40 itself is valid
    t[0][0, 1, 1] = cm.LAG_MAX                                             # ... and takes part in sums
    out = cm.closure(*t, 0)
    assert out["votes"][0, 1].tolist() == [0, 1] and out["votes"][1, 0].tolist() == [0, 1]


def test_a_pair_with_no_valid_entry_is_copied_and_never_good():
    t = empty(3, 2)
    put(t, 0, 1, [(10, 0.5), (11, 0.4)])
    put(t, 1, 0, [(-10, 0.5), (-11, 0.4)])
    t[0][0, 2] = [7, 8]
    t[1][0, 2, 0] = np.float64(np.frombuffer(np.uint64(0x7FF8000000000ABC).tobytes(), dtype=np.float64)[0])
    t[2][0, 2] = [-1, 0]
    t[0][0, 2, 1] = cm.LAG_MAX + 5                                         # ret 0, but past the limit
    out = cm.closure(*t, 1, min_confirm=0)
    assert (out["best_lag"][0, 2], out["best_ret"][0, 2], out["best_entry"][0, 2]) == (7, -1, 0)
    assert out["best_coef"][0, 2].tobytes() == t[1][0, 2, 0].tobytes()     # the NaN's payload too
    assert out["confirm"][0, 2] == 0 and out["placed"].tolist() == [1, 1, 0]


def test_k_1_is_the_identity():
    p = cm.planted(6, 1, 5)
    out = cm.closure(p["lag"], p["coef"], p["ret"], 2)
    assert out["best_lag"].tobytes() == p["lag"][:, :, 0].tobytes() and out["best_ret"].tobytes() == p["ret"][:, :, 0].tobytes()
    assert out["best_coef"].tobytes() == np.ascontiguousarray(p["coef"][:, :, 0]).tobytes() and not out["best_entry"].any()


def test_one_clip():
    out = cm.closure(np.zeros((1, 1, 3), np.int64), np.array([[[1.0, 0.2, 0.1]]]), np.zeros((1, 1, 3), np.int32), 0)
    assert out["root"] == 0 and out["placed"].tolist() == [1] and out["offset"].tolist() == [0] and out["support"].tolist() == [0]
    assert out["confirm"].tolist() == [[0]] and not out["votes"].any() and out["best_entry"].tolist() == [[0]]


def consistent(T, k=1):
    C = len(T)
    t = empty(C, k)
    for a in range(C):
        for b in range(C):
            if a != b:
                put(t, a, b, [(T[b] - T[a], 0.5)])
    return t


def test_min_confirm_decides_what_is_usable():
    t = consistent([0, 100, 250])
    out = cm.closure(*t, 0, min_confirm=0)
    assert out["placed"].tolist() == [1, 1, 1] and out["offset"].tolist() == [0, 100, 250] and out["support"].tolist() == [0, 4, 4]
    assert (out["confirm"][~np.eye(3, dtype=bool)] == 2).all()
    assert cm.closure(*t, 0, min_confirm=2)["offset"].tolist() == [0, 100, 250]
    out = cm.closure(*t, 0, min_confirm=3)                                 # nothing is usable: only the root is placed
    assert out["root"] == 0 and out["placed"].tolist() == [1, 0, 0] and out["offset"].tolist() == [0, 0, 0]
    assert out["support"].tolist() == [0, 0, 0]


def test_a_given_root_and_a_chosen_one():
    t = consistent([0, 100, 250, 300])
    assert cm.closure(*t, 0)["root"] == 0                                  # all scores equal: the smallest index
    out = cm.closure(*t, 0, root=2)
    assert out["root"] == 2 and out["offset"].tolist() == [-250, -150, 0, 50] and out["placed"].tolist() == [1] * 4
    t[2][0, :, :] = -1                                                     # clip 0 as a source computed nothing ...
    t[2][1, 0, :] = -1                                                     # ... and (1, 0) neither: clips 2 and 3 lead with 5 usable pairs
    t[2][0, 0, 0] = 0
    out = cm.closure(*t, 0)
    assert out["root"] == 2 and out["offset"].tolist() == [-250, -150, 0, 50]


def test_the_lower_median_of_an_even_count():
    t = empty(3, 1)
    for (a, b), l in {(0, 1): 10, (1, 0): -12, (0, 2): 4, (2, 1): 10, (1, 2): -6, (2, 0): -10}.items():
        put(t, a, b, [(l, 0.5)])
    out = cm.closure(*t, 2, min_confirm=0, root=0)
    # E_1 = {10, 12, 14, 16}, E_2 = {2, 4, 4, 10}
    assert out["offset"].tolist() == [0, 12, 4] and out["support"].tolist() == [0, 3, 3] and out["placed"].tolist() == [1, 1, 1]


def test_three_hops_are_not_placed():
    t = empty(4, 1)
    for a in range(3):
        put(t, a, a + 1, [(100, 0.5)])
    out = cm.closure(*t, 0, min_confirm=0, root=0)
    assert out["placed"].tolist() == [1, 1, 1, 0] and out["offset"].tolist() == [0, 100, 200, 0] and out["support"].tolist() == [0, 1, 1, 0]


def edge_cases():
    """the hand-written tables of the tests above as (name, (lag, coef, ret), tolerance, min_confirm, root), for the device
    (tests/test_gpu_closure.py runs each against the model)"""
    out = []

    def add(name, t, tol, mc=1, root=-1):
        out.append((name, tuple(a.copy() for a in t), tol, mc, root))

    t = empty(2, 3)
    put(t, 0, 1, [(100, 0.5), (200, 0.7), (300, 0.7)])                     # equal votes, equal finite coefficients: the smaller j
    put(t, 1, 0, [(-100, 0.2), (-200, 0.2), (-300, 0.2)])
    add("ties", t, 0)
    t[2][1, 0, 1:] = -1
    add("votes beat coefficients", t, 0)
    t = empty(2, 3)
    put(t, 0, 1, [(100, 0.1), (200, np.nan), (300, -0.5)])
    put(t, 1, 0, [(-100, 0.2), (-200, 0.2), (-300, 0.2)])
    add("a NaN does not displace", t, 0)
    t[2][1, 0, 0] = -1
    add("a NaN with more votes", t, 0)
    t = empty(2, 2)
    put(t, 0, 1, [(cm.LAG_MAX + 1, 0.9), (5, 0.1)])
    put(t, 1, 0, [(-cm.LAG_MAX - 1, 0.9), (-cm.LAG_MAX, 0.8)])
    add("past the limit", t, 2)
    t[0][0, 1, 1] = cm.LAG_MAX
    add("at the limit", t, 0)
    t = empty(3, 2)                                                        # the largest sums there are, under the largest tolerance
    put(t, 0, 1, [(cm.LAG_MAX, 0.5), (-cm.LAG_MAX, 0.4)])
    put(t, 1, 0, [(-cm.LAG_MAX, 0.5), (0, 0.4)])
    put(t, 0, 2, [(cm.LAG_MAX, 0.5), (-cm.LAG_MAX, 0.6)])
    put(t, 2, 1, [(cm.LAG_MAX, 0.5), (-cm.LAG_MAX, 0.6)])
    put(t, 1, 2, [(1, 0.5), (cm.LAG_MAX + 1, 0.6)])
    put(t, 2, 0, [(-cm.LAG_MAX, 0.5), (-cm.LAG_MAX - 1, 0.6)])
    add("the largest tolerance", t, cm.LAG_MAX, 0)
    add("the largest lags, tolerance 0", t, 0, 0, 2)
    t = empty(3, 2)
    put(t, 0, 1, [(10, 0.5), (11, 0.4)])
    put(t, 1, 0, [(-10, 0.5), (-11, 0.4)])
    t[0][0, 2] = [7, cm.LAG_MAX + 5]
    t[1][0, 2, 0] = np.frombuffer(np.uint64(0x7FF8000000000ABC).tobytes(), dtype=np.float64)[0]
    t[2][0, 2] = [-1, 0]
    add("no valid entry", t, 1, 0)
    add("one clip", (np.zeros((1, 1, 3), np.int64), np.array([[[1.0, 0.2, 0.1]]]), np.zeros((1, 1, 3), np.int32)), 0)
    t = consistent([0, 100, 250])
    for mc in (0, 2, 3):
        add("min_confirm %d" % mc, t, 0, mc)
    t = consistent([0, 100, 250, 300])
    add("all scores equal", t, 0)
    add("a given root", t, 0, 1, 2)
    t[2][0, :, :] = -1
    t[2][1, 0, :] = -1
    t[2][0, 0, 0] = 0
    add("a chosen root", t, 0)
    t = empty(3, 1)
    for (a, b), l in {(0, 1): 10, (1, 0): -12, (0, 2): 4, (2, 1): 10, (1, 2): -6, (2, 0): -10}.items():
        put(t, a, b, [(l, 0.5)])
    add("the lower median", t, 2, 0, 0)
    t = empty(4, 1)
    for a in range(3):
        put(t, a, a + 1, [(100, 0.5)])
    add("three hops", t, 0, 0, 0)
    return out


def test_the_edge_tables_for_the_device_say_what_the_tests_above_say():
    cases = {name: cm.closure(*t, tol, mc, root) for name, t, tol, mc, root in edge_cases()}
    assert len(cases) == len(edge_cases()) == 18                          # (no name twice)
    assert cases["ties"]["best_entry"][0, 1] == 1 and cases["ties"]["votes"][0, 1].tolist() == [1, 1, 1]
    assert cases["a NaN does not displace"]["best_entry"][0, 1] == 0 and cases["a NaN with more votes"]["best_entry"][0, 1] == 1
    assert cases["at the limit"]["votes"][0, 1].tolist() == [0, 1]
    big = cases["the largest tolerance"]
    # (0, 1, 0) = 2^40: the reverse -2^40 closes it, and over clip 2 the sum 2^40 + 2^40 is 2^40 off, the tolerance;
    # (0, 1, 1) = -2^40: the reverse 0 is 2^40 off, and over clip 2 the sum 2^40 - 2^40 too; (1, 2, 1) is past the limit
    assert big["votes"][0, 1].tolist() == [2, 2] and big["votes"][1, 2].tolist() == [2, 0]
    # ... and with tolerance 0 only the reverse -2^40 is left for (0, 1, 0)
    assert cases["the largest lags, tolerance 0"]["votes"][0, 1].tolist() == [1, 0]
    assert cases["the lower median"]["offset"].tolist() == [0, 12, 4] and cases["three hops"]["placed"].tolist() == [1, 1, 1, 0]
    assert cases["a chosen root"]["root"] == 2 and cases["min_confirm 3"]["placed"].tolist() == [1, 0, 0]


def test_the_kernels_limit_is_the_headers():
    internal = open(os.path.join(graft.PKG_DIR, "csrc", "asx_internal.h")).read()
    api = open(os.path.join(graft.PKG_DIR, "csrc", "asx_api.hip")).read()
    kernels = open(os.path.join(graft.PKG_DIR, "csrc", "xcorr_kernels.hip")).read()
    d = re.search(r"^#define\s+ASX_CLOSURE_LAG_LIMIT\s+\(\(int64_t\)1 << (\d+)\)", internal, flags=re.M)
    assert d and 1 << int(d.group(1)) == cm.LAG_MAX
    assert "#define ASX_CLOSURE_LAG_MAX" not in internal and "#define ASX_CLOSURE_LAG" not in kernels
    assert "static_assert(ASX_CLOSURE_LAG_MAX == ASX_CLOSURE_LAG_LIMIT" in api


# ---- C. surface -------------------------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()


def test_the_call_is_declared_listed_and_exported():
    hdr = header()
    m = asx()
    from audiosync_amd import hipxcorr
    assert re.search(r"\bint %s\s*\(" % CALL, hdr)
    assert CALL in hipxcorr.ABI_SYMBOLS and CALL in hipxcorr.SIGNATURES
    restype, args = hipxcorr.SIGNATURES[CALL]
    assert restype is ctypes.c_int and len(args) == 19
    assert args[3:8] == [ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert args[:3] == [ctypes.c_void_p] * 3 and args[8:] == [ctypes.c_void_p] * 11
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    assert hasattr(L, CALL)                                                # (fails without the feature)
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    d = re.search(r"^#define\s+ASX_CLOSURE_LAG_MAX\s+\(\(int64_t\)1 << (\d+)\)", hdr, flags=re.M)
    assert d and 1 << int(d.group(1)) == hipxcorr.CLOSURE_LAG_MAX == cm.LAG_MAX == 1 << 40
    assert hdr.index("int asx_topk_best_dev") < hdr.index("int " + CALL)
    for name in ("pool_closure_dev", "pool_closure", "closure_args"):
        assert callable(getattr(m, name)) and callable(getattr(hipxcorr, name)), name


def test_the_header_states_the_rule():
    flat = re.sub(r"[\s*]+", " ", header())
    at = flat.index("Each pair's lag by triangle closure over a clip pool")
    text = flat[at:flat.index("int " + CALL, at)]
    for phrase in ("d_pairs == NULL and nsources = nsamples = C = nclips", "pair (a, b) is index a * C + b", "(a * C + b) * k + j",
                   "the lag of pair (a, b) estimates T_b - T_a", "lag_ac + lag_cb", "lag_ab = -lag_ba",
                   "fills the others with ret != 0", "Everything is integer arithmetic, apart from coefficient comparisons",
                   "valid when ret == 0 and |lag| <= ASX_CLOSURE_LAG_MAX", "fits an int64",
                   "|lag_abj + lag_baq| <= tolerance", "|lag_acp + lag_cbq - lag_abj| <= tolerance",
                   "Votes count clips, not combinations", "0 .. C - 1", "Invalid entries and the diagonal get 0",
                   "receives all C * C * k values", "scan j upwards over the valid entries", "its votes are larger",
                   "coef[j] > coef[best]", "a NaN never wins", "the smallest j wins ties", "entry 0 is copied as it is",
                   "best_entry = 0", "the layout asx_results_to_ms_dev takes", "asx_topk_best_dev's rule", "the pick is the identity",
                   "good when a != b and it has a valid entry", "|L_ab + L_ba| <= tolerance", "|L_ac + L_cb - L_ab| <= tolerance",
                   "only the PICKED entries vote", "confirms nothing", "usable when it is good and confirm >= min_confirm",
                   "score[a] = #usable (a, .) + #usable (., a)", "the smallest index wins among equals",
                   "offset 0, support 0, placed 1", "L_rb if (r, b) is usable", "-L_br if (b, r) is usable", "L_rc + L_cb",
                   "-(L_bc + L_cr)", "the lower median of E_b", "(|E_b| - 1) / 2", "within tolerance of the median",
                   "An empty E_b gives offset 0, support 0, placed 0", "decoys at +-P", "lags alone cannot decide",
                   "falls back to the coefficient", "nothing launched and the outputs untouched", "nclips == 0",
                   "nclips * nclips * k > INT32_MAX", "k outside 1..ASX_TOPK_MAX", "tolerance < 0 or > ASX_CLOSURE_LAG_MAX",
                   "min_confirm < 0", "root outside [-1, nclips)", "nclips == 1 is legal", "takes no plan", "allocates nothing",
                   "never synchronises the host", "capturable", "Not offered", "three or more hops", "least-squares",
                   "an explicit pair list", "weighting by coefficient"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase


def test_integration_names_the_call_where_it_promised_it():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    at = doc.index("### The K strongest lags of every pair of two pools")
    section = doc[at:doc.index("**How sharp is a candidate?**", at)]
    assert "asx_pool_closure_dev(" in section and "asx_results_to_ms_dev(d_best_lag" in section
    assert "wants the candidates" not in doc
    assert "pool_closure(" in section


def test_the_host_checks_raise_before_anything_is_uploaded(monkeypatch):
    asx()
    from audiosync_amd import hipxcorr

    def no_device(*a, **kw):
        raise AssertionError("reached the library")

    p = cm.planted(4, 3, 1)
    good = dict(lag=p["lag"], coef=p["coef"], ret=p["ret"], tolerance=2, min_confirm=1, root=-1)
    bad = [dict(lag=p["lag"][:, :3]), dict(lag=p["lag"][:, :, 0]), dict(coef=p["coef"][:3]), dict(ret=p["ret"][:, :, :2]),
           dict(lag=p["lag"].astype(np.float64)), dict(ret=p["ret"].astype(np.float32)), dict(coef=p["coef"].astype(np.complex128)),
           dict(coef=p["coef"] > 0), dict(lag=p["lag"] > 0), dict(lag=np.zeros((2, 2, 9), np.int64), coef=np.zeros((2, 2, 9)),
                                                                 ret=np.zeros((2, 2, 9), np.int32)),
           dict(lag=np.zeros((2, 2, 0), np.int64), coef=np.zeros((2, 2, 0)), ret=np.zeros((2, 2, 0), np.int32)),
           dict(lag=np.zeros((0, 0, 2), np.int64), coef=np.zeros((0, 0, 2)), ret=np.zeros((0, 0, 2), np.int32)),
           dict(tolerance=True), dict(tolerance=2.0), dict(tolerance=-1), dict(tolerance=(1 << 40) + 1), dict(tolerance=None),
           dict(min_confirm=False), dict(min_confirm=1.0), dict(min_confirm=-1), dict(root=True), dict(root=0.0), dict(root=-2),
           dict(root=4), dict(ret=p["ret"].astype(np.int64) + (1 << 40))]
    monkeypatch.setattr(hipxcorr, "lib", no_device)
    monkeypatch.setattr(hipxcorr, "_Staging", no_device)
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.pool_closure(**args)
        with pytest.raises(ValueError):
            hipxcorr.closure_args(**args)
    with pytest.raises(AssertionError):                                    # the stand-in does catch a call that gets through
        hipxcorr.pool_closure(**good)
    lg, cf, rt, C, k, tol, mc, root = hipxcorr.closure_args(p["lag"].astype(np.int32), p["coef"].astype(np.float32), p["ret"].astype(np.int64),
                                                            np.int64(1 << 40), np.int32(0), np.int64(3))
    assert (C, k, tol, mc, root) == (4, 3, 1 << 40, 0, 3) and all(type(v) is int for v in (C, k, tol, mc, root))
    assert (lg.dtype, cf.dtype, rt.dtype) == (np.int64, np.float64, np.int32) and all(a.flags["C_CONTIGUOUS"] for a in (lg, cf, rt))
    assert lg.tobytes() == p["lag"].tobytes() and rt.tobytes() == p["ret"].tobytes()
    assert hipxcorr.closure_args(p["lag"], p["coef"], p["ret"], 0)[5:] == (0, 1, -1)


# ---- D. census --------------------------------------------------------------------------------------------------------------------
def test_four_closure_kernels_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_closure_", n)}
    found = sorted(re.match(r"(?:void )?(k_closure_\w+)", n).group(1) for n in mine)
    assert found == ["k_closure_confirm", "k_closure_offsets", "k_closure_root", "k_closure_votes"], found
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    assert len([n for n in names if re.match(r"(void )?k_topk_best\b", n)]) == 1


# ---- E. the premise of the end-to-end test, by the references alone ------------------------------------------------------------------
E2E_N, E2E_K, E2E_SEP, E2E_TOL = 144000, 3, 1000, 2
E2E_OFFSETS = (0, 20000, 45000, 70000)
# (a, b): (where the private event sits in clip a -- past its first N frames, so the pair (b, a) does not see it --, where in clip b)
E2E_EVENTS = {(0, 1): (150000, 100000), (2, 3): (160000, 90000)}
E2E_EVENT_LEN, E2E_EVENT_GAIN = 30000, 3.0


@functools.lru_cache(maxsize=None)
def e2e_clips():
    """4 clips of 2N frames cut from one noise recording at E2E_OFFSETS, so the lag of (a, b) is offset_b - offset_a; per pair of
    E2E_EVENTS a loud private burst in both clips, which plants the decoy lag pa - pb with r about 3^2 * 30 000 > N"""
    n = E2E_N
    rng = np.random.default_rng(20261)
    rec = rng.standard_normal(max(E2E_OFFSETS) + 2 * n).astype(np.float32)
    clips = np.stack([rec[o:o + 2 * n] for o in E2E_OFFSETS]).copy()
    for (a, b), (pa, pb) in E2E_EVENTS.items():
        burst = (E2E_EVENT_GAIN * rng.standard_normal(E2E_EVENT_LEN)).astype(np.float32)
        clips[a, pa:pa + E2E_EVENT_LEN] += burst
        clips[b, pb:pb + E2E_EVENT_LEN] += burst
    clips.setflags(write=False)
    return clips


def e2e_true_lags():
    o = np.array(E2E_OFFSETS, dtype=np.int64)
    return o[None, :] - o[:, None]


@functools.lru_cache(maxsize=None)
def e2e_reference_tables():
    from topk_model import model
    clips = e2e_clips()
    C, n = len(clips), E2E_N
    lag = np.zeros((C, C, E2E_K), dtype=np.int64)
    coef = np.zeros((C, C, E2E_K))
    ret = np.zeros((C, C, E2E_K), dtype=np.int32)
    for a in range(C):
        for b in range(C):
            for j, (r, l, c) in enumerate(model(clips[a], clips[b, :n], E2E_K, E2E_SEP)):
                lag[a, b, j], coef[a, b, j], ret[a, b, j] = l, c, r
    return lag, coef, ret


def check_e2e(lag, coef, ret, out):
    """tables of the four clips (the model's or the device's) and closure's outputs for them: the premise and the result"""
    true = e2e_true_lags()
    for (a, b), (pa, pb) in E2E_EVENTS.items():
        assert lag[a, b, 0] == pa - pb != true[a, b] and ret[a, b, 0] == 0, (a, b, lag[a, b])      # entry 0 is the decoy
        assert true[a, b] in lag[a, b, 1:].tolist()
        assert out["best_entry"][a, b] != 0
    assert out["best_lag"].tobytes() == true.tobytes() and not out["best_ret"].any()
    off = ~np.eye(len(true), dtype=bool)
    assert (out["confirm"][off] == 3).all() and (out["confirm"][~off] == 0).all()
    assert out["placed"].tolist() == [1] * 4 and out["root"] == 0
    assert (np.abs(out["offset"] - np.array(E2E_OFFSETS)) <= E2E_TOL).all() and (out["support"][1:] == 6).all()


def test_the_references_alone_meet_the_premise_of_the_end_to_end_test():
    lag, coef, ret = e2e_reference_tables()
    assert (lag[:, :, 0][np.eye(4, dtype=bool)] == 0).all() and (np.abs(coef[:, :, 0][np.eye(4, dtype=bool)] - 1.0) < 1e-12).all()
    check_e2e(lag, coef, ret, cm.closure(lag, coef, ret, E2E_TOL))
    by_coef = take(lag, cm.by_coefficient(coef, ret))
    print("by coefficient:", by_coef.tolist())
