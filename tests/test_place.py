"""Placement over chains of usable pairs (asx_pool_place_dev), the parts that need no GPU: what the rule of tests/place_model.py does
on the tables of long events, where closure alone (tests/closure_model.py) leaves most clips unplaced; hand cases of the rule; the
header, the C-ABI and the binding; the host checks of place_args; and the premises of every fixture that tests/test_gpu_place.py runs
on the device, asserted here on the models alone, so that a GPU failure cannot hide behind a bad fixture.

What the fixtures say and the issue's wording does not:
  * band tables are built per (C, seed); whether garbage lags close a triangle by accident depends on the seed.  The seeds of BANDS
    are ones at which no out-of-band pair is usable at min_confirm 1 and 2 (asserted); at C = 12, seed 2, two such pairs are usable and
    one clip lands 177 011 frames off, which is the second finding of the issue and is asserted too.
  * in these tables every clip has a usable pair and the usable pairs connect them all, so "reaches every clip that has a usable
    pair" is asserted as: hops >= 0 exactly on the root's component, which is every clip."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import closure_model as cm
import place_model as pm
from test_closure import empty, put
from util import ROOT, asx, graft

CALL = "asx_pool_place_dev"
TOL = 4


def component(U, root):
    """the clips that chains of usable pairs, in either direction, connect to root: a plain graph search, not the model's layers"""
    C = U.shape[0]
    link = U | U.T
    seen = np.zeros(C, dtype=bool)
    seen[root] = True
    stack = [root]
    while stack:
        for c in np.flatnonzero(link[stack.pop()] & ~seen):
            seen[c] = True
            stack.append(int(c))
    return seen


def tables(first):
    return first["best_lag"], first["best_ret"], first["confirm"]


# ---- (a) the chain that closure does not finish -------------------------------------------------------------------------------------
def chain_tables():
    t = empty(4, 1)
    for a in range(3):
        put(t, a, a + 1, [(100, 0.5)])
    return t


def test_the_chain_closure_leaves_unplaced_is_placed():
    t = chain_tables()
    closed = cm.closure(*t, 0, min_confirm=0, root=0)
    assert closed["placed"].tolist() == [1, 1, 1, 0]
    out = pm.place(*tables(closed), 0, 0, 0)
    assert out["hops"].tolist() == [0, 1, 2, 3] and out["offset"].tolist() == [0, 100, 200, 300]
    assert out["degree"].tolist() == [1, 2, 2, 1] and out["support"].tolist() == [1, 2, 2, 1] and not out["step"].any()
    assert out["state"].tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]] and not out["resid"].any()
    short = pm.place(*tables(closed), 0, 0, 0, max_hops=2)
    assert short["hops"].tolist() == [0, 1, 2, -1] and short["offset"].tolist() == [0, 100, 200, 0]
    assert short["state"][2, 3] == 0 and short["degree"].tolist() == [1, 2, 1, 0]
    # place_model.chain is the same picked table, for any C
    L, R, F = pm.chain(4)
    assert (pm.usable_pairs(L, R, F, 0) == pm.usable_pairs(*tables(closed), 0)).all()
    assert pm.place(L, R, F, 0, 0, 0)["offset"].tolist() == [0, 100, 200, 300]
    back = pm.place(L, R, F, 3, 0, 0)                                      # against the pairs' direction: o[c] - L_bc
    assert back["hops"].tolist() == [3, 2, 1, 0] and back["offset"].tolist() == [-300, -200, -100, 0]


# ---- (b) band tables: the normal case of a long event ---------------------------------------------------------------------------------
BANDS = {12: (3, 1), 24: (3, 2)}                                           # C: (k, seed)


@functools.lru_cache(maxsize=None)
def band_tables(C, masked=False, spacing=40000, k=None, seed=None):
    kk, ss = BANDS.get(C, (2, C))
    return pm.band(C, k or kk, seed if seed is not None else ss, spacing=spacing, masked=masked)


@functools.lru_cache(maxsize=None)
def band_case(C, masked=False, spacing=40000, k=None, seed=None):
    """band tables and closure's picks for them at TOL -> (band dict, picked dict)"""
    p = band_tables(C, masked, spacing, k, seed)
    return p, cm.picked(p["lag"], p["coef"], p["ret"], TOL)


def check_band(p, first, mc, want_all=True):
    """the premises of a band table at min_confirm mc, and what placement makes of it"""
    C = len(p["T"])
    L, R, F = tables(first)
    U = pm.usable_pairs(L, R, F, mc)
    assert not (U & ~p["in_band"]).any()                                    # no garbage pair came out usable
    closed = cm.place(first, TOL, mc)
    r = closed["root"]
    assert closed["placed"].sum() < C                                       # closure alone does not place the pool
    out = pm.place(L, R, F, r, TOL, mc, 64, 0)
    reached = out["hops"] >= 0
    assert (reached == component(U, r)).all() and (not want_all or reached.all())
    assert out["hops"].max() < 64 and out["hops"].max() >= 3
    err = np.abs(out["offset"] - (p["T"] - p["T"][r]))
    assert (err[reached] <= out["hops"][reached]).all(), (err, out["hops"])
    true_pair = U & (np.abs(L - p["true_lag"]) <= 1) & reached[:, None] & reached[None, :]
    assert true_pair.sum() >= C - 1 and (out["state"][true_pair] == 1).all()
    for sweeps in (1, 3):
        swept = pm.place(L, R, F, r, TOL, mc, 64, sweeps)
        assert (swept["hops"] == out["hops"]).all()
        err = np.abs(swept["offset"] - (p["T"] - p["T"][r]))
        assert (err[reached] <= out["hops"].max()).all(), (sweeps, err)
        assert (swept["state"][true_pair] == 1).all()
    return out


@pytest.mark.parametrize("mc", [1, 2])
@pytest.mark.parametrize("C", sorted(BANDS))
def test_band_tables_are_placed_within_a_frame_per_hop(C, mc):
    p, first = band_case(C)
    out = check_band(p, first, mc)
    print(C, mc, "hops", out["hops"].tolist())


@pytest.mark.parametrize("C,spacing", [(65, 40000), (70, 40000), (300, 12000)])
def test_the_masked_band_tables_of_the_device_tests(C, spacing):
    """... and at C = 300 the spacing is one at which the model needs fewer than 64 hops, from closure's root and from clip C - 1"""
    p, first = band_case(C, True, spacing)
    for mc in (1, 2):
        out = check_band(p, first, mc)
        corner = pm.place(*tables(first), C - 1, TOL, mc, 64, 0)
        assert (corner["hops"] >= 0).all() and corner["hops"].max() < 64
        print(C, mc, "depth", int(out["hops"].max()), "from the corner", int(corner["hops"].max()))


def test_garbage_that_closes_a_triangle_by_accident_carries_a_clip_away():
    """the second finding: a property of the input, which the verdicts show"""
    p, first = band_case(12, k=3, seed=2)
    L, R, F = tables(first)
    U = pm.usable_pairs(L, R, F, 1)
    assert int((U & ~p["in_band"]).sum()) == 2
    r = cm.place(first, TOL, 1)["root"]
    out = pm.place(L, R, F, r, TOL, 1)
    err = np.abs(out["offset"] - (p["T"] - p["T"][r]))
    assert err.max() > 100000
    assert (out["state"] == 2).any() and (out["support"] < out["degree"]).any()
    assert not (pm.usable_pairs(L, R, F, 2) & ~p["in_band"]).any()          # a larger min_confirm masks them here
    check_band(p, first, 2)


# ---- (c) dense pools: every pair computed, a few picks wrong ----------------------------------------------------------------------------
DENSE = [(5, 8), (9, 4), (65, 3)]


@functools.lru_cache(maxsize=None)
def dense_case(C, k):
    p = cm.planted(C, k, 11 + C, bad_pairs=3)
    return p, cm.picked(p["lag"], p["coef"], p["ret"], TOL)


@pytest.mark.parametrize("C,k", DENSE)
def test_dense_pools_get_a_verdict_per_pair(C, k):
    p, first = dense_case(C, k)
    L, R, F = tables(first)
    r = cm.place(first, TOL, 0)["root"]
    off = ~np.eye(C, dtype=bool)
    for sweeps in (0, 2):
        out = pm.place(L, R, F, r, TOL, 0, 64, sweeps)
        assert (out["hops"] >= 0).all() and out["hops"].max() <= 2
        assert (np.abs(out["offset"] - (p["T"] - p["T"][r])) <= 1).all()
        usable = pm.usable_pairs(L, R, F, 0)
        right = usable & (np.abs(L - p["true_lag"]) <= 1)
        wrong = usable & ~right
        assert wrong.sum() >= 1 and right.sum() >= C * (C - 1) - 4
        assert (out["state"][wrong] == 2).all() and (out["state"][right] == 1).all() and (out["state"][~usable] == 0).all()
        assert (np.abs(out["resid"][wrong]) > TOL).all() and (out["state"][~off] == 0).all()


# ---- (d) two components ---------------------------------------------------------------------------------------------------------------
def test_only_the_roots_component_is_reached_and_a_second_call_reaches_the_other():
    p, _ = band_case(24)
    lag, coef, ret, low = pm.cut(p, 10)
    first = cm.picked(lag, coef, ret, TOL)
    L, R, F = tables(first)
    assert low.sum() == 10
    a = int(np.flatnonzero(low)[0])
    out = pm.place(L, R, F, a, TOL, 1)
    assert ((out["hops"] >= 0) == low).all() and (out["offset"][~low] == 0).all() and (out["degree"][~low] == 0).all()
    assert (out["state"][~low] == 0).all() and (out["state"][:, ~low] == 0).all()
    b = int(np.flatnonzero(out["hops"] < 0)[0])
    other = pm.place(L, R, F, b, TOL, 1)
    assert ((other["hops"] >= 0) == ~low).all()
    for o, root, part in ((out, a, low), (other, b, ~low)):
        err = np.abs(o["offset"] - (p["T"] - p["T"][root]))
        assert (err[part] <= o["hops"][part]).all()


# ---- (e) further cases ----------------------------------------------------------------------------------------------------------------
def test_a_root_that_is_no_clip_reaches_nothing():
    L, R, F = pm.chain(4)
    for root in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        out = pm.place(L, R, F, root, 0, 0, 64, 2)
        assert out["hops"].tolist() == [-1] * 4 and not out["state"].any()
        assert not any(out[n].any() for n in ("offset", "support", "degree", "step", "resid"))


def test_one_clip():
    L, R, F = pm.chain(1)
    out = pm.place(L, R, F, 0, 0, 0, 1, 1)
    assert {n: v.reshape(-1).tolist() for n, v in out.items()} == dict(offset=[0], hops=[0], support=[0], degree=[0], step=[0], resid=[0],
                                                                       state=[0])


def median_tables():
    """clip 3 hangs on the clips 1 and 2 of layer 1, over four pairs: E_3 = {10 + 30, 20 + 24, 10 + 32, 20 + 26} = {40, 42, 44, 46}"""
    L = np.zeros((4, 4), dtype=np.int64)
    R = np.full((4, 4), -3, dtype=np.int32)
    for (a, b), l in {(0, 1): 10, (0, 2): 20, (1, 3): 30, (2, 3): 24, (3, 1): -32, (3, 2): -26}.items():
        L[a, b], R[a, b] = l, 0
    return L, R, np.zeros((4, 4), dtype=np.int32)


def test_the_lower_median_of_an_even_count():
    out = pm.place(*median_tables(), 0, 2, 0)
    assert out["hops"].tolist() == [0, 1, 1, 2] and out["offset"].tolist() == [0, 10, 20, 42]
    assert out["degree"].tolist() == [2, 3, 3, 4] and out["support"].tolist() == [2, 3, 2, 3]
    assert out["resid"][1, 3] == -2 and out["resid"][2, 3] == 2 and out["resid"][3, 1] == 0 and out["resid"][3, 2] == -4
    assert out["state"][3, 2] == 2 and out["state"][2, 3] == 1


def step_tables():
    """a chain 0 - 1 - 2 - 3 and a pair (1, 3) that says 230 where the chain says 200: layer 2 places clip 3 from clip 1 alone, at
    330; the first sweep sees clip 2 as well, E_3 = {300, 330}, and nothing moves after it"""
    L, R, F = pm.chain(4)
    L[1, 3], R[1, 3] = 230, 0
    return L, R, F


def test_the_step_is_not_zero_while_a_sweep_moves_something_and_zero_at_a_fixed_point():
    t = step_tables()
    assert pm.place(*t, 0, 0, 0)["offset"].tolist() == [0, 100, 200, 330] and not pm.place(*t, 0, 0, 0)["step"].any()
    steps = [pm.place(*t, 0, 0, 0, 64, s) for s in range(1, 4)]
    assert steps[0]["step"].tolist() == [0, 0, 0, -30] and steps[0]["offset"].tolist() == [0, 100, 200, 300]
    assert not steps[1]["step"].any() and not steps[2]["step"].any()
    assert steps[1]["offset"].tolist() == steps[2]["offset"].tolist() == [0, 100, 200, 300]
    assert all(s["offset"][0] == 0 and s["hops"].tolist() == [0, 1, 2, 2] for s in steps)


def hand_cases():
    """the hand-written tables above as (name, (L, R, F), root, tolerance, min_confirm, max_hops, sweeps), for the device"""
    out = []
    for C in (1, 2, 4):
        out.append(("chain of %d" % C, pm.chain(C), 0, 0, 0, 64, 0))
        out.append(("chain of %d backwards, swept" % C, pm.chain(C), C - 1, 0, 0, 64, 1))
    out.append(("chain cut short", pm.chain(4), 0, 0, 0, 2, 0))
    out.append(("one hop of a chain", pm.chain(4), 1, 0, 0, 1, 3))
    out.append(("nothing usable", pm.chain(4), 0, 0, 1, 64, 1))
    for root in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        out.append(("root %d" % root, pm.chain(4), root, 0, 0, 64, 2))
    out.append(("the lower median", median_tables(), 0, 2, 0, 64, 0))
    for s in range(0, 4):
        out.append(("%d sweeps" % s, step_tables(), 0, 0, 0, 64, s))
    big = pm.chain(3, pm.LAG_MAX)                                           # the largest lags, and the largest tolerance
    out.append(("lags of 2^40", big, 0, 0, 0, 1024, 64))
    out.append(("tolerance 2^40", big, 2, pm.LAG_MAX, 0, 64, 1))
    return out


def test_the_hand_tables_for_the_device_say_what_the_tests_above_say():
    cases = {name: pm.place(*t, root, tol, mc, mh, sw) for name, t, root, tol, mc, mh, sw in hand_cases()}
    assert len(cases) == len(hand_cases())
    assert cases["chain of 4"]["hops"].tolist() == [0, 1, 2, 3] and cases["chain cut short"]["hops"].tolist() == [0, 1, 2, -1]
    assert cases["one hop of a chain"]["hops"].tolist() == [1, 0, 1, -1] and cases["nothing usable"]["hops"].tolist() == [0, -1, -1, -1]
    assert cases["the lower median"]["offset"].tolist() == [0, 10, 20, 42]
    assert cases["1 sweeps"]["step"].tolist() == [0, 0, 0, -30] and not cases["3 sweeps"]["step"].any()
    assert cases["lags of 2^40"]["offset"].tolist() == [0, 1 << 40, 2 << 40]
    assert cases["tolerance 2^40"]["offset"].tolist() == [-2 << 40, -1 << 40, 0]


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()


def test_the_call_is_declared_listed_and_exported():
    hdr = header()
    m = asx()
    from audiosync_amd import hipxcorr
    assert re.search(r"\bint %s\s*\(" % CALL, hdr)
    assert CALL in hipxcorr.ABI_SYMBOLS and CALL in hipxcorr.SIGNATURES
    restype, args = hipxcorr.SIGNATURES[CALL]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int and len(args) == 18
    assert args == [vp, vp, vp, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int] + [vp] * 9
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    assert hasattr(L, CALL)                                                # (fails without the feature)
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name, value in (("ASX_PLACE_HOPS_MAX", pm.HOPS_MAX), ("ASX_PLACE_SWEEPS_MAX", pm.SWEEPS_MAX)):
        d = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, hdr, flags=re.M)
        assert d and int(d.group(1)) == value == getattr(hipxcorr, name[4:]) == getattr(m, name[4:]), name
    assert pm.LAG_MAX == hipxcorr.CLOSURE_LAG_MAX
    assert hdr.index("int asx_pool_closure_dev") < hdr.index("int " + CALL)
    for name in ("pool_place_dev", "pool_place", "place_args"):
        assert callable(getattr(m, name)) and callable(getattr(hipxcorr, name)), name


def test_the_header_states_the_rule():
    flat = re.sub(r"[\s*]+", " ", header())
    at = flat.index("Every clip that a chain of usable pairs reaches")
    text = flat[at:flat.index("int " + CALL, at)]
    for phrase in ("closure's d_best_lag, d_best_ret, d_confirm", "in DEVICE memory", "a replayed graph follows a root that changed",
                   "int64 sums and integer counts", "no output depends on the launch geometry", "exactly as in asx_pool_closure_dev",
                   "x != y, ret == 0, |lag| <= ASX_CLOSURE_LAG_MAX", "confirm[x * C + y] >= min_confirm", "r = d_root[0]",
                   "outside [0, C), no clip is reached", "every hops is -1, every state is 0 and everything else is 0",
                   "hops[r] = 0 and offset[r] = 0", "For h = 1 .. max_hops", "o[c] + L_cb", "o[c] - L_bc", "0 <= hops[c] < h",
                   "the lower median of E_b", "(|E_b| - 1) / 2", "all lie in layer h - 1", "not a spanning tree",
                   "hops -1, offset 0, support 0, degree 0 and step 0", "Jacobi median relaxation", "every clip b with hops > 0",
                   "over ALL reached c", "the root stays 0", "d_step[b] = o_s[b] - o_{s-1}[b] of the last sweep", "a fixed point",
                   "(max_hops + sweeps) * 2^40 < 2^52", "about one frame per hop", "no sweep shrinks that",
                   "by the largest hops of the pool", "d_degree[b] = |E_b| over ALL reached neighbours", "within tolerance of o[b]",
                   "d_resid = L_ab - (o[b] - o[a])", "d_state = 1 if |resid| <= tolerance, 2 if not", "the diagonal included: state 0, resid 0",
                   "close triangles by accident", "Mask the pairs you do not believe", "a larger min_confirm",
                   "nothing launched and the outputs untouched", "other than d_scratch when sweeps == 0", "nclips == 0",
                   "nclips * nclips > INT32_MAX", "tolerance < 0 or > ASX_CLOSURE_LAG_MAX", "min_confirm < 0",
                   "max_hops outside [1, ASX_PLACE_HOPS_MAX]", "sweeps outside [0, ASX_PLACE_SWEEPS_MAX]", "nclips == 1 is legal",
                   "takes no plan", "allocates nothing", "never synchronises the host", "capturable", "2 + max_hops + sweeps kernel launches",
                   "none of which waits for another block", "they may be dirty", "must not alias", "Not offered",
                   "components other than the root's", "weighting by coefficient", "least-squares"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase


def test_the_documents_name_the_call():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "asx_pool_place_dev(" in doc and "pool_place(" in doc and "d_root" in doc[doc.index("asx_pool_place_dev("):]
    assert "min_confirm" in doc[doc.index("asx_pool_place_dev("):] and "d_state" in doc
    assert CALL in open(os.path.join(ROOT, "README.md")).read()
    assert "k_place_layer" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_host_checks_raise_before_anything_is_uploaded(monkeypatch):
    asx()
    from audiosync_amd import hipxcorr

    def no_device(*a, **kw):
        raise AssertionError("reached the library")

    L, R, F = median_tables()
    good = dict(best_lag=L, best_ret=R, confirm=F, root=0, tolerance=2, min_confirm=1, max_hops=64, sweeps=0)
    bad = [dict(best_lag=L[:3]), dict(best_lag=L[:, :3]), dict(best_ret=R[:3, :3]), dict(confirm=F.reshape(-1)), dict(best_lag=L[None]),
           dict(best_lag=L.astype(np.float64)), dict(best_ret=R.astype(np.float32)), dict(confirm=F > 0), dict(best_lag=L > 0),
           dict(best_lag=np.zeros((0, 0), np.int64), best_ret=np.zeros((0, 0), np.int32), confirm=np.zeros((0, 0), np.int32)),
           dict(best_ret=R.astype(np.int64) + (1 << 40)), dict(confirm=F.astype(np.int64) - (1 << 40)),
           dict(best_lag=np.full((4, 4), 2 ** 63, dtype=np.uint64)),
           dict(root=True), dict(root=0.0), dict(root=None), dict(root=2 ** 31), dict(root=-2 ** 31 - 1),
           dict(tolerance=True), dict(tolerance=2.0), dict(tolerance=-1), dict(tolerance=(1 << 40) + 1),
           dict(min_confirm=False), dict(min_confirm=1.0), dict(min_confirm=-1),
           dict(max_hops=True), dict(max_hops=0), dict(max_hops=1025), dict(max_hops=64.0),
           dict(sweeps=False), dict(sweeps=-1), dict(sweeps=65), dict(sweeps=1.0)]
    monkeypatch.setattr(hipxcorr, "lib", no_device)
    monkeypatch.setattr(hipxcorr, "_Staging", no_device)
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.pool_place(**args)
        with pytest.raises(ValueError):
            hipxcorr.place_args(**args)
    with pytest.raises(AssertionError):                                    # the stand-in does catch a call that gets through
        hipxcorr.pool_place(**good)
    got = hipxcorr.place_args(L.astype(np.int32), R.astype(np.int64), F.astype(np.uint8), np.int64(7), np.int64(1 << 40), np.int32(0),
                              np.int64(1024), np.int32(64))
    assert got[3:] == (4, 7, 1 << 40, 0, 1024, 64) and all(type(v) is int for v in got[3:])
    assert [a.dtype for a in got[:3]] == [np.int64, np.int32, np.int32] and all(a.flags["C_CONTIGUOUS"] for a in got[:3])
    assert got[0].tobytes() == L.tobytes() and got[1].tobytes() == R.tobytes()
    assert hipxcorr.place_args(L, R, F, -1, 0)[4:] == (-1, 0, 1, 64, 0)     # a root that is no clip is legal


# ---- the premise of the end-to-end test, by the references alone ------------------------------------------------------------------------
E2E_N, E2E_C, E2E_K, E2E_SEP, E2E_TOL = 144000, 6, 2, 1000, 2
E2E_OVERLAP = E2E_N // 8       # min_overlap: a neighbour behind a clip overlaps its first N frames by 0.2 N less the noise of the offsets


@functools.lru_cache(maxsize=None)
def e2e_offsets():
    rng = np.random.default_rng(20263)
    return tuple(int(v) for v in (E2E_N * 8 // 10) * np.arange(E2E_C) + rng.integers(-3000, 3001, size=E2E_C))


@functools.lru_cache(maxsize=None)
def e2e_clips():
    """six clips of 2N frames cut from one noise recording about 0.8 N apart: only neighbours share frames that a pair sees"""
    o = e2e_offsets()
    rec = np.random.default_rng(20264).standard_normal(max(o) - min(o) + 2 * E2E_N).astype(np.float32)
    clips = np.stack([rec[v - min(o):v - min(o) + 2 * E2E_N] for v in o]).copy()
    clips.setflags(write=False)
    return clips


def e2e_true_lags():
    o = np.array(e2e_offsets(), dtype=np.int64)
    return o[None, :] - o[:, None]


@functools.lru_cache(maxsize=None)
def e2e_reference_tables():
    import ncc_full_model as fm
    clips, C = e2e_clips(), E2E_C
    lag = np.zeros((C, C, E2E_K), dtype=np.int64)
    coef = np.zeros((C, C, E2E_K))
    ret = np.zeros((C, C, E2E_K), dtype=np.int32)
    for a in range(C):
        for b in range(C):
            for j, (r, l, c, _) in enumerate(fm.topk(clips[a], clips[b, :E2E_N], E2E_K, E2E_SEP, min_overlap=E2E_OVERLAP)):
                lag[a, b, j], coef[a, b, j], ret[a, b, j] = l, c, r
    return lag, coef, ret


def check_e2e(lag, ret, closed, placed):
    """tables of the six clips (the model's or the device's), closure's outputs for them at min_confirm 1 and placement's: the premise
    and the result"""
    C, true = E2E_C, e2e_true_lags()
    near = np.abs(np.arange(C)[None, :] - np.arange(C)[:, None]) == 1
    for a, b in np.argwhere(near):
        assert true[a, b] in lag[a, b][ret[a, b] == 0].tolist(), (a, b, lag[a, b], true[a, b])
    U = pm.usable_pairs(closed["best_lag"], closed["best_ret"], closed["confirm"], 1)
    assert (U == near).all()                                                # every neighbour pair, and no other
    assert (closed["best_lag"][near] == true[near]).all()
    r = closed["root"]
    assert 0 in closed["placed"].tolist()                                   # the root and two hops either way at the most
    assert (placed["hops"] == np.abs(np.arange(C) - r)).all()
    o = np.array(e2e_offsets(), dtype=np.int64)
    assert (np.abs(placed["offset"] - (o - o[r])) <= E2E_TOL).all()
    assert (placed["state"][near] == 1).all() and not placed["state"][~near].any() and not placed["step"].any()


def test_the_references_alone_meet_the_premise_of_the_end_to_end_test():
    lag, coef, ret = e2e_reference_tables()
    closed = cm.closure(lag, coef, ret, E2E_TOL, 1)
    check_e2e(lag, ret, closed, pm.place(closed["best_lag"], closed["best_ret"], closed["confirm"], closed["root"], E2E_TOL, 1))


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def test_four_place_kernels_within_their_budget():
    from test_kernel_resources import READELF, demangled, kernels_of
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_place_", n)}
    found = sorted(re.match(r"(?:void )?(k_place_\w+)", n).group(1) for n in mine)
    assert found == ["k_place_init", "k_place_layer", "k_place_sweep", "k_place_verdict"], found
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 64 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] <= 128, (n, r)
