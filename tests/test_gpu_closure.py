"""Triangle closure over a clip pool on the MI355X (asx_pool_closure_dev, pool_closure_dev, pool_closure).

Every output -- votes, the picked (lag, coef, ret, entry), confirm, the root, offset, support, placed -- must be bit for bit what
tests/closure_model.py gives: the rule is integer arithmetic and coefficient comparisons, so there is no tolerance anywhere, and a
picked coefficient is compared by its bytes (NaN payloads are copied through).  The shapes are the smallest at which the kernels
can go wrong: both ends of k, a c range past one 64-lane wave with a ragged tail (65, 70), past a 256-thread block, past the
256-clip LDS chunk of the row and past the 16-b tile of a block (300)."""
import functools

import numpy as np
import pytest

import closure_model as cm
from test_closure import E2E_K, E2E_N, E2E_SEP, E2E_TOL, check_e2e, e2e_clips, edge_cases
from util import asx

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 2), (3, 1), (5, 8), (9, 4), (65, 3), (70, 8), (300, 2)]
GUARD = 5
INT_FILL, FLOAT_FILL = -77, 7.5
PER_PAIR = (("best_lag", np.int64), ("best_coef", np.float64), ("best_ret", np.int32), ("best_entry", np.int32),
            ("confirm", np.int32))
PER_CLIP = (("offset", np.int64), ("support", np.int32), ("placed", np.int32))


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    return t


def sizes(C, k):
    s = {name: (C * C, dt) for name, dt in PER_PAIR}
    s.update({name: (C, dt) for name, dt in PER_CLIP})
    s["root"] = (1, np.int32)
    s["votes"] = (C * C * k, np.int32)
    return s


def outputs(torch, C, k):
    """sentinel-filled device outputs, each GUARD elements longer than the call may write"""
    out = {}
    for name, (n, dt) in sizes(C, k).items():
        tdt = {np.int64: torch.int64, np.float64: torch.float64, np.int32: torch.int32}[dt]
        out[name] = torch.full((n + GUARD,), FLOAT_FILL if dt is np.float64 else INT_FILL, dtype=tdt, device="cuda")
    return out


def call(mod, d_in, C, k, tol, mc, root, out, votes=True, stream=0):
    mod.pool_closure_dev(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), C, k, tol, mc, root,
                         out["best_lag"].data_ptr(), out["best_coef"].data_ptr(), out["best_ret"].data_ptr(),
                         out["best_entry"].data_ptr(), out["confirm"].data_ptr(), out["root"].data_ptr(), out["offset"].data_ptr(),
                         out["support"].data_ptr(), out["placed"].data_ptr(), d_votes=out["votes"].data_ptr() if votes else 0,
                         stream=stream)


def fetch(out, C, k, votes=True):
    """the outputs as host arrays in the model's shapes; the guard elements (and all of votes when it was not given) are untouched"""
    got = {}
    for name, (n, dt) in sizes(C, k).items():
        host = out[name].cpu().numpy()
        fill = np.array(FLOAT_FILL if dt is np.float64 else INT_FILL, dtype=dt)
        assert (host[n:] == fill).all(), (name, host[n:])
        if name == "votes" and not votes:
            assert (host == fill).all()
            continue
        got[name] = host[:n]
    got["root"] = int(got["root"][0])
    for name, _ in PER_PAIR:
        got[name] = got[name].reshape(C, C)
    if votes:
        got["votes"] = got["votes"].reshape(C, C, k)
    return got


def upload(torch, lag, coef, ret):
    return [torch.from_numpy(np.ascontiguousarray(lag, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(ret, dtype=np.int32)).cuda()]


def run(mod, torch, lag, coef, ret, tol, mc, root=-1, votes=True):
    C, _, k = lag.shape
    d_in = upload(torch, lag, coef, ret)
    out = outputs(torch, C, k)
    torch.cuda.synchronize()
    call(mod, d_in, C, k, tol, mc, root, out, votes)
    torch.cuda.synchronize()
    return fetch(out, C, k, votes)


def assert_same(got, want, what):
    for name, w in want.items():
        if name not in got:
            continue
        if name == "root":
            assert got[name] == w, (what, name, got[name], w)
            continue
        g = got[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != np.ascontiguousarray(w).tobytes():
            bad = np.argwhere(g.view(np.int64 if g.dtype == np.float64 else g.dtype) != w.view(np.int64 if w.dtype == np.float64 else w.dtype))
            raise AssertionError((what, name, len(bad), bad[:5].tolist(), [g[tuple(i)] for i in bad[:5]], [w[tuple(i)] for i in bad[:5]]))


@functools.lru_cache(maxsize=None)
def table(C, k, decoys):
    p = cm.planted(C, k, 11 + C, period=2400 if decoys == "periodic" else None)
    return p["lag"], p["coef"], p["ret"]


@functools.lru_cache(maxsize=None)
def first(C, k, decoys, tol):
    return cm.picked(*table(C, k, decoys), tol)


@pytest.mark.parametrize("tol", [0, 2])
@pytest.mark.parametrize("decoys", ["random", "periodic"])
@pytest.mark.parametrize("C,k", SHAPES)
def test_every_output_is_the_models_bit_for_bit(mod, torch, C, k, decoys, tol):
    t = table(C, k, decoys)
    for mc in (0, 2):
        want = cm.place(first(C, k, decoys, tol), tol, mc)
        assert_same(run(mod, torch, *t, tol, mc), want, (C, k, decoys, tol, mc))
    root = C - 1                                                            # ... and with a given root
    assert_same(run(mod, torch, *t, tol, 1, root), cm.place(first(C, k, decoys, tol), tol, 1, root), (C, k, decoys, tol, "root"))


@pytest.mark.parametrize("case", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_the_edges_of_the_rule_on_the_device(mod, torch, case):
    """the hand-written tables of tests/test_closure.py: exact ties of votes and finite coefficients, NaN coefficients, lags at and
    past 2^40 under tolerance 0 and 2^40, pairs without a valid entry, the lower median of an even count, three hops"""
    name, t, tol, mc, root = case
    assert_same(run(mod, torch, *t, tol, mc, root), cm.closure(*t, tol, mc, root), name)


@functools.lru_cache(maxsize=None)
def sparse_table():
    """a third of all entries at a ret other than 0, NaN coefficients with a payload among them, a lag past the limit"""
    lag, coef, ret = (a.copy() for a in table(9, 4, "random"))
    rng = np.random.default_rng(99)
    hit = rng.random(ret.shape) < 1.0 / 3.0
    ret[hit] = rng.choice(np.array([-1, -2, -3, -4, 1], dtype=np.int32), size=ret.shape)[hit]
    coef[rng.random(coef.shape) < 0.1] = np.frombuffer(np.uint64(0x7FF80000DEADBEEF).tobytes(), dtype=np.float64)[0]
    lag[2, 5, 1], ret[2, 5, 1] = cm.LAG_MAX + 1, 0
    lag[7, 7] = 0
    ret[3, 4] = -4                                                          # a pair with no valid entry
    return lag, coef, ret


def test_a_third_of_the_entries_not_valid(mod, torch):
    t = sparse_table()
    assert 0.25 < (t[2] != 0).mean() < 0.45
    for tol, mc in ((2, 0), (2, 2), (0, 1)):
        assert_same(run(mod, torch, *t, tol, mc), cm.closure(*t, tol, mc), (tol, mc))


def test_votes_null_and_given_and_a_replayed_graph_give_the_same_bytes(mod, torch):
    C, k, tol, mc = 70, 8, 2, 2
    t = table(C, k, "random")
    want = cm.place(first(C, k, "random", tol), tol, mc)
    assert_same(run(mod, torch, *t, tol, mc, votes=False), want, "votes NULL")
    d_in = upload(torch, *t)
    out = outputs(torch, C, k)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(mod, d_in, C, k, tol, mc, -1, out, True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(fetch(out, C, k), want, "graph")


def test_refusals_leave_the_outputs_untouched(mod, torch):
    C, k = 5, 8
    t = table(C, k, "random")
    d_in = upload(torch, *t)
    out = outputs(torch, C, k)
    torch.cuda.synchronize()
    ptr = {n: v.data_ptr() for n, v in out.items()}
    good = dict(d_lag=d_in[0].data_ptr(), d_coef=d_in[1].data_ptr(), d_ret=d_in[2].data_ptr(), nclips=C, k=k, tolerance=2, min_confirm=1,
                root=-1, d_best_lag=ptr["best_lag"], d_best_coef=ptr["best_coef"], d_best_ret=ptr["best_ret"],
                d_best_entry=ptr["best_entry"], d_confirm=ptr["confirm"], d_root=ptr["root"], d_offset=ptr["offset"],
                d_support=ptr["support"], d_placed=ptr["placed"], d_votes=ptr["votes"])
    bad = [{n: 0} for n in good if n.startswith("d_") and n != "d_votes"]
    bad += [dict(nclips=0), dict(nclips=46341, k=1), dict(nclips=16384, k=8), dict(nclips=2 ** 33), dict(k=0), dict(k=9), dict(tolerance=-1),
            dict(tolerance=(1 << 40) + 1), dict(min_confirm=-1), dict(root=-2), dict(root=C)]
    assert len(bad) == 12 + 11
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(mod.AsxError):
            mod.pool_closure_dev(**args)
    torch.cuda.synchronize()
    for name, (n, dt) in sizes(C, k).items():
        host = out[name].cpu().numpy()
        assert (host == np.array(FLOAT_FILL if dt is np.float64 else INT_FILL, dtype=dt)).all(), name
    mod.pool_closure_dev(**dict(good, tolerance=1 << 40, root=C - 1, d_votes=0))        # the limits themselves are legal
    torch.cuda.synchronize()
    assert int(out["root"].cpu()[0]) == C - 1


def test_the_wrapper_returns_what_the_raw_call_returns(mod, torch):
    t = sparse_table()
    raw = run(mod, torch, *t, 2, 1)
    got = mod.pool_closure(*t, 2, votes=True)
    assert set(got) == set(raw) and isinstance(got["root"], int)
    assert_same(got, raw, "wrapper")
    assert_same(got, cm.closure(*t, 2, 1), "wrapper against the model")
    less = mod.pool_closure(t[0].astype(np.int32), t[1], t[2].astype(np.int64), np.int64(2), min_confirm=0, root=3)
    assert "votes" not in less and less["root"] == 3
    assert_same(less, cm.closure(*t, 2, 0, 3), "wrapper, root 3")


def test_end_to_end_at_144000(mod, torch):
    """four clips of one recording, a private loud event in two pairs: the device's own top-k tables put the decoy first, closure on
    the device equals the model on those tables bit for bit, picks the planted lags and places the clips; the picks go into
    asx_results_to_ms_dev as they stand"""
    n, C, k = E2E_N, 4, E2E_K
    clips = e2e_clips()
    with mod.Plan(n, C * C, 0) as plan:
        dev = plan.xcorr_pool_topk_f32(clips, clips[:, :n], k, E2E_SEP)     # one array as both pools: a sample is a clip's first N frames
    assert dev[0].shape == (C, C, k)
    d_t = upload(torch, *dev)
    out = outputs(torch, C, k)
    ms = torch.full((C * C,), -1, dtype=torch.int64, device="cuda")
    acc = torch.full((C * C,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call(mod, d_t, C, k, E2E_TOL, 1, -1, out)
    mod.results_to_ms_dev(out["best_lag"].data_ptr(), out["best_coef"].data_ptr(), out["best_ret"].data_ptr(), C * C, ms.data_ptr(),
                          acc.data_ptr(), 0.5, 48000.0)
    torch.cuda.synchronize()
    got = fetch(out, C, k)
    assert_same(got, cm.closure(*dev, E2E_TOL, 1), "device tables")
    check_e2e(*dev, got)
    x = got["best_lag"].astype(np.float64) * (1000.0 / 48000.0)
    assert ms.cpu().numpy().tolist() == (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64).reshape(-1).tolist()
    assert acc.cpu().numpy().tolist() == ((got["best_ret"] == 0) & (got["best_coef"] >= 0.5)).astype(np.int32).reshape(-1).tolist()
