"""Placement over chains of usable pairs on the MI355X (asx_pool_place_dev, pool_place_dev, pool_place).

Every output -- offset, hops, support, degree, step, resid, state -- must be bit for bit what tests/place_model.py gives: the rule is
int64 sums and integer counts, so there is no tolerance anywhere.  Outputs are sentinel-filled and GUARD elements longer than the call
may write.  The shapes are the smallest at which the kernels can go wrong: the smallest pools (1, 2, 4), a clip range past one
64-lane wave with a ragged tail (65, 70) and past a 256-thread block (300), layers cut short by max_hops, both parities of the sweep
count (the result ends in d_offset either way), a root chosen by closure and one forced.  The premises of every table are asserted on
the models alone in tests/test_place.py."""
import functools

import numpy as np
import pytest

import closure_model as cm
import place_model as pm
import test_place as tp
from test_gpu_closure import assert_same, sparse_table
from test_gpu_closure import call as closure_call
from test_gpu_closure import fetch as closure_fetch
from test_gpu_closure import outputs as closure_outputs
from test_gpu_closure import upload as closure_upload
from util import asx

pytestmark = pytest.mark.gpu

GUARD = 5
FILL = -77


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    return t


def sizes(C):
    return {name: (C * C if name in ("resid", "state") else C, dt) for name, dt in pm.OUTPUTS + (("scratch", np.int64),)}


def outputs(torch, C):
    """sentinel-filled device outputs (and the scratch buffer), each GUARD elements longer than the call may write"""
    return {name: torch.full((n + GUARD,), FILL, dtype=torch.int64 if dt is np.int64 else torch.int32, device="cuda")
            for name, (n, dt) in sizes(C).items()}


def upload(torch, L, R, F):
    return [torch.from_numpy(np.ascontiguousarray(L, dtype=np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(R, dtype=np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32)).cuda()]


def call(mod, d_in, C, tol, mc, d_root, max_hops, sweeps, out, scratch=True, stream=0):
    mod.pool_place_dev(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), C, tol, mc, d_root.data_ptr(), max_hops, sweeps,
                       out["offset"].data_ptr(), out["hops"].data_ptr(), out["support"].data_ptr(), out["degree"].data_ptr(),
                       out["step"].data_ptr(), out["resid"].data_ptr(), out["state"].data_ptr(),
                       d_scratch=out["scratch"].data_ptr() if scratch else 0, stream=stream)


def fetch(out, C, scratch_untouched=False):
    """the outputs as host arrays in the model's shapes; the guard elements are untouched"""
    got = {}
    for name, (n, dt) in sizes(C).items():
        host = out[name].cpu().numpy()
        assert (host[n:] == FILL).all(), (name, host[n:])
        if name == "scratch":
            assert not scratch_untouched or (host == FILL).all()
            continue
        got[name] = host[:n].reshape(C, C) if name in ("resid", "state") else host[:n]
    return got


def run(mod, torch, d_in, C, root, tol, mc, max_hops=64, sweeps=0, out=None):
    fresh = out is None                                                     # (then a call without sweeps leaves the scratch buffer alone)
    out = out or outputs(torch, C)
    d_root = torch.tensor([root], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call(mod, d_in, C, tol, mc, d_root, max_hops, sweeps, out)
    torch.cuda.synchronize()
    return fetch(out, C, fresh and sweeps == 0)


@pytest.mark.parametrize("case", tp.hand_cases(), ids=[c[0] for c in tp.hand_cases()])
def test_the_hand_tables_on_the_device(mod, torch, case):
    """the chains of 1, 2 and 4 clips (closure alone leaves the last of four unplaced: tests/test_place.py), roots that are no clip, the
    lower median of an even count, sweeps up to a fixed point, lags and a tolerance of 2^40 under the largest max_hops and sweeps"""
    name, t, root, tol, mc, max_hops, sweeps = case
    C = t[0].shape[0]
    assert_same(run(mod, torch, upload(torch, *t), C, root, tol, mc, max_hops, sweeps), pm.place(*t, root, tol, mc, max_hops, sweeps), name)


# (C, masked, spacing): garbage out of band at 12 and 24, masked above; 300 at the spacing of tests/test_place.py
POOLS = [(12, False, 40000), (24, False, 40000), (65, True, 40000), (70, True, 40000), (300, True, 12000)]


@functools.lru_cache(maxsize=None)
def picked(C, masked, spacing, tol):
    if tol == tp.TOL:
        return tp.band_case(C, masked, spacing)[1]
    p = tp.band_tables(C, masked, spacing)
    return cm.picked(p["lag"], p["coef"], p["ret"], tol)


@pytest.mark.parametrize("tol", [0, 4])
@pytest.mark.parametrize("C,masked,spacing", POOLS)
def test_every_output_is_the_models_bit_for_bit(mod, torch, C, masked, spacing, tol):
    first = picked(C, masked, spacing, tol)
    t = tp.tables(first)
    d_in = upload(torch, *t)
    out = outputs(torch, C)                                                 # one set for all runs: each runs over the last one's bytes
    runs = 0
    for mc in (0, 1, 2):
        closed = cm.place(first, tol, mc)
        if mc > 0 and tol == tp.TOL:
            assert closed["placed"].sum() < C                               # closure alone leaves clips unplaced
        for root in (closed["root"], C - 1):
            depth = int(pm.place(*t, root, tol, mc, 64, 0)["hops"].max())
            assert depth < 64                                               # (0 where nothing is usable: tolerance 0 confirms no jittered pair)
            for max_hops in sorted({max(depth, 1), max(depth - 1, 1), 64}):
                for sweeps in (0, 1, 3):
                    if max_hops == 64 and sweeps == 1:
                        continue                                            # (both parities ran at the model's depth)
                    want = pm.place(*t, root, tol, mc, max_hops, sweeps)
                    assert_same(run(mod, torch, d_in, C, root, tol, mc, max_hops, sweeps, out), want, (C, tol, mc, root, max_hops, sweeps))
                    runs += 1
    assert runs >= 3 * 2 * 5                                                # (max_hops 1 and 64 where the depth is 0 or 1)


@pytest.mark.parametrize("C,k", tp.DENSE)
def test_dense_pools(mod, torch, C, k):
    _, first = tp.dense_case(C, k)
    t = tp.tables(first)
    d_in = upload(torch, *t)
    for mc, root, sweeps in ((0, cm.place(first, tp.TOL, 0)["root"], 0), (0, 0, 2), (1, C - 1, 1)):
        assert_same(run(mod, torch, d_in, C, root, tp.TOL, mc, 64, sweeps), pm.place(*t, root, tp.TOL, mc, 64, sweeps), (C, k, mc, root, sweeps))


def test_a_third_of_the_entries_not_valid_and_a_lag_past_the_limit(mod, torch):
    lag, coef, ret = sparse_table()
    assert 0.25 < (ret != 0).mean() < 0.45
    for tol, mc in ((2, 0), (2, 2), (0, 1)):
        first = cm.picked(lag, coef, ret, tol)
        L = first["best_lag"].copy()
        R = first["best_ret"].copy()
        L[2, 5], R[2, 5] = pm.LAG_MAX + 1, 0                                # picked or not: a lag past the limit is not usable
        L[5, 2], R[5, 2] = -pm.LAG_MAX - 1, 0
        t = (L, R, first["confirm"])
        assert (R != 0).any() and not pm.usable_pairs(*t, 0)[2, 5] and not pm.usable_pairs(*t, 0)[5, 2]
        for root in (0, 5):
            for sweeps in (0, 2):
                assert_same(run(mod, torch, upload(torch, *t), 9, root, tol, mc, 64, sweeps), pm.place(*t, root, tol, mc, 64, sweeps),
                            (tol, mc, root, sweeps))


def closure_then_place(mod, torch, lag, coef, ret, tol, mc, max_hops, sweeps, stream=0):
    """both calls on one stream, closure's d_root handed to place as it is: no host step in between -> (closure's outputs, place's)"""
    C, _, k = lag.shape
    d_t = closure_upload(torch, lag, coef, ret)
    c_out = closure_outputs(torch, C, k)
    p_out = outputs(torch, C)
    torch.cuda.synchronize()

    def both(s):
        closure_call(mod, d_t, C, k, tol, mc, -1, c_out, True, s)
        mod.pool_place_dev(c_out["best_lag"].data_ptr(), c_out["best_ret"].data_ptr(), c_out["confirm"].data_ptr(), C, tol, mc,
                           c_out["root"].data_ptr(), max_hops, sweeps, p_out["offset"].data_ptr(), p_out["hops"].data_ptr(),
                           p_out["support"].data_ptr(), p_out["degree"].data_ptr(), p_out["step"].data_ptr(), p_out["resid"].data_ptr(),
                           p_out["state"].data_ptr(), d_scratch=p_out["scratch"].data_ptr(), stream=s)
    return both, c_out, p_out, d_t


def test_closure_then_place_on_one_stream_and_in_a_replayed_graph_that_follows_the_root(mod, torch):
    C, tol, mc = 24, tp.TOL, 1
    p, first = tp.band_case(C)
    k = p["lag"].shape[2]
    t = tp.tables(first)
    closed = cm.place(first, tol, mc)
    want = pm.place(*t, closed["root"], tol, mc, 64, 3)
    both, c_out, p_out, keep = closure_then_place(mod, torch, p["lag"], p["coef"], p["ret"], tol, mc, 64, 3)
    both(0)
    torch.cuda.synchronize()
    assert_same(closure_fetch(c_out, C, k), closed, "closure")
    assert_same(fetch(p_out, C), want, "place behind closure")
    # place alone in a graph, its root in device memory: the replay follows a root that the host never saw the call with
    d_in = upload(torch, *t)
    d_root = torch.tensor([closed["root"]], dtype=torch.int32, device="cuda")
    out = outputs(torch, C)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(mod, d_in, C, tol, mc, d_root, 64, 3, out, True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(fetch(out, C), want, "graph")
    other = (closed["root"] + 7) % C
    d_root.fill_(other)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(fetch(out, C), pm.place(*t, other, tol, mc, 64, 3), "graph, root overwritten on the device")
    d_root.fill_(C)                                                         # ... and one that is no clip
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(fetch(out, C), pm.place(*t, C, tol, mc, 64, 3), "graph, no root")


def test_a_second_call_over_dirty_outputs_and_a_null_scratch(mod, torch):
    C, tol, mc = 70, tp.TOL, 1
    _, first = tp.band_case(C, True, 40000)
    t = tp.tables(first)
    d_in = upload(torch, *t)
    root = cm.place(first, tol, mc)["root"]
    out = outputs(torch, C)
    a = run(mod, torch, d_in, C, root, tol, mc, 64, 2, out)
    b = run(mod, torch, d_in, C, root, tol, mc, 64, 2, out)                 # over its own results
    assert_same(b, a, "second call")
    c = run(mod, torch, d_in, C, C - 1, tol, mc, 5, 1, out)                 # over another call's
    assert_same(c, pm.place(*t, C - 1, tol, mc, 5, 1), "dirty")
    out = outputs(torch, C)
    d_root = torch.tensor([root], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call(mod, d_in, C, tol, mc, d_root, 64, 0, out, scratch=False)
    torch.cuda.synchronize()
    assert_same(fetch(out, C, True), pm.place(*t, root, tol, mc, 64, 0), "scratch NULL")


def test_refusals_leave_the_outputs_untouched(mod, torch):
    C = 5
    _, first = tp.dense_case(5, 8)
    d_in = upload(torch, *tp.tables(first))
    out = outputs(torch, C)
    d_root = torch.tensor([0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = {n: v.data_ptr() for n, v in out.items()}
    good = dict(d_lag=d_in[0].data_ptr(), d_ret=d_in[1].data_ptr(), d_confirm=d_in[2].data_ptr(), nclips=C, tolerance=2, min_confirm=1,
                d_root=d_root.data_ptr(), max_hops=64, sweeps=1, d_offset=ptr["offset"], d_hops=ptr["hops"], d_support=ptr["support"],
                d_degree=ptr["degree"], d_step=ptr["step"], d_resid=ptr["resid"], d_state=ptr["state"], d_scratch=ptr["scratch"])
    bad = [{n: 0} for n in good if n.startswith("d_")]
    bad += [dict(nclips=0), dict(nclips=46341), dict(nclips=2 ** 33), dict(tolerance=-1), dict(tolerance=(1 << 40) + 1), dict(min_confirm=-1),
            dict(max_hops=0), dict(max_hops=-1), dict(max_hops=1025), dict(sweeps=-1), dict(sweeps=65)]
    assert len(bad) == 12 + 11
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(mod.AsxError):
            mod.pool_place_dev(**args)
    torch.cuda.synchronize()
    for name in sizes(C):
        assert (out[name].cpu().numpy() == FILL).all(), name
    mod.pool_place_dev(**dict(good, tolerance=1 << 40, max_hops=1024, sweeps=0, d_scratch=0))       # the limits themselves are legal
    torch.cuda.synchronize()
    want = pm.place(*tp.tables(first), 0, 1 << 40, 1, 1024, 0)
    assert (out["scratch"].cpu().numpy() == FILL).all() and want["hops"].max() >= 1
    assert_same(fetch(out, C, True), want, "the limits")


def test_the_wrapper_returns_what_the_raw_call_returns(mod, torch):
    _, first = tp.dense_case(9, 4)
    t = tp.tables(first)
    for sweeps in (0, 3):
        raw = run(mod, torch, upload(torch, *t), 9, 4, 2, 1, 64, sweeps)
        got = mod.pool_place(*t, 4, 2, sweeps=sweeps)
        assert set(got) == set(raw) == {n for n, _ in pm.OUTPUTS}
        assert_same(got, raw, "wrapper")
        assert_same(got, pm.place(*t, 4, 2, 1, 64, sweeps), "wrapper against the model")
    less = mod.pool_place(t[0].astype(np.int32), t[1].astype(np.int64), t[2].astype(np.int64), np.int64(-1), np.int64(0), min_confirm=0,
                          max_hops=1)
    assert_same(less, pm.place(*t, -1, 0, 0, 1, 0), "wrapper, no root")


def test_end_to_end_at_144000(mod, torch):
    """six clips about 0.8 N apart, so that only neighbours overlap: the device's own full-range NCC top-k tables go through closure
    and then placement, both on the device with no host step in between; closure alone leaves clips unplaced, placement reaches all
    six at their offsets, and both equal their models on those tables bit for bit"""
    n, C, k = tp.E2E_N, tp.E2E_C, tp.E2E_K
    clips = tp.e2e_clips()
    with mod.Plan(n, C * C, 0) as plan:
        lag, coef, _, ret = plan.xcorr_pool_ncc_full_topk_f32(clips, clips[:, :n], k, tp.E2E_SEP, min_overlap=tp.E2E_OVERLAP)
    assert lag.shape == (C, C, k)
    both, c_out, p_out, keep = closure_then_place(mod, torch, lag, coef, ret, tp.E2E_TOL, 1, 64, 0)
    both(0)
    torch.cuda.synchronize()
    closed, placed = closure_fetch(c_out, C, k), fetch(p_out, C)
    want = cm.closure(lag, coef, ret, tp.E2E_TOL, 1)
    assert_same(closed, want, "closure on the device's tables")
    assert_same(placed, pm.place(want["best_lag"], want["best_ret"], want["confirm"], want["root"], tp.E2E_TOL, 1), "place")
    tp.check_e2e(lag, ret, closed, placed)
