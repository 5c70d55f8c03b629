"""Normalised cross-correlation over track pools on the MI355X (asx_xcorr_pool_ncc_f32_dev, asx_xcorr_pool_ncc_topk_f32_dev): k = 1
and entry 0, every pair bit for bit the strided top-k call on that pair alone (all combinations, listed pairs, one recording as both
pools over two NCC groups), indices outside a pool, the moments formed once per track, refusals.  N = 144 000, real-column plans."""
import numpy as np
import pytest

import edges
import ncc_model
import ncc_topk_model as tm
import oracle
from util import asx

pytestmark = pytest.mark.gpu

N = 144000
SEP = N // 100
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pools():
    """3 sources x 4 samples: fixture C (p = 0, 1) and fixture A, and a generator sample that belongs to none of the sources"""
    def make():
        c0, c1, a = tm.fixture_c(N, 0), tm.fixture_c(N, 1), ncc_model.fixture_a(N, 0)
        extra = oracle.synth_pair(91, 2, N, 1)
        return np.stack([c0[0], a[0], c1[0]]), np.stack([c0[1], a[1], c1[1], extra[1]])
    return cached("pools", make)


def same(a, b):
    return [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]


def entry(out, *index):
    return [np.asarray(a)[index].tobytes() for a in out]


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


def test_k_one_and_entry_zero_are_the_pool_call(mod):
    srcs, smps = pools()
    listed = np.array([(2, 1), (0, 0), (2, 2), (0, 3), (1, 1)], dtype=np.int32)
    rows = np.array([(0, N - 1), (70000, 80000), (5, 4), (0, N // 2), (14000, 15000)], dtype=np.int64)
    with mod.Plan(N, 4, 0) as plan:
        assert plan.layout == "real-column"
        for pairs, windows in ((None, None), (listed, None), (listed, rows)):
            want = plan.xcorr_pool_ncc_f32(srcs, smps, pairs, windows)
            one = plan.xcorr_pool_ncc_topk_f32(srcs, smps, 1, SEP, pairs, windows)
            assert same([a[..., 0] for a in one], want)
            four = plan.xcorr_pool_ncc_topk_f32(srcs, smps, 4, SEP, pairs, windows)
            assert same([a[..., 0] for a in four], want)
        assert want[3].tolist() == [0, 0, -2, 0, 0]
        # and the pool call is the strided call on the materialised pairs
        assert same(plan.xcorr_ncc_f32(srcs[listed[:, 0]], smps[listed[:, 1]], rows), want)


def test_every_pair_is_the_strided_call_on_that_pair_alone(mod):
    srcs, smps = pools()
    k = 4
    listed = np.array([(2, 3), (0, 0), (1, 2), (0, 0), (2, 0), (1, 1), (0, 2), (2, 3)], dtype=np.int32)
    rows = np.array([(0, N - 1), (70000, 80000), (100, N - 100), (0, N // 2), (14000, 15000), (0, N - 1), (N - 1, N - 1), (3, 2)],
                    dtype=np.int64)
    with mod.Plan(N, 5, 0) as plan:
        alone = {(a, b): plan.xcorr_ncc_topk_f32(srcs[a], smps[b], k, SEP) for a in range(3) for b in range(4)}
        got = plan.xcorr_pool_ncc_topk_f32(srcs, smps, k, SEP)
        assert all(g.shape == (3, 4, k) for g in got)
        for (a, b), want in alone.items():
            assert entry(got, a, b) == entry(want, 0), (a, b, [g[a, b] for g in got], want)
        # the matched pairs find their copies, the quietest last
        assert got[0][0, 0].tolist()[:3] == list(tm.fixture_c(N, 0)[2]) and got[0][2, 2].tolist()[:3] == list(tm.fixture_c(N, 1)[2])
        assert int(got[0][1, 1, 0]) == ncc_model.fixture_a(N, 0)[2]
        got = plan.xcorr_pool_ncc_topk_f32(srcs, smps, k, SEP, listed, rows)
        for i, (a, b) in enumerate(listed.tolist()):
            want = plan.xcorr_ncc_topk_f32(srcs[a], smps[b], k, SEP, rows[i])
            assert entry(got, i) == entry(want, 0), (i, a, b)
        assert got[3][7].tolist() == [-2] * k


def test_one_recording_as_both_pools_over_two_ncc_groups(mod, torch):
    """18 source windows and 18 sample windows of one recording, a hop apart: 324 pairs, an NCC group being 310"""
    hop, c, k = 1000, 18, 2
    rng = np.random.default_rng(77)
    rec = np.concatenate([tm.fixture_c(N, 0)[0], rng.standard_normal(17 * hop).astype(np.float32)])
    assert rec.size == 17 * hop + 2 * N and hop % 4 == 0
    d_rec = torch.from_numpy(rec).cuda()

    def outputs(count):
        return (torch.zeros(count, dtype=torch.int64, device="cuda"), torch.zeros(count, dtype=torch.float64, device="cuda"),
                torch.zeros(count, dtype=torch.float64, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"))

    with mod.Plan(N, c * c, 0) as plan:
        assert plan.group >= c * c
        want = outputs(c * c * k)
        torch.cuda.synchronize()
        for a in range(c):
            ptrs = [t.data_ptr() + a * c * k * t.element_size() for t in want]
            plan.xcorr_ncc_topk_dev(d_rec.data_ptr() + 4 * a * hop, 0, d_rec.data_ptr(), hop, 0, 0, c, 1e-3, k, SEP, *ptrs)
        plan.sync()
        before = plan.debug_ncc()
        got = outputs(c * c * k)
        plan.xcorr_pool_ncc_topk_dev(d_rec.data_ptr(), hop, c, d_rec.data_ptr(), hop, c, 0, 0, 0, c * c, 1e-3, k, SEP,
                                     *(t.data_ptr() for t in got))
        plan.sync()
        after = plan.debug_ncc()
    assert (after[2] - before[2], after[3] - before[3]) == (c, c)
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    assert same(got, want), [np.flatnonzero(g != w)[:8] for g, w in zip(got, want)]
    lag = got[0].reshape(c, c, k)
    # sample window b lies in source window a at lag (b - a) hop
    assert all(int(lag[a, b, 0]) == (b - a) * hop for a in range(c) for b in range(a, c))
    assert got[3].tolist() == [0] * (c * c * k)


def test_an_index_outside_its_pool(mod):
    srcs, smps = pools()
    k = 3
    good = np.array([(0, 0), (1, 1), (2, 2), (0, 3), (2, 0), (1, 2)], dtype=np.int32)
    bad = good.copy()
    bad[1], bad[3], bad[4] = (3, 1), (0, -1), (-5, 4)
    rows = np.array([(0, N - 1), (0, N - 1), (0, N - 1), (8, 2), (72000, 72010), (0, N - 1)], dtype=np.int64)
    with mod.Plan(N, 4, 0) as plan:
        want = plan.xcorr_pool_ncc_topk_f32(srcs, smps, k, SEP, good, rows)
        assert want[3][3].tolist() == [-2] * k and want[3][4].tolist() == [0, -3, -3]
        got = plan.xcorr_pool_ncc_topk_f32(srcs, smps, k, SEP, bad, rows)
        for i in (1, 3, 4):
            assert got[0][i].tolist() == [0] * k and got[3][i].tolist() == [-4] * k, (i, got)
            assert np.isnan(got[1][i]).all() and np.isnan(got[2][i]).all()
        for i in (0, 2, 5):
            assert entry(got, i) == entry(want, i), i
        one = plan.xcorr_pool_ncc_f32(srcs, smps, bad, rows)
        assert one[3].tolist() == [0, -4, 0, -4, -4, 0] and one[0][[1, 3, 4]].tolist() == [0, 0, 0]
        assert np.isnan(one[1][[1, 3, 4]]).all() and np.isnan(one[2][[1, 3, 4]]).all()
        assert same([a[[0, 2, 5]] for a in one], [a[[0, 2, 5], 0] for a in want])


def test_the_moments_are_formed_once_per_track(mod):
    srcs, smps = pools()
    with mod.Plan(N, 4, 0) as plan:
        assert plan.debug_ncc() == (0, 0, 0, 0)
        seen = plan.debug_ncc()

        def grew(by):
            nonlocal seen
            now = plan.debug_ncc()
            step = (now[2] - seen[2], now[3] - seen[3])
            seen = now
            return step == by

        plan.xcorr_pool_ncc_f32(srcs, smps)                                        # batch = nsources * nsamples
        assert grew((3, 4)) and plan.debug_ncc()[:2] == (3, 4)
        plan.xcorr_pool_ncc_f32(srcs, smps, np.array([(1, 2)], dtype=np.int32))    # batch = 1
        assert grew((3, 4))
        plan.xcorr_pool_ncc_topk_f32(srcs, smps, 4, SEP)
        assert grew((3, 4))
        plan.xcorr_pool_ncc_topk_f32(srcs, smps, 4, SEP, np.array([(0, 0)], dtype=np.int32))
        assert grew((3, 4))
        plan.xcorr_pool_ncc_topk_f32(srcs[:2], smps[:1], 1, 0)                     # smaller pools: the set does not shrink
        assert grew((2, 1)) and plan.debug_ncc()[:2] == (3, 4)
        plan.xcorr_pool_ncc_f32(smps.repeat(2, axis=1)[:, :2 * N], smps[:2])       # more sources: it grows
        assert grew((4, 2)) and plan.debug_ncc()[:2] == (4, 4)
        # the strided forms: a table and a moment set per pair, or one table for a broadcast source
        plan.xcorr_ncc_f32(srcs, smps[:3])
        assert grew((3, 3))
        plan.xcorr_ncc_f32(srcs[0], smps)
        assert grew((1, 4))
        plan.xcorr_ncc_topk_f32(srcs, smps[1], 3, SEP)
        assert grew((3, 1))
        assert plan.debug_bank()[:2] == (4, 4)


def test_refusals(mod, torch):
    srcs, smps = pools()
    k, batch = 2, 12
    d_srcs = torch.from_numpy(np.concatenate([srcs.reshape(-1), srcs[0][:8]])).cuda()
    d_smps = torch.from_numpy(smps.reshape(-1)).cuda()
    kinds = ("int64", "float64", "float64", "int32")

    def outputs():
        return [edges.guarded(torch, kind, batch * k) for kind in kinds]

    def untouched(out):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, batch * k) and view.cpu().tolist() == [edges.PAYLOAD] * (batch * k) for whole, view in out)

    ps, pm = d_srcs.data_ptr(), d_smps.data_ptr()
    good = dict(srcs=ps, ss=2 * N, ns=3, smps=pm, ts=N, nt=4, batch=batch, energy=1e-3, k=k, sep=0, drop=None)
    cases = [("null", dict(drop=1)), ("null", dict(drop=2)), ("null", dict(drop=3)), ("null", dict(srcs=0)), ("null", dict(smps=0)),
             ("16-byte aligned", dict(srcs=ps + 4)), ("multiples of 4", dict(ss=2 * N + 2)), ("multiples of 4", dict(ts=N + 1)),
             ("2\\^31 - 1", dict(ns=2 ** 31)), ("every combination", dict(batch=11)), ("empty pool", dict(ns=0, pairs=True)),
             ("min_energy", dict(energy=0.0)), ("min_energy", dict(energy=2.0)), ("min_energy", dict(energy=float("nan"))),
             ("k = 0", dict(k=0)), ("k = 9", dict(k=9)), ("negative", dict(sep=-1))]
    d_pairs = torch.zeros((batch, 2), dtype=torch.int32, device="cuda")
    with mod.Plan(N, 4, 0) as plan:
        for text, change in cases:
            a = dict(good)
            a.update(change)
            pairs = d_pairs.data_ptr() if a.pop("pairs", False) else 0
            out = outputs()
            ptrs = [view.data_ptr() for _, view in out]
            if a["drop"] is not None:
                ptrs[a["drop"]] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_pool_ncc_topk_dev(a["srcs"], a["ss"], a["ns"], a["smps"], a["ts"], a["nt"], pairs, 0, 0, a["batch"], a["energy"],
                                             a["k"], a["sep"], *ptrs)
            assert untouched(out), (text, change)
            if "k = " in text or text == "negative":
                continue
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_pool_ncc_dev(a["srcs"], a["ss"], a["ns"], a["smps"], a["ts"], a["nt"], pairs, 0, 0, a["batch"], a["energy"], *ptrs)
            assert untouched(out), (text, change, "k = 1")
        out = outputs()
        ptrs = [view.data_ptr() for _, view in out]
        L = mod.lib()
        assert L.asx_xcorr_pool_ncc_topk_f32_dev(None, ps, 2 * N, 3, pm, N, 4, None, None, 0, batch, 1e-3, k, 0, *ptrs, None) == -1
        assert L.asx_xcorr_pool_ncc_f32_dev(None, ps, 2 * N, 3, pm, N, 4, None, None, 0, batch, 1e-3, *ptrs, None) == -1
        # batch == 0 returns 0 and nothing is written; no set has been allocated by any of the refused calls
        assert L.asx_xcorr_pool_ncc_topk_f32_dev(plan._h, ps, 2 * N, 3, pm, N, 4, d_pairs.data_ptr(), None, 0, 0, 1e-3, k, 0, *ptrs, None) == 0
        assert untouched(out) and plan.debug_ncc() == (0, 0, 0, 0) and plan.debug_bank()[:2] == (0, 0)
        # d_lag may be NULL
        plan.xcorr_pool_ncc_topk_dev(ps, 2 * N, 3, pm, N, 4, 0, 0, 0, batch, 1e-3, k, SEP, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, batch * k) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * (batch * k) and out[3][1].cpu().tolist() == [0] * (batch * k)
    with mod.Plan(5000, 2, 0) as packed:
        assert packed.layout == "packed"
        out = outputs()
        with pytest.raises(mod.AsxError, match="real-column"):
            packed.xcorr_pool_ncc_topk_dev(ps, 10000, 3, pm, 5000, 4, 0, 0, 0, batch, 1e-3, k, 0, *(view.data_ptr() for _, view in out))
        assert untouched(out)
