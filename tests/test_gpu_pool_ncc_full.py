"""Full-range normalised cross-correlation over track pools on the MI355X (asx_xcorr_pool_ncc_full_f32_dev,
asx_xcorr_pool_ncc_full_topk_f32_dev): k = 1 and entry 0, every pair bit for bit the strided full-range top-k call on that pair alone
(all combinations, listed pairs with rows, one recording as both pools over more than one group), indices outside a pool, poisoned
surroundings and guarded outputs, growth of the track set, its tables against the exact integer reference, refusals, and fixture F
of tests/ncc_pool_full_model.py through the call and triangle closure.  N = 144 000, real-column plans.  There is no tolerance of
this file's own: every pool value is a strided value bit for bit, so FULL_TOL and TABLE_TOL are the strided tests'."""
import numpy as np
import pytest

import closure_model
import edges
import ncc_exact as ex
import ncc_full_model as fm
import ncc_pool_full_model as pm
import ncc_topk_model as tm
import oracle
from test_gpu_ncc_full import FULL_TOL
from test_gpu_ncc_tables import TABLE_TOL, exact_of, same_tables, tracks
from util import asx

pytestmark = pytest.mark.gpu

N = 144000
SEP = N // 100
MO = (N + 1) // 2
KINDS = ("int64", "float64", "float64", "int32")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pools():
    """3 sources x 4 samples: fixtures D and E of ncc_full_model, fixture C of ncc_topk_model, and a generator sample that belongs to
    none of the sources"""
    def make():
        d, e, c = fm.fixture_d(N, 0), fm.fixture_e(N, 0), tm.fixture_c(N, 0)
        extra = oracle.synth_pair(91, 2, N, 1)
        return np.stack([d[0], e[0], c[0]]), np.stack([d[1], e[1], c[1], extra[1]])
    return cached("pools", make)


def same(a, b):
    return [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]


def entry(out, *index):
    return [np.asarray(a)[index].tobytes() for a in out]


def outputs(torch, count):
    return (torch.zeros(count, dtype=torch.int64, device="cuda"), torch.zeros(count, dtype=torch.float64, device="cuda"),
            torch.zeros(count, dtype=torch.float64, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"))


def call_group(plan):
    """the pairs of one group of the pool full-range calls: the strided full-range set's"""
    return max(1, min(plan.group, (1 << 30) // (72 * plan.sample_len)))


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


def test_k_one_and_entry_zero_are_the_one_lag_pool_call(mod):
    srcs, smps = pools()
    listed = np.array([(0, 0), (1, 1), (2, 2), (1, 3), (0, 1)], dtype=np.int32)
    # entirely negative, straddling zero, inside [0, N-1], not a row of the call, the whole range
    rows = np.array([(-N + 1, -1), (-40000, 50000), (5, N // 2), (7, 3), (-N + 1, N - 1)], dtype=np.int64)
    with mod.Plan(N, 4, 0) as plan:
        assert plan.layout == "real-column"
        for pairs, windows in ((None, None), (listed, None), (listed, rows)):
            want = plan.xcorr_pool_ncc_full_f32(srcs, smps, pairs, windows)
            one = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, 1, SEP, pairs, windows)
            assert same([a[..., 0] for a in one], want)
            four = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, 4, SEP, pairs, windows)
            assert same([a[..., 0] for a in four], want)
        assert want[3].tolist() == [0, 0, 0, -2, 0] and int(want[0][0]) == fm.fixture_d(N, 0)[2] < 0
        assert four[3][3].tolist() == [-2] * 4
        # and the one-lag pool call is the strided full-range call on the materialised pairs
        assert same(plan.xcorr_ncc_full_f32(srcs[listed[:, 0]], smps[listed[:, 1]], rows), want)
        assert same(plan.xcorr_ncc_full_f32(srcs[listed[:, 0]], smps[listed[:, 1]]), plan.xcorr_pool_ncc_full_f32(srcs, smps, listed))


def test_every_pair_is_the_strided_call_on_that_pair_alone(mod):
    srcs, smps = pools()
    k = 4
    listed = np.array([(2, 3), (0, 0), (1, 2), (0, 0), (2, 0), (1, 1), (0, 2), (2, 3)], dtype=np.int32)
    rows = np.array([(-N + 1, N - 1), (-40000, -20000), (-100, N - 100), (-N + 1, 0), (14000, 15000), (-N // 2, N // 2), (1 - N, 1 - N),
                     (3, 2)], dtype=np.int64)
    with mod.Plan(N, 5, 0) as plan:
        alone = {(a, b): plan.xcorr_ncc_full_topk_f32(srcs[a], smps[b], k, SEP) for a in range(3) for b in range(4)}
        got = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP)
        assert all(g.shape == (3, 4, k) for g in got)
        for (a, b), want in alone.items():
            assert entry(got, a, b) == entry(want, 0), (a, b, [g[a, b] for g in got], want)
        # the planted negative lags are found: fixture D's, and fixture E's ahead of its positive one
        assert int(got[0][0, 0, 0]) == fm.fixture_d(N, 0)[2] < 0
        assert got[0][1, 1].tolist()[:2] == list(fm.fixture_e(N, 0)[2]) and got[0][1, 1, 0] < 0
        assert sorted(got[0][2, 2].tolist()[:3]) == sorted(tm.fixture_c(N, 0)[2])
        got = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP, listed, rows)
        for i, (a, b) in enumerate(listed.tolist()):
            want = plan.xcorr_ncc_full_topk_f32(srcs[a], smps[b], k, SEP, rows[i])
            assert entry(got, i) == entry(want, 0), (i, a, b)
        assert got[3][7].tolist() == [-2] * k


def test_one_recording_as_both_pools_over_more_than_one_group(mod, torch):
    """5 source windows and 5 sample windows of one recording, a hop apart: 25 pairs in groups of 16"""
    hop, c, k = 1000, 5, 2
    rng = np.random.default_rng(78)
    rec = np.concatenate([tm.fixture_c(N, 0)[0], rng.standard_normal((c - 1) * hop).astype(np.float32)])
    assert rec.size == (c - 1) * hop + 2 * N and hop % 4 == 0
    d_rec = torch.from_numpy(rec).cuda()
    with mod.Plan(N, 16, 0) as plan:
        g = call_group(plan)
        assert g < c * c < 2 * g and (c * c) % g != 0, (g, c)          # one whole group and a partial one
        want = outputs(torch, c * c * k)
        torch.cuda.synchronize()
        for a in range(c):
            ptrs = [t.data_ptr() + a * c * k * t.element_size() for t in want]
            plan.xcorr_ncc_full_topk_dev(d_rec.data_ptr() + 4 * a * hop, 0, d_rec.data_ptr(), hop, 0, 0, c, 1e-3, MO, k, SEP, *ptrs)
        plan.sync()
        before = plan.debug_ncc(), plan.debug_ncc_full(), plan.debug_bank()
        got = outputs(torch, c * c * k)
        plan.xcorr_pool_ncc_full_topk_dev(d_rec.data_ptr(), hop, c, d_rec.data_ptr(), hop, c, 0, 0, 0, c * c, 1e-3, MO, k, SEP,
                                          *(t.data_ptr() for t in got))
        plan.sync()
        after = plan.debug_ncc(), plan.debug_ncc_full(), plan.debug_bank()
    assert (after[0][2] - before[0][2], after[0][3] - before[0][3]) == (c, c)
    assert (after[1][2] - before[1][2], after[1][3] - before[1][3]) == (c, c) and after[1][:2] == (c, c)
    assert after[2][2] - before[2][2] == 1
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    assert same(got, want), [np.flatnonzero(g != w)[:8] for g, w in zip(got, want)]
    lag = got[0].reshape(c, c, k)
    # sample window b lies in source window a at lag (b - a) hop, whatever its sign: the overlap N - |lag| is far above min_overlap
    assert N - (c - 1) * hop >= MO
    assert all(int(lag[a, b, 0]) == (b - a) * hop for a in range(c) for b in range(c)), lag[:, :, 0]
    assert got[3].tolist() == [0] * (c * c * k)


def test_an_index_outside_its_pool(mod):
    srcs, smps = pools()
    k = 3
    good = np.array([(0, 0), (1, 1), (2, 2), (0, 3), (2, 0), (1, 2)], dtype=np.int32)
    bad = good.copy()
    bad[1], bad[3], bad[4] = (3, 1), (0, -1), (-5, 4)
    rows = np.array([(-N + 1, N - 1), (-N + 1, N - 1), (-N + 1, N - 1), (8, 2), (-72010, -72000), (-N + 1, N - 1)], dtype=np.int64)
    with mod.Plan(N, 4, 0) as plan:
        want = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP, good, rows)
        assert want[3][3].tolist() == [-2] * k and want[3][4].tolist() == [0, -3, -3]
        got = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP, bad, rows)
        for i in (1, 3, 4):                                    # -4 ahead of the -2 of pair 3 and the -3 of pair 4
            assert got[0][i].tolist() == [0] * k and got[3][i].tolist() == [-4] * k, (i, got)
            assert np.isnan(got[1][i]).all() and np.isnan(got[2][i]).all()
        for i in (0, 2, 5):
            assert entry(got, i) == entry(want, i), i
        # the other pairs: bit for bit a call without the bad pairs
        keep = np.array([0, 2, 5])
        less = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP, good[keep], rows[keep])
        assert same([a[keep] for a in got], less)
        one = plan.xcorr_pool_ncc_full_f32(srcs, smps, bad, rows)
        assert one[3].tolist() == [0, -4, 0, -4, -4, 0] and one[0][[1, 3, 4]].tolist() == [0, 0, 0]
        assert np.isnan(one[1][[1, 3, 4]]).all() and np.isnan(one[2][[1, 3, 4]]).all()
        assert same([a[keep] for a in one], [a[keep, 0] for a in want])


@pytest.mark.parametrize("poison", edges.POISONS)
def test_edges(mod, torch, poison):
    """poison in front of, between and behind the tracks of both pools, guards around the outputs: the dense call's results, nothing
    written past batch * k, the pools unchanged"""
    srcs, smps = pools()
    k, batch, front, gap = 2, 12, 4, 4
    with mod.Plan(N, 5, 0) as plan:
        assert call_group(plan) < batch
        want = plan.xcorr_pool_ncc_full_f32(srcs, smps)
        want2 = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP)
        b_src, o_src, s_src = edges.embed(srcs, front, 2 * N + gap, poison, torch)
        b_smp, o_smp, s_smp = edges.embed(smps, front, N + gap, poison, torch, back=2 * N)
        before = edges.snapshot(b_src), edges.snapshot(b_smp)
        p_src, p_smp = b_src.data_ptr() + 4 * o_src, b_smp.data_ptr() + 4 * o_smp
        out = [edges.guarded(torch, kind, batch) for kind in KINDS]
        torch.cuda.synchronize()
        plan.xcorr_pool_ncc_full_dev(p_src, s_src, 3, p_smp, s_smp, 4, 0, 0, 0, batch, 1e-3, MO, *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want]
        assert not any(edges.check_guards(w, batch) for w, _ in out)
        out = [edges.guarded(torch, kind, batch * k) for kind in KINDS]
        torch.cuda.synchronize()
        plan.xcorr_pool_ncc_full_topk_dev(p_src, s_src, 3, p_smp, s_smp, 4, 0, 0, 0, batch, 1e-3, MO, k, SEP,
                                          *(v.data_ptr() for _, v in out))
        plan.sync()
        assert [v.cpu().numpy().tobytes() for _, v in out] == [a.tobytes() for a in want2]
        assert not any(edges.check_guards(w, batch * k) for w, _ in out)
        assert edges.unchanged(b_src, before[0]) and edges.unchanged(b_smp, before[1])


def test_growth(mod):
    """small pools, larger ones, small ones again: the same bits, and the track set grows once and never shrinks"""
    srcs, smps = pools()
    k = 2
    with mod.Plan(N, 4, 0) as plan:
        assert plan.debug_ncc_full() == (0, 0, 0, 0)
        small = plan.xcorr_pool_ncc_full_topk_f32(srcs[:2], smps[:2], k, SEP)
        assert plan.debug_ncc_full() == (2, 2, 2, 2)
        large = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP)
        assert plan.debug_ncc_full() == (3, 4, 5, 6)
        assert same([a[:2, :2] for a in large], small)
        assert same(plan.xcorr_pool_ncc_full_topk_f32(srcs[:2], smps[:2], k, SEP), small)
        assert plan.debug_ncc_full() == (3, 4, 7, 8)
        assert same(plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, k, SEP), large)
        assert plan.debug_ncc_full()[:2] == (3, 4) and plan.debug_bank()[:2] == (3, 4) and plan.debug_ncc()[:2] == (3, 4)
        # more samples than sources, then more sources than samples: each side grows on its own
        plan.xcorr_pool_ncc_full_f32(srcs[:1], np.concatenate([smps, smps[:1]]))
        assert plan.debug_ncc_full()[:2] == (3, 5)


def test_tables(mod):
    """inputs A, B and C of tests/ncc_exact.py (the full-range variants) as the three tracks of both pools: the tables of each track
    against the exact integer reference, a sample track against another pair's source, and the strided full-range call's bits"""
    pairs = [tracks(kind, N, True) for kind in "ABC"]
    srcs, smps = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(N, 3, 0) as plan:
        with pytest.raises(mod.AsxError, match="no such set"):
            plan.debug_ncc_tables("pool_full")
        plan.xcorr_pool_ncc_full_f32(srcs, smps, np.array([(2, 0), (1, 1)], dtype=np.int32))     # every track's tables, whatever the pairs
        got = [plan.debug_ncc_tables("pool_full", t, t) for t in range(3)]
        for t, kind in enumerate("ABC"):
            fig = ex.compare(got[t], exact_of(kind, N, True), relative=kind in "AB")
            print("ncc tables pool_full", kind, N, " ".join("%s %.3g" % kv for kv in sorted(fig.items())))
            assert all(v <= TABLE_TOL for v in fig.values()), (kind, fig)
        mixed = plan.debug_ncc_tables("pool_full", 0, 2)
        assert mixed["vy"] == got[2]["vy"] and mixed["vmax"] == got[0]["vmax"]
        assert mixed["ttab"][1:].tobytes() == got[2]["ttab"][1:].tobytes() and mixed["ptab"][1:].tobytes() == got[0]["ptab"][1:].tobytes()
        for s, t in ((3, 0), (0, 3)):
            with pytest.raises(mod.AsxError, match="outside"):
                plan.debug_ncc_tables("pool_full", s, t)
        for t in range(3):
            plan.xcorr_ncc_full_f32(srcs[t], smps[t])
            assert same_tables(plan.debug_ncc_tables("full"), got[t]), t


def test_refusals(mod, torch):
    srcs, smps = pools()
    k, batch = 2, 12
    d_srcs = torch.from_numpy(np.concatenate([srcs.reshape(-1), srcs[0][:8]])).cuda()
    d_smps = torch.from_numpy(smps.reshape(-1)).cuda()

    def fresh():
        return [edges.guarded(torch, kind, batch * k) for kind in KINDS]

    def untouched(out):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, batch * k) and view.cpu().tolist() == [edges.PAYLOAD] * (batch * k) for whole, view in out)

    def no_set(plan):
        return (plan.debug_ncc_full() == (0, 0, 0, 0) and plan.debug_ncc() == (0, 0, 0, 0) and plan.debug_bank()[:2] == (0, 0)
                and mod.lib().asx_plan_debug_ncc_tables(plan._h, 2, 0, 0, None, None, None, None, None) == -1
                and mod.lib().asx_plan_debug_ncc_tables(plan._h, 3, 0, 0, None, None, None, None, None) == -1)

    ps, pm_ = d_srcs.data_ptr(), d_smps.data_ptr()
    good = dict(srcs=ps, ss=2 * N, ns=3, smps=pm_, ts=N, nt=4, batch=batch, energy=1e-3, overlap=MO, k=k, sep=0, drop=None)
    cases = [("null", dict(drop=1)), ("null", dict(drop=2)), ("null", dict(drop=3)), ("null", dict(srcs=0)), ("null", dict(smps=0)),
             ("16-byte aligned", dict(srcs=ps + 4)), ("multiples of 4", dict(ss=2 * N + 2)), ("multiples of 4", dict(ts=N + 1)),
             ("2\\^31 - 1", dict(ns=2 ** 31)), ("every combination", dict(batch=11)), ("empty pool", dict(ns=0, pairs=True)),
             ("min_overlap", dict(overlap=0)), ("min_overlap", dict(overlap=N + 1)), ("min_overlap", dict(overlap=-3)),
             ("min_energy", dict(energy=0.0)), ("min_energy", dict(energy=2.0)), ("min_energy", dict(energy=float("nan"))),
             ("k = 0", dict(k=0)), ("k = 9", dict(k=mod.hipxcorr.TOPK_MAX + 1)), ("negative", dict(sep=-1))]
    d_pairs = torch.zeros((batch, 2), dtype=torch.int32, device="cuda")
    with mod.Plan(N, 4, 0) as plan:
        for text, change in cases:
            a = dict(good)
            a.update(change)
            pairs = d_pairs.data_ptr() if a.pop("pairs", False) else 0
            out = fresh()
            ptrs = [view.data_ptr() for _, view in out]
            if a["drop"] is not None:
                ptrs[a["drop"]] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_pool_ncc_full_topk_dev(a["srcs"], a["ss"], a["ns"], a["smps"], a["ts"], a["nt"], pairs, 0, 0, a["batch"],
                                                  a["energy"], a["overlap"], a["k"], a["sep"], *ptrs)
            assert untouched(out) and no_set(plan), (text, change)
            if "k = " in text or text == "negative":
                continue
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_pool_ncc_full_dev(a["srcs"], a["ss"], a["ns"], a["smps"], a["ts"], a["nt"], pairs, 0, 0, a["batch"],
                                             a["energy"], a["overlap"], *ptrs)
            assert untouched(out) and no_set(plan), (text, change, "k = 1")
        out = fresh()
        ptrs = [view.data_ptr() for _, view in out]
        L = mod.lib()
        assert L.asx_xcorr_pool_ncc_full_topk_f32_dev(None, ps, 2 * N, 3, pm_, N, 4, None, None, 0, batch, 1e-3, MO, k, 0, *ptrs, None) == -1
        assert L.asx_xcorr_pool_ncc_full_f32_dev(None, ps, 2 * N, 3, pm_, N, 4, None, None, 0, batch, 1e-3, MO, *ptrs, None) == -1
        # batch == 0 returns 0 and nothing is written; no set has been allocated by any of the refused calls
        assert L.asx_xcorr_pool_ncc_full_topk_f32_dev(plan._h, ps, 2 * N, 3, pm_, N, 4, d_pairs.data_ptr(), None, 0, 0, 1e-3, MO, k, 0,
                                                      *ptrs, None) == 0
        assert untouched(out) and no_set(plan)
        # d_lag may be NULL
        plan.xcorr_pool_ncc_full_topk_dev(ps, 2 * N, 3, pm_, N, 4, 0, 0, 0, batch, 1e-3, MO, k, SEP, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, batch * k) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * (batch * k) and out[3][1].cpu().tolist() == [0] * (batch * k)
    with mod.Plan(5000, 2, 0) as packed:
        assert packed.layout == "packed"
        out = fresh()
        with pytest.raises(mod.AsxError, match="real-column"):
            packed.xcorr_pool_ncc_full_topk_dev(ps, 10000, 3, pm_, 5000, 4, 0, 0, 0, batch, 1e-3, 2500, k, 0,
                                                *(view.data_ptr() for _, view in out))
        assert untouched(out) and no_set(packed)


def test_fixture_f_end_to_end(mod):
    """fixture F through the all-pairs call and triangle closure: the device's tables meet the premise the float64 model meets
    (tests/test_pool_ncc_full.py), closure over them is the model's bit for bit, and every clip lands on its offset"""
    srcs, smps = pm.pools()
    model, cv = pm.full_tables(), pm.curves()
    with mod.Plan(N, pm.C * pm.C, 0) as plan:
        lag, coef, peak, ret = plan.xcorr_pool_ncc_full_topk_f32(srcs, smps, pm.K, pm.SEP)
    assert lag.shape == (pm.C, pm.C, pm.K)
    dev = {"lag": lag, "coef": coef, "peak": peak, "ret": ret}
    pm.check_premise(dev)
    worst = 0.0
    for a in range(pm.C):
        for b in range(pm.C):
            for j in range(pm.K):
                if model["peak"][a, b, j] <= 0.1:       # noise entries near the energy threshold may differ in the last bits
                    continue
                assert (int(lag[a, b, j]), int(ret[a, b, j])) == (int(model["lag"][a, b, j]), int(model["ret"][a, b, j])), (a, b, j)
                c = cv[(a, b)]
                scale = float(np.sqrt(c[1][int(lag[a, b, j]) + N - 1] / (c[2] * c[3])))
                err = abs(float(peak[a, b, j]) - float(model["peak"][a, b, j]))
                worst = max(worst, err * scale)
                assert err <= FULL_TOL / scale + 1e-7, (a, b, j, peak[a, b, j], model["peak"][a, b, j])
                assert abs(float(coef[a, b, j]) - float(model["coef"][a, b, j])) < 1e-5, (a, b, j)
    print("fixture F: worst scaled |peak - model|", worst)
    got = mod.pool_closure(lag, coef, ret, pm.TOL, votes=True)
    want = closure_model.closure(lag, coef, ret, pm.TOL)
    for name, value in want.items():
        if name == "root":
            assert got["root"] == value
        else:
            assert np.asarray(got[name]).tobytes() == np.asarray(value).tobytes(), name
    assert np.array_equal(got["best_lag"], pm.true_lags())
    assert got["root"] == 0 and got["offset"].tolist() == list(pm.OFFSETS) and got["placed"].tolist() == [1] * pm.C
    assert got["support"].tolist() == [0, 6, 6, 6]
