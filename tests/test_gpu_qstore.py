"""Partial storing of Q in the pruned inverse pass (asx_plan_set_qstore, include/audiosync/xcorr_hip.h; csrc/rlayout.hip: k_rows_rm,
k_q_predict, the exact check in k_prune_select, the second run in asx_api.hip: resolve_overflows) against the SAME PLAN with the
switch off: lag, coefficient and ret bit for bit, the Pearson-mode and overflow counters equal, and all three results equal to the
unpruned pass's as well.  asx_plan_qstore_stats says which way each pair went: a list, everything, or a second run.

N = 960 000 is the smallest length with a two-half row kernel (the only row schedule with a k_rows_rm instance); mode 2 lets groups of
a few pairs in.  The comb pair is built so that the prediction is WRONG: in the rows the prediction looks at, the sample's spectrum
carries the source at another delay than everywhere else (tests/test_qstore_model.py: comb_pair; checked on the CPU with
tests/model_fourstep.py)."""
import numpy as np
import pytest

import oracle
from util import asx

SEED = 20260101
T = 16
R0 = 8          # predictor rows of mode 2
N = 960000
M2 = 2400
COEF_TOL = 1e-5

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, what):
    for x, y, name in zip(a, b, ("lag", "coef", "ret")):
        assert np.array_equal(bits(x), bits(y)), (what, name, x, y)


def minus(a, b):
    return tuple(int(x) - int(y) for x, y in zip(a, b))


def three_ways(mod, src, smp, host=False, group=None):
    """the same pairs with partial storing (mode 2), without (mode 0) and through the unpruned pass, on one plan ->
    ((lag, coef, ret) of mode 2, what asx_plan_qstore_stats counted for it)"""
    src = np.ascontiguousarray(src, dtype=np.float32)
    smp = np.ascontiguousarray(smp, dtype=np.float32)
    b, n = smp.shape
    with mod.Plan(n, group or b, 0) as plan:
        assert plan.layout == "real-column" and plan.split[1:] == (M2, T)
        if host:
            call = lambda: plan.xcorr_batch_f32(src, smp)
        else:
            call = lambda: plan._strided_f32(src.reshape(-1), 2 * n, smp.reshape(-1), n, b)
        counters = lambda: (plan.pearson_modes(), (plan.peak_overflows(),), plan.qstore_stats())
        plan.set_qstore(2)
        c0 = counters()
        on = call()
        c1 = counters()
        plan.set_qstore(0)
        off = call()
        c2 = counters()
        plan.set_prune(False)
        unpruned = call()
    stats = minus(c1[2], c0[2])
    print("qstore stats (list, all, redone, tiles stored):", stats)
    assert c2[2] == c1[2], "mode 0 counts nothing"
    assert stats[0] + stats[1] == b, stats
    same(on, off, "mode 2 against mode 0")
    same(on, unpruned, "mode 2 against the unpruned pass")
    assert minus(c1[0], c0[0]) == minus(c2[0], c1[0]), ("Pearson modes", c0[0], c1[0], c2[0])
    assert minus(c1[1], c0[1]) == minus(c2[1], c1[1]), ("peak overflows", c0[1], c1[1], c2[1])
    return on, stats


def tile_of(lag, n, m2=M2):
    return ((lag % (2 * n)) % m2) // T


def generator(n, pairs, shift):
    g = [oracle.synth_pair(SEED, p, n, shift) for p in pairs]
    return np.stack([x[0] for x in g]), np.stack([x[1] for x in g]), [x[2] for x in g]


def planted(n, delay, seed):
    """noise, and the same noise from `delay` on plus as much noise again"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n)
    return src.astype(np.float32), (src[delay:delay + n] + rng.standard_normal(n)).astype(np.float32)


def unrelated(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(2 * n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def predictor_rows(n):
    m1 = n // M2
    return m1, m1 // 3


def model_prediction(src, smp, c):
    """tests/test_qstore_model.py: predict, on the float64 model's Q -> (the list or None, p / median)"""
    from test_qstore_model import predict, q_model
    n = len(smp)
    m1, a = predictor_rows(n)
    return predict(q_model(src, smp, m1, M2), a, R0, c)


@pytest.fixture(scope="module")
def comb():
    """(source, sample, true delay, decoy delay) at N; asserted to be what it claims on the CPU"""
    from test_qstore_model import comb_pair, qstore_c
    d_true, d_decoy = 123456, 300700
    m1, a = predictor_rows(N)
    src, smp = comb_pair(N, m1, a, R0, d_true, d_decoy, 77)
    listed, ratio = model_prediction(src, smp, qstore_c())
    t_true, t_decoy = tile_of(d_true, N), tile_of(d_decoy, N)
    print("comb pair: list %s, true tile %d at %.2f medians, decoy tile %d at %.2f" % (listed, t_true, ratio[t_true], t_decoy, ratio[t_decoy]))
    assert t_true != t_decoy and listed is not None and t_decoy in listed and t_true not in listed
    return src, smp, d_true, d_decoy


@gpu
@pytest.mark.parametrize("shift", [0, 1])
def test_generator_pairs_get_a_list_and_none_runs_again(mod, shift):
    src, smp, lags = generator(N, range(6), shift)
    on, stats = three_ways(mod, src, smp)
    assert [int(v) for v in on[0]] == lags
    # (a peak in tile 0, which is always stored, need not stand out of the other tiles: such a pair may store everything)
    away = sum(1 for l in lags if tile_of(l, N) != 0)
    assert stats[0] >= away and stats[2] == 0 and stats[3] <= 4 * stats[0] + (M2 // T) * stats[1], stats


@gpu
def test_headline_length(mod):
    src, smp, lags = generator(1440000, (0, 8, 64, 3), 1)
    on, stats = three_ways(mod, src, smp)
    assert [int(v) for v in on[0]] == lags
    assert all(tile_of(l, 1440000) != 0 for l in lags)
    assert stats[0] == 4 and stats[1] == 0 and stats[2] == 0 and stats[3] <= 4 * 4, stats


@gpu
def test_unrelated_tracks_store_everything(mod):
    pairs = [unrelated(N, 500 + i) for i in range(6)]
    on, stats = three_ways(mod, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    assert stats == (0, 6, 0, 6 * (M2 // T)), stats


@gpu
def test_planted_peaks_in_the_first_tile_the_last_tile_and_at_a_tile_edge(mod):
    delays = [7 * M2 + 5, 11 * M2 + 149 * T + 9, 13 * M2 + 37 * T + 15, 17 * M2 + 38 * T]
    pairs = [planted(N, d, 600 + i) for i, d in enumerate(delays)]
    on, stats = three_ways(mod, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    assert [int(v) for v in on[0]] == delays
    assert stats[0] == 4 and stats[1] == 0 and stats[2] == 0 and stats[3] <= 4 * 4, stats


@gpu
def test_special_inputs(mod):
    """a pure tone (its near-tie list overflows: the ordinary second look), a DC offset in both tracks, a silent track, a NaN, and
    tracks so quiet that every energy underflows and every bound is +infinity"""
    i = np.arange(2 * N, dtype=np.float64)
    g = oracle.synth_pair(SEED, 5, N, 1)
    off = 2.0 * float(np.std(g[0]))
    nan_src = g[0].copy()
    nan_src[1234] = np.nan
    pairs = [
        (np.sin(0.31 * i), np.sin(0.31 * i[:N] + 0.4)),
        (g[0].astype(np.float64) + off, g[1].astype(np.float64) + off),
        (g[0], np.zeros(N)),
        (nan_src, g[1]),
        (g[0].astype(np.float64) * 1e-16, g[1].astype(np.float64) * 1e-16),
    ]
    on, stats = three_ways(mod, np.stack([p[0] for p in pairs]).astype(np.float32), np.stack([p[1] for p in pairs]).astype(np.float32))
    assert int(on[0][4]) == g[2]
    assert stats[1] >= 3, stats  # the silent, the NaN and the underflowing pair have no tile that stands out


@gpu
def test_the_comb_pair_runs_again(mod, comb):
    src, smp, d_true, d_decoy = comb
    on, stats = three_ways(mod, src[None], smp[None])
    assert stats == (1, 0, 1, stats[3]) and stats[3] <= 4, stats
    o_ret, o_lag, o_coef = oracle.cross_correlation(src, smp)
    assert o_lag == d_true and int(on[0][0]) == o_lag and int(on[2][0]) == o_ret
    assert abs(float(on[1][0]) - o_coef) < COEF_TOL, (float(on[1][0]), o_coef)


def mixed_group(comb):
    g = oracle.synth_pair(SEED, 9, N, 1)
    u = unrelated(N, 901)
    return [(g[0], g[1]), u, (comb[0], comb[1]), (g[0], np.zeros(N, dtype=np.float32))]


@gpu
def test_a_group_that_mixes_every_kind_of_pair(mod, comb):
    """a list pair, a pair that stores everything, the comb pair and a silent pair in one group: each pair's results are those of
    running it alone with the switch off"""
    pairs = mixed_group(comb)
    on, stats = three_ways(mod, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    assert stats[:3] == (2, 2, 1), stats
    with mod.Plan(N, 1, 0) as plan:
        plan.set_qstore(0)
        for i, (s, t) in enumerate(pairs):
            alone = plan._strided_f32(np.ascontiguousarray(s, dtype=np.float32), 2 * N, np.ascontiguousarray(t, dtype=np.float32), N, 1)
            same([v[i:i + 1] for v in on], alone, "pair %d alone" % i)


@gpu
def test_the_host_pointer_call_runs_a_short_pair_again_too(mod, comb):
    """asx_xcorr_batch_f32: the second run behind fetch_results' look at the list, and the results copied out again; two groups"""
    pairs = mixed_group(comb)
    on, stats = three_ways(mod, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), host=True, group=2)
    assert stats[:3] == (2, 2, 1), stats
