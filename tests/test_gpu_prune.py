"""The pruned inverse column pass (asx_plan_set_prune, include/audiosync/xcorr_hip.h; csrc/rlayout.hip: k_rows_re, k_tile_bounds,
k_prune_select, k_inv_cols_r<..., AsxSelPrune>) against the unpruned pass ON THE SAME PLAN: lag and ret equal, the coefficient bit for bit, and all
three against the float64 oracle under the project's tolerance.  The coefficient of the spectral Pearson form is built from the
float32 r[peak], so its bits also say that k_rows_re leaves the Q that k_rows_r leaves.

Inputs: generator pairs at the six production lengths, a tone, unrelated noise, a DC offset in both tracks, a silent track, NaN
input, and a pair whose peak is NOT in the tile with the largest bound (a pulse train of period M2 puts the energy of r into one
column tile; a stronger planted delay sits elsewhere).  asx_plan_prune_stats on the headline pairs checked on the CPU
(tests/test_prune_bound.py): at most two tiles per pair are transformed."""
import numpy as np
import pytest

import oracle
from util import asx

COEF_TOL = 1e-5
PRODUCTION = [144000, 288000, 480000, 720000, 960000, 1440000]
SEED = 20260101

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def on_and_off(mod, src, smp):
    """the same pairs through the pruned and the unpruned pass of one plan -> ((lag, coef, ret) on, (lag, coef, ret) off, stats)"""
    n = smp.shape[1]
    with mod.Plan(n, src.shape[0], 0) as plan:
        assert plan.layout == "real-column"
        plan.set_prune(True)
        on = plan.xcorr_batch_f32(src, smp)
        stats = plan.prune_stats()
        plan.set_prune(False)
        off = plan.xcorr_batch_f32(src, smp)
        assert plan.prune_stats() == stats, "the unpruned pass counts nothing"
    return on, off, stats


MARGIN_DEFINED = 1.0 + 1e-12  # tests/test_gpu_exact_peak.py: below it the float64 reference is within rounding of a tie


def check(mod, src, smp, names):
    on, off, stats = on_and_off(mod, src, smp)
    print("tiles transformed %d of %d" % stats)
    assert stats[1] > 0 and 0 < stats[0] <= stats[1], stats
    for b, name in enumerate(names):
        assert int(on[0][b]) == int(off[0][b]), (name, "lag", on[0][b], off[0][b])
        assert int(on[2][b]) == int(off[2][b]), (name, "ret", on[2][b], off[2][b])
        assert bits(on[1])[b] == bits(off[1])[b], (name, "coefficient bits", float(on[1][b]), float(off[1][b]))
        o_ret, o_lag, o_coef, o_r, margin = oracle.cross_correlation(src[b], smp[b], want_results=True)
        if margin <= MARGIN_DEFINED:
            continue
        assert int(on[2][b]) == o_ret, (name, int(on[2][b]), o_ret)
        assert int(on[0][b]) == o_lag, (name, int(on[0][b]), o_lag, margin)
        if o_ret == 0:
            assert abs(float(on[1][b]) - o_coef) < COEF_TOL or (np.isnan(on[1][b]) and np.isnan(o_coef)), (name, float(on[1][b]), o_coef)
    return on, stats


@gpu
@pytest.mark.parametrize("n", PRODUCTION)
def test_generator_pairs_at_every_production_length(mod, n):
    pairs = [oracle.synth_pair(SEED, p, n, 1) for p in range(4)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    on, stats = check(mod, src, smp, ["pair %d" % p for p in range(4)])
    assert [int(v) for v in on[0]] == [p[2] for p in pairs]


def special_pairs(n, M2):
    i = np.arange(2 * n, dtype=np.float64)
    rng = np.random.default_rng(n + 5)
    out = {}
    out["two tones"] = (np.sin(0.31 * i) + 0.7 * np.sin(0.071 * i + 1.0), np.sin(0.31 * i[:n] + 0.4) + 0.7 * np.sin(0.071 * i[:n] + 1.3))
    out["unrelated noise"] = (rng.standard_normal(2 * n), rng.standard_normal(n))
    g = oracle.synth_pair(SEED, 5, n, 1)
    off = 2.0 * float(np.std(g[0]))
    out["dc offset in both"] = (g[0].astype(np.float64) + off, g[1].astype(np.float64) + off)
    out["silent sample"] = (g[0].astype(np.float64), np.zeros(n))
    out["pulse tile + planted delay"] = pulse_pair(n, M2, rng)
    return {k: (a.astype(np.float32), b.astype(np.float32)) for k, (a, b) in out.items()}


def pulse_pair(n, M2, rng, delay=40077, col_src=37, col_smp=5):
    """source = pulses every M2 samples + noise, sample = pulses every M2 samples + the source's noise from `delay` on: r has a
    comb of equal values in the column (col_src - col_smp) mod M2 -- one column tile holds their whole energy, 2 M1 values a fifth
    of the peak each -- and the peak at `delay`, in another tile"""
    noise = rng.standard_normal(2 * n)
    amp = np.sqrt(0.2 * n / (n // M2))
    src = noise.copy()
    src[col_src::M2] += amp
    smp = noise[delay:delay + n].copy()
    smp[col_smp::M2] += amp
    return src, smp


@gpu
def test_special_inputs(mod):
    n, M2, T = 144000, 480, 16
    pairs = special_pairs(n, M2)
    names = list(pairs)
    src = np.stack([pairs[k][0] for k in names])
    smp = np.stack([pairs[k][1] for k in names])
    # the constructed pair is what it claims to be (float64, numpy): the tile with the largest energy is not the peak's
    s, t = pairs["pulse tile + planted delay"]
    F = 2 * n
    r = np.fft.irfft(np.fft.rfft(s.astype(np.float64)) * np.conj(np.fft.rfft(np.concatenate([t, np.zeros(n, np.float32)]).astype(np.float64))), F)
    energy = (r.reshape(F // M2, M2 // T, T) ** 2).sum(axis=(0, 2))
    peak = int(np.abs(r).argmax())
    assert peak == 40077 and int(energy.argmax()) == ((37 - 5) % M2) // T != (peak % M2) // T
    with mod.Plan(n, 1, 0) as plan:
        assert plan.split[1:] == (M2, T)
    check(mod, src, smp, names)


@gpu
def test_very_quiet_pairs(mod):
    """Tracks so quiet that |Q|^2 underflows in float32 although r does not (amplitude 1e-16: |r| ~ 5e-23): under the energy floor
    (csrc/asx_internal.h) a tile has no bound and is transformed, so the pair keeps the unpruned pass's answer"""
    n = 144000
    src, smp, lag = oracle.synth_pair(SEED, 2, n, 1)
    scales = [1e-10, 1e-14, 1e-16]
    s = np.stack([(src.astype(np.float64) * c).astype(np.float32) for c in scales])
    t = np.stack([(smp.astype(np.float64) * c).astype(np.float32) for c in scales])
    on, stats = check(mod, s, t, ["scale %g" % c for c in scales])
    assert [int(v) for v in on[0]] == [lag] * 3, on[0]
    with mod.Plan(n, 1, 0) as plan:
        plan.xcorr_batch_f32(s[2:], t[2:])
        assert plan.prune_stats() == (30, 30)       # nothing is pruned under the floor
        ub, best = plan.debug_prune(0)
        assert np.isinf(ub).all(), ub


@gpu
def test_the_bound_on_the_device_is_tight_on_an_impulse_pair(mod):
    """one non-zero lag: its tile's bound is the value itself but for the factor and the double weight of rows 0 and M1 -- a wrong
    scale in k_tile_bounds (2 M1 for 4 M1, say) fails here; every tile's bound holds against the r the device computes"""
    import torch
    n, M1, M2, T = 144000, 300, 480, 16
    src = np.zeros(2 * n, dtype=np.float32)
    smp = np.zeros(n, dtype=np.float32)
    src[50000] = 2.0
    smp[100] = 3.0
    with mod.Plan(n, 1, 0) as plan:
        lag, coef, ret = plan.xcorr_batch_f32(src[None], smp[None])
        ub, best = plan.debug_prune(0)
        d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        d_lag = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
        d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
        plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
        r = d_r.cpu().numpy()
    assert int(lag[0]) == 49900 == int(np.abs(r).argmax())
    m = np.abs(r).reshape(2 * M1, M2 // T, T).max(axis=(0, 2))
    tile = (49900 % M2) // T
    print("tile %d: max |r| %.9g, bound %.9g, ratio - 1 = %.3e" % (tile, m[tile], ub[tile], ub[tile] / m[tile] - 1))
    assert best == tile
    assert (m <= ub).all(), (np.flatnonzero(m > ub), m[m > ub], ub[m > ub])
    assert abs(m[tile] - 6.0 * 2 * n) <= 1e-5 * 6.0 * 2 * n and ub[tile] <= m[tile] * (1 + 1.0 / M1 + 2.0 ** -13), (m[tile], ub[tile])


@gpu
def test_nan_input(mod):
    n = 144000
    src, smp, _ = oracle.synth_pair(SEED, 6, n, 1)
    src = src.copy()
    src[1234] = np.nan
    good = oracle.synth_pair(SEED, 7, n, 1)
    on, off, stats = on_and_off(mod, np.stack([src, good[0]]), np.stack([smp, good[1]]))
    for a, b in zip(on, off):
        assert np.array_equal(bits(a), bits(b)), (a, b)
    o_ret, o_lag, o_coef = oracle.cross_correlation(src, smp)
    assert (int(on[2][0]), int(on[0][0])) == (o_ret, o_lag)
    assert int(on[0][1]) == good[2]


@gpu
def test_headline_pairs_transform_at_most_two_tiles(mod):
    n = 1440000
    pairs = [oracle.synth_pair(SEED, p, n, 1) for p in (0, 8, 64)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    on, off, stats = on_and_off(mod, src, smp)
    print("tiles transformed %d of %d" % stats)
    assert stats[1] == 3 * 150, stats
    assert stats[0] <= 2 * 3, stats
    assert [int(v) for v in on[0]] == [p[2] for p in pairs]
    for a, b in zip(on, off):
        assert np.array_equal(bits(a), bits(b))


@gpu
def test_a_group_of_many_pairs_and_several_groups(mod):
    """a batch that spans launch groups (max_batch below the batch): every group runs the pruned chain on its own workspaces"""
    n = 144000
    pairs = [oracle.synth_pair(SEED, 100 + p, n, 1) for p in range(40)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    with mod.Plan(n, 16, 0) as plan:
        on = plan.xcorr_batch_f32(src, smp)
        stats = plan.prune_stats()
        plan.set_prune(False)
        off = plan.xcorr_batch_f32(src, smp)
    assert stats[1] == 40 * 30, stats
    for a, b in zip(on, off):
        assert np.array_equal(bits(a), bits(b))
    assert [int(v) for v in on[0]] == [p[2] for p in pairs]
