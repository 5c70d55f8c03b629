"""The tile energies of the row pass and the bounds made of them (csrc/rlayout.hip: k_rows_re, k_tile_bounds) at the smallest length
of each k_rows_re instance: N = 144 000 (480-point rows, 30 tiles), 480 000 (1200-point rows in one piece, 75 tiles), 960 000 (the
two-half form, 150 tiles).  k_rows_re writes |Q|^2 of column c into LDS slot c and sixteen lanes add a tile; k_tile_bounds sums a
pair's rows in slices, one block each, and the pair's last-arriving block adds the slices.

One pair of unrelated uniform noise tracks per length (every tile carries about the same energy, so a column summed into the wrong
tile shows), alone and inside batches of five different pairs."""
import numpy as np
import pytest

from util import asx

LENGTHS = [144000, 480000, 960000]
TILES = {144000: 30, 480000: 75, 960000: 150}
# sum of r^2 over a tile against the square of its bound, largest ub^2 / sum - 1 over all tiles of the three pairs below, measured on
# the build of round 7 (one thread per tile, one block per pair): RATIO_ROUND7.  The test allows that plus 2^-10 (SLACK).
RATIO_ROUND7 = 5.581450718e-03
SLACK = 2.0 ** -10

gpu = pytest.mark.gpu


def noise_pair(n, k=0):
    rng = np.random.default_rng(1000 * k + n // 1000)
    return rng.uniform(-1.0, 1.0, 2 * n).astype(np.float32), rng.uniform(-1.0, 1.0, n).astype(np.float32)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_r(plan, src, smp):
    """the float32 r (times F) the device computes for one pair, every lag"""
    import torch
    n = smp.size
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_lag = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
    d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
    plan.sync()
    return d_r.cpu().numpy()


def tile_ratios(mod, n):
    """(ub, best, sum of r^2 per tile in float64) of the noise pair of length n, run alone"""
    src, smp = noise_pair(n)
    with mod.Plan(n, 1, 0) as plan:
        M1, M2, T = plan.split
        assert plan.layout == "real-column" and T == 16 and M2 // T == TILES[n], plan.split
        plan.set_prune(True)
        plan.xcorr_batch_f32(src[None], smp[None])
        ub, best = plan.debug_prune(0)
        r = device_r(plan, src, smp)
    energy = (r.astype(np.float64).reshape(2 * M1, M2 // T, T) ** 2).sum(axis=(0, 2))
    return np.array(ub, dtype=np.float32), int(best), energy


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def alone(mod):
    """per length: (ub, best, tile energies of r) of the noise pair run alone -- computed once, shared, not modified"""
    return {n: tile_ratios(mod, n) for n in LENGTHS}


@gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_every_column_lands_in_its_tile(alone, n):
    """For every tile: sum of r^2 over the tile <= ub^2 (the bound holds), and ub^2 <= that sum times (1 + x): the bound is made of
    this tile's sixteen columns and of nothing else -- one column of a neighbour moves it by about 6 %.  x covers the double weight
    of rows 0 and M1 (order 1 / M1) and the factor delta.  Measured on round 7's build with these inputs: largest ub^2 / sum - 1 =
    5.581e-3 (RATIO_ROUND7; at N = 144 000, M1 = 300; 4.380e-3 and 5.119e-3 at the other two, profiles/r8_rows_eng/tile_ratios_parent.txt);
    x = that + 2^-10 = 6.558e-3.  This build leaves the same ub bits as round 7's (tile_ratios_new.txt)."""
    ub, best, energy = alone[n]
    ub2 = ub.astype(np.float64) ** 2
    ratio = ub2 / energy - 1.0
    print("N = %d: %d tiles, ub^2 / sum r^2 - 1 in [%.6e, %.6e], best %d" % (n, ub.size, ratio.min(), ratio.max(), best))
    assert ub.size == TILES[n] and np.isfinite(ub).all()
    assert (energy <= ub2).all(), (np.flatnonzero(energy > ub2), ratio.min())
    assert (ub2 <= energy * (1.0 + RATIO_ROUND7 + SLACK)).all(), (np.flatnonzero(ratio > RATIO_ROUND7 + SLACK), ratio.max())
    assert best == int(np.argmax(ub))  # ties: the smallest tile, as argmax


@gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_bounds_do_not_depend_on_the_batch_position_or_the_call(mod, alone, n):
    """the pair at positions 0, 2 and 4 of a batch of five different pairs, two consecutive calls each: the ub bits and best of the
    pair run alone (no atomics on the values, slices added in slice order whichever block arrives last); lag, ret and coefficient
    bit-equal with pruning on and off; the two calls transform the same number of tiles"""
    ub0, best0, _ = alone[n]
    p = noise_pair(n)
    others = [noise_pair(n, k) for k in range(1, 5)]
    with mod.Plan(n, 5, 0) as plan:
        for pos in (0, 2, 4):
            batch = others[:pos] + [p] + others[pos:]
            src = np.stack([b[0] for b in batch])
            smp = np.stack([b[1] for b in batch])
            plan.set_prune(True)
            s0 = plan.prune_stats()
            on1 = plan.xcorr_batch_f32(src, smp)
            ub1, best1 = plan.debug_prune(pos)
            s1 = plan.prune_stats()
            on2 = plan.xcorr_batch_f32(src, smp)
            ub2, best2 = plan.debug_prune(pos)
            s2 = plan.prune_stats()
            plan.set_prune(False)
            off = plan.xcorr_batch_f32(src, smp)
            assert plan.prune_stats() == s2
            for ub, best in ((ub1, best1), (ub2, best2)):
                assert np.array_equal(bits32(ub), bits32(ub0)), (pos, np.flatnonzero(bits32(ub) != bits32(ub0)))
                assert int(best) == best0, (pos, best, best0)
            assert (s1[0] - s0[0], s1[1] - s0[1]) == (s2[0] - s1[0], s2[1] - s1[1]) and s1[1] - s0[1] == 5 * TILES[n], (s0, s1, s2)
            for on in (on1, on2):
                assert np.array_equal(np.asarray(on[0]), np.asarray(off[0])), (pos, "lag", on[0], off[0])
                assert np.array_equal(np.asarray(on[2]), np.asarray(off[2])), (pos, "ret", on[2], off[2])
                assert np.array_equal(bits64(on[1]), bits64(off[1])), (pos, "coefficient bits", on[1], off[1])
