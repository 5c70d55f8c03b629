"""The copy wave of partial storing applies the conjugate four-step twiddle itself (csrc/rlayout.hip: k_rows_rm, ASX_QTW_LATE): a block
of a pair with a list keeps A +- Bw in LDS, and the lane that stores column c of a listed tile forms Q[c] from it with the register
path's expressions.  Mode 2 against mode 0 (and the unpruned pass) on one plan, groups of four pairs: lag, ret and coefficient bit for
bit.  The spectral coefficient is built from the float32 r[peak], which sums the peak column's Q over every row, so equal bits mean that
all rows of that column were stored with k_rows_re's bits.

A lane holding column c derives upper = c >= NS, i = c mod NS, j = i mod Q0, t = i div Q0 (NS = 1200, Q0 = 100, twelve legs).  The
planted delays put the peak's column (delay mod M2, tests/model_fourstep.py) into every branch of that: tile 0 with a list of one tile
(three unused entries), t = 0 away from tile 0, a middle leg, t = 11, the first column at or above NS (times wh, t = 0), an upper column
with a leg, and the last tile.  One pair of unrelated tracks, which has no list and keeps the register path, rides in the first group.
The float64 model (tests/test_qstore_model.py) is asked first: it alone must list each peak's tile, so that none of the planted pairs
is one the device may run again."""
import numpy as np
import pytest

from test_gpu_qstore import M2, N, T, mod, model_prediction, planted, three_ways, tile_of, unrelated  # noqa: F401 (mod: fixture)

NS, Q0, LEGS = M2 // 2, 100, 12

# name -> (column of the peak, upper, t)
COLUMNS = {
    "tile 0, a list of one tile": (5, False, 0),
    "t = 0, lower half": (3 * T + 7, False, 0),
    "a middle leg, lower half": (37 * T + 15, False, 6),
    "t = R0 - 1, lower half": (71 * T + 14, False, LEGS - 1),
    "the first column of the upper half": (NS, True, 0),
    "upper half with a leg": (NS + 3 * Q0 + 45, True, 3),
    "the last tile": (149 * T + 7, True, LEGS - 1),
}


def branch(c):
    i = c % NS
    return c >= NS, i // Q0


@pytest.fixture(scope="module")
def pairs():
    """[(source, sample, delay or None)]: the planted pairs in COLUMNS' order with the unrelated pair fourth, checked on the CPU"""
    from test_qstore_model import qstore_c
    out = []
    for k, (name, (c, upper, t)) in enumerate(COLUMNS.items()):
        assert branch(c) == (upper, t), (name, c, branch(c))
        delay = (7 + 3 * k) * M2 + c
        src, smp = planted(N, delay, 700 + k)
        listed, ratio = model_prediction(src, smp, qstore_c())
        tile = tile_of(delay, N)
        print("%s: column %d, tile %d at %.1f medians, list %s" % (name, c, tile, ratio[tile], listed))
        assert tile == c // T and listed is not None and tile in listed, (name, tile, listed)
        if tile == 0:
            assert listed == [0], (name, listed)
        out.append((src, smp, delay))
    u = unrelated(N, 790)
    listed, _ = model_prediction(u[0], u[1], qstore_c())
    assert listed is None, listed
    out.insert(3, (u[0], u[1], None))
    return out


@pytest.mark.gpu
def test_every_branch_of_the_copy_wave_stores_the_register_paths_bits(mod, pairs):
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    on, stats = three_ways(mod, src, smp, host=True, group=4)   # asserts the bits, the Pearson modes and the overflow counts
    for i, (_, _, delay) in enumerate(pairs):
        assert delay is None or int(on[0][i]) == delay, (i, int(on[0][i]), delay)
    planted_n = len(COLUMNS)
    assert stats[0] == planted_n and stats[1] == 1 and stats[2] == 0, stats
    assert stats[3] <= 4 * planted_n + M2 // T, stats
