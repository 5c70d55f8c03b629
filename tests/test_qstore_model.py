"""The prediction of partial storing (csrc/rlayout.hip: k_q_predict) stated in Python on tests/model_fourstep.py's Q, no GPU.  Per pair
p[t] = the float64 sum over the predictor rows [a, a + R0) of the row's float32 tile energies; the list is tile 0 plus the up-to-three
tiles t != 0 of largest p[t] that exceed c medians of p (ties: the smaller tile; the median: the element of rank ntiles / 2); no list
when no tile, tile 0 included, exceeds it.  Here at the N = 144 000 geometry (300 x 480, 30 tiles), where the model is quick: the
generator's pairs get the peak's tile into the list, unrelated noise gets none for the c of csrc/asx_internal.h, and the comb
construction of tests/test_gpu_qstore.py misses.  A wrong list costs time only: k_prune_select checks it against the exact bounds."""
import os
import re

import numpy as np
import pytest

import model_fourstep as mf
import oracle
from util import ROOT

T = 16
SEED = 20260101
N, M1, M2 = 144000, 300, 480
A, R0 = M1 // 3, 8


def qstore_c():
    text = open(os.path.join(ROOT, "old-audiosync_amd", "csrc", "asx_internal.h")).read()
    return float(re.search(r"#define ASX_QSTORE_C\s+([0-9.e+-]+)", text).group(1))


def q_model(src, smp, m1, m2):
    n = len(smp)
    t = np.zeros(2 * n)
    t[:n] = smp
    return mf.rlayout_rows(mf.rlayout_fwd_cols(np.asarray(src, dtype=np.float64), m1, m2), mf.rlayout_fwd_cols(t, m1, m2), m1, m2)


def predict(Q, a, r0, c):
    """-> (the list [0, ...] or None for "store everything", p / median)"""
    q = Q[a:a + r0].astype(np.complex64)
    sq = q.real * q.real + q.imag * q.imag
    eng = sq.reshape(r0, -1, T).sum(axis=2, dtype=np.float32)   # (the kernel adds a balanced tree: a rounding apart)
    p = eng.astype(np.float64).sum(axis=0)
    med = np.sort(p)[len(p) // 2]
    order = sorted(range(1, len(p)), key=lambda t: (-p[t], t))[:3]
    picks = [t for t in order if p[t] > c * med]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = p / med
    if not picks and not p[0] > c * med:
        return None, ratio
    return [0] + picks, ratio


def tile_of(lag):
    return ((lag % (2 * N)) % M2) // T


def test_the_constant_is_between_the_noise_and_the_generator():
    assert 1.5 <= qstore_c() <= 2.0


@pytest.mark.parametrize("shift", [0, 1])
def test_generator_pairs_get_the_peaks_tile(shift):
    c = qstore_c()
    for pair in range(12):
        src, smp, lag = oracle.synth_pair(SEED, pair, N, shift)
        listed, ratio = predict(q_model(src, smp, M1, M2), A, R0, c)
        t = tile_of(lag)
        print("shift %d pair %d: list %s, peak's tile %d at %.2f medians, the largest other tile at %.2f" %
              (shift, pair, listed, t, ratio[t], np.sort(np.delete(ratio, [0, t]))[-1]))
        # (tile 0 is stored whatever the list says; a peak there need not stand out of the other tiles to be found)
        assert t == 0 or (listed is not None and t in listed), (pair, t, listed, ratio[t])
        assert listed is None or (len(listed) <= 4 and listed[0] == 0)


def test_unrelated_noise_stores_everything():
    """300 pairs of unrelated Gaussian tracks: the largest tile stays under c medians in every one"""
    c = qstore_c()
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in range(300):
        src, smp = rng.standard_normal(2 * N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        listed, ratio = predict(q_model(src, smp, M1, M2), A, R0, c)
        worst = max(worst, float(ratio.max()))
        assert listed is None, (i, listed, ratio.max())
    print("largest tile over 300 noise pairs: %.3f medians (c = %.2f)" % (worst, c))
    assert worst < c / 1.2, "a fifth of margin over what a few hundred pairs reach"


def comb_pair(n, m1, a, r0, d_true, d_decoy, seed, margin=6):
    """source = noise; sample = the source from d_true on + noise -- but in the bins of the sample's spectrum that fall into the
    predictor rows (and `margin` rows around them: the zero-padded transform's odd bins are interpolated from their neighbours) the
    source from d_decoy on takes its place.  Row k1 of the 2n-point spectrum holds the bins k = k1 (mod 2 M1), and the mirrors of
    the bins k = 2 M1 - k1; bin j of the n-point spectrum is bin 2 j of it.  The decoy holds a few percent of the bins: the true
    delay stays the peak."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n)
    noise = rng.standard_normal(n)
    y_true, y_decoy = np.fft.rfft(src[d_true:d_true + n]), np.fft.rfft(src[d_decoy:d_decoy + n])
    k1 = (2 * np.arange(n // 2 + 1)) % (2 * m1)
    lo, hi = a - margin, a + r0 + margin
    mask = ((k1 >= lo) & (k1 < hi)) | ((2 * m1 - k1 >= lo) & (2 * m1 - k1 < hi))
    smp = np.fft.irfft(np.where(mask, y_decoy, y_true), n) + noise
    return src.astype(np.float32), smp.astype(np.float32)


def test_the_comb_pair_misses():
    """the list names the decoy's tile and not the true one, whose bound k_prune_select will then find unstored"""
    d_true, d_decoy = 40077, 100300
    src, smp = comb_pair(N, M1, A, R0, d_true, d_decoy, 11)
    listed, ratio = predict(q_model(src, smp, M1, M2), A, R0, qstore_c())
    t_true, t_decoy = tile_of(d_true), tile_of(d_decoy)
    print("list %s; true tile %d at %.2f medians, decoy tile %d at %.2f" % (listed, t_true, ratio[t_true], t_decoy, ratio[t_decoy]))
    assert t_true != t_decoy and listed is not None and t_decoy in listed and t_true not in listed
    r = mf.reference_r(src.astype(np.float64), smp.astype(np.float64))
    assert int(np.abs(r).argmax()) == d_true, "the true delay is still the peak"
