"""The energy bound of the pruned inverse column pass (csrc/rlayout.hip: k_rows_re, k_tile_bounds, k_prune_select), modelled in float32
numpy, no GPU:  eng[k1][tile] = sum over the tile's sixteen columns of |Q[k1][j2]|^2 in float32, ub[tile] = sqrt(4 M1 sum_k1 eng)
(1 + delta) rounded up to float32.  The bound must hold for the float32 model's |r^| of EVERY tile -- on the bench generator's
pairs and on tiles built to strain it (one element holding the whole energy, constant and alternating columns, edge rows with an
imaginary part, NaN) -- and on the headline pairs checked when the change was proposed exactly one tile may survive it."""
import os
import re

import numpy as np
import pytest

import model_fourstep as mf
import oracle
from util import ROOT

T = 16
SEED = 20260101


def delta():
    text = open(os.path.join(ROOT, "old-audiosync_amd", "csrc", "asx_internal.h")).read()
    return float(re.search(r"#define ASX_PRUNE_DELTA\s+([0-9.e+-]+)f", text).group(1))


def floor_per_term():
    text = open(os.path.join(ROOT, "old-audiosync_amd", "csrc", "asx_internal.h")).read()
    return float(re.search(r"#define ASX_PRUNE_FLOOR_PER_TERM\s+([0-9.e+-]+)", text).group(1))


def test_delta_is_at_least_two_to_the_minus_fourteen():
    assert delta() >= 2.0 ** -14


def test_the_floor_is_two_to_the_25_smallest_normal_floats_per_term():
    assert floor_per_term() == 2.0 ** 25 * 2.0 ** -126


def q_of_r(r, M1, M2):
    """rows k1 = 0 .. M1 of Q whose c2r column transform (unnormalised, length 2 M1) is r[2 M1][M2]"""
    return np.fft.rfft(np.asarray(r, dtype=np.float64).reshape(2 * M1, M2), axis=0) / (2 * M1)


def inv_cols_f32(Q, M1, M2):
    """tests/model_fourstep.py::rlayout_inv_cols on a float32 Q in float32 throughout: the tangling in complex64 and the M1-point
    inverse transform as a complex64 matrix product (a plain DFT: it accumulates M1 float32 terms per output, more rounding
    than the kernel's three-stage transform, so it strains the factor harder)"""
    Q = Q.astype(np.complex64)
    Zp = np.zeros((M1, M2), dtype=np.complex64)
    for u in range(M1 // 2 + 1):
        qa, qb = Q[u], Q[M1 - u]
        S = qa + np.conj(qb)
        D = qa - np.conj(qb)
        t = (1j * np.conj(mf.tw(2 * M1, u))).astype(np.complex64) * D
        Zp[u] = S + t
        if (M1 - u) % M1 != u:
            Zp[M1 - u] = np.conj(S - t)
    k = np.arange(M1)
    W = np.exp(2j * np.pi * ((k[:, None] * k[None, :]) % M1) / M1).astype(np.complex64)  # unnormalised inverse DFT
    z = W @ Zp
    assert z.dtype == np.complex64
    r = np.zeros((2 * M1, M2), dtype=np.float32)
    r[0::2] = z.real
    r[1::2] = z.imag
    return r


def bounds_f32(Q, M1, M2):
    """what k_rows_re and k_tile_bounds leave: float32 tile energies per row, float64 over the rows, the factor, rounded up"""
    Q = Q.astype(np.complex64)
    sq = Q.real * Q.real + Q.imag * Q.imag                                  # float32
    g = sq.reshape(M1 + 1, M2 // T, 4, 4).sum(axis=3, dtype=np.float32)     # (the kernel adds a balanced tree; any order is within the factor)
    eng = g.sum(axis=2, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = eng.astype(np.float64).sum(axis=0)
        ub = np.sqrt(4.0 * M1 * e) * (1.0 + delta())
        f = ub.astype(np.float32)
        f = np.where(f < ub, np.nextafter(f, np.float32(np.inf)), f)
        f = np.where(e < floor_per_term() * T * (M1 + 1), np.float32(np.inf), f)    # under the floor: no bound
    return f


def tile_max(r, M2):
    return np.abs(r).reshape(r.shape[0], M2 // T, T).max(axis=(0, 2))


def assert_bounded(Q, M1, M2, what):
    ub = bounds_f32(Q, M1, M2)
    m = tile_max(inv_cols_f32(Q, M1, M2), M2)
    ok = np.isnan(ub) | (m <= ub)
    assert ok.all(), (what, np.flatnonzero(~ok)[:4], m[~ok][:4], ub[~ok][:4])
    return ub, m


@pytest.mark.parametrize("M1,M2", [(300, 480), (20, 32)])
def test_the_bound_holds_on_tiles_built_to_strain_it(M1, M2):
    rng = np.random.default_rng(M1)
    # one element holds the whole energy of its tile: |r| = the tile's Frobenius norm, only delta is left
    for j1, j2 in [(0, 0), (1, 5), (2 * M1 - 1, M2 - 1), (M1, 17), (M1 + 1, 16)]:
        r = np.zeros((2 * M1, M2))
        r[j1, j2] = 12345.678 if j1 & 1 else -0.3
        ub, m = assert_bounded(q_of_r(r, M1, M2), M1, M2, ("one element", j1, j2))
        t = j2 // T
        assert m[t] > 0 and ub[t] <= m[t] * (1 + 2.0 / M1), (ub[t], m[t])  # and it is tight: rows 0 and M1 count twice, no more
    # constant columns (row 0 alone), alternating columns (row M1 alone), both
    r = np.zeros((2 * M1, M2)); r[:, 3] = 1.0; r[:, M2 - 8] = -7.0
    assert_bounded(q_of_r(r, M1, M2), M1, M2, "constant columns")
    r = np.zeros((2 * M1, M2)); r[0::2, 9] = 1.0; r[1::2, 9] = -1.0
    assert_bounded(q_of_r(r, M1, M2), M1, M2, "alternating column")
    r = np.ones((2 * M1, M2)); r[1::2] = 0.25
    assert_bounded(q_of_r(r, M1, M2), M1, M2, "constant + alternating")
    # noise, and noise of wildly different scale from tile to tile
    r = rng.standard_normal((2 * M1, M2))
    assert_bounded(q_of_r(r, M1, M2), M1, M2, "noise")
    r = r * np.repeat(10.0 ** rng.integers(-12, 12, M2 // T), T)[None, :]
    assert_bounded(q_of_r(r, M1, M2), M1, M2, "scaled noise")
    # rows 0 and M1 with an imaginary part as large as the real one (in exact arithmetic they are real; the kernel's tangling mixes
    # the residue in): the weight 2 of those rows covers it, the weight 1 of Parseval would not
    Q = np.zeros((M1 + 1, M2), dtype=complex)
    Q[0] = rng.standard_normal(M2) + 1j * rng.standard_normal(M2)
    Q[M1] = rng.standard_normal(M2) - 1j * Q[0].real
    assert_bounded(Q, M1, M2, "edge rows with imaginary parts")


def test_a_nan_bound_skips_nothing():
    M1, M2 = 20, 32
    Q = q_of_r(np.random.default_rng(1).standard_normal((2 * M1, M2)), M1, M2)
    Q[7, 3] = np.nan
    ub = bounds_f32(Q, M1, M2)
    assert np.isnan(ub[0]) and not np.isnan(ub[1])
    with np.errstate(invalid="ignore"):
        assert not (ub[0] < np.float32(1e30)) and not (ub[1] < np.float32(np.nan))  # NaN bound, NaN threshold: the comparison is false


def generator_q(n, pair, shift=1):
    src, smp, lag = oracle.synth_pair(SEED, pair, n, shift)
    M2 = {1440000: 2400, 480000: 1200, 144000: 480}[n]
    M1 = n // M2
    t = np.zeros(2 * n)
    t[:n] = smp
    Q = mf.rlayout_rows(mf.rlayout_fwd_cols(src, M1, M2), mf.rlayout_fwd_cols(t, M1, M2), M1, M2)
    F = 2 * n
    b2 = 2 * 4.0 * 2.0 ** -24 * np.log2(F) * F * np.linalg.norm(src.astype(np.float64)) * np.linalg.norm(smp.astype(np.float64))
    return Q, M1, M2, b2, lag


def survivors(Q, M1, M2, b2):
    ub, m = assert_bounded(Q, M1, M2, "generator pair")
    peak = float(m.max())
    return np.flatnonzero(~(ub < np.float32(peak - b2))), int(m.argmax()), ub, peak


@pytest.mark.parametrize("pair", [0, 8, 64])
def test_headline_pairs_keep_exactly_one_tile(pair):
    Q, M1, M2, b2, lag = generator_q(1440000, pair)
    keep, peak_tile, ub, peak = survivors(Q, M1, M2, b2)
    second = np.sort(ub)[-2]
    print("pair %d: tiles kept %s, peak's tile %d, second-largest bound / peak %.3f, b2 / peak %.1e" % (pair, keep, peak_tile, second / peak, b2 / peak))
    assert list(keep) == [peak_tile] == [int(ub.argmax())]
    assert peak_tile == ((lag % (2 * 1440000)) % M2) // T


@pytest.mark.parametrize("scale", [1e-8, 1e-12, 1e-14, 1e-15, 1e-16, 1e-18])
def test_a_scaled_down_pair_is_bounded_or_has_no_bound(scale):
    """quiet tracks: |Q|^2 goes denormal and then to zero in float32 while r is still an ordinary number (amplitude 1e-16: every
    energy 0, max |r^| 4.9e-23).  Modelled both ways the hardware may treat the squares: denormals kept, and flushed to zero."""
    Q, M1, M2, b2, lag = generator_q(144000, 2)
    Q = Q * scale * scale
    ub, m = assert_bounded(Q, M1, M2, ("scaled", scale))
    assert m.max() > 0
    # flushed: every square under the smallest normal float counts as zero
    q = Q.astype(np.complex64)
    re2, im2 = q.real * q.real, q.imag * q.imag
    tiny = np.float32(2.0 ** -126)
    sq = np.where(re2 < tiny, np.float32(0), re2) + np.where(im2 < tiny, np.float32(0), im2)
    e = sq.reshape(M1 + 1, M2 // T, T).sum(axis=2, dtype=np.float32).astype(np.float64).sum(axis=0)
    ubf = np.where(e < floor_per_term() * T * (M1 + 1), np.inf, np.sqrt(4.0 * M1 * e) * (1.0 + delta()))
    assert (m <= ubf).all(), (scale, np.flatnonzero(m > ubf)[:4])
    if scale <= 1e-16:
        assert np.isinf(ub).all()


def test_a_short_pair_is_bounded_too():
    Q, M1, M2, b2, lag = generator_q(144000, 2)
    keep, peak_tile, ub, peak = survivors(Q, M1, M2, b2)
    assert peak_tile in keep
