"""Self-test of tests/guards_ref.py (no GPU): the float64 references agree with the suite's older models, a float32 model of the
kernel's own summation order passes the cell check, every check FAILS on a planted fault, and the sweeps the device tests run
across the coefficient's tolerance do straddle it in the float64 prediction."""
import math

import numpy as np
import pytest

import guards_ref as G
import model_fourstep as mf
from util import asx

U = G.U


def noise_matrix(seed, rows, M2, offset=0.0):
    return (np.random.default_rng(seed).uniform(-1, 1, rows * M2) + offset).astype(np.float32)


def tone_pair(n):
    """test_gpu_exact_peak.tonal_pairs' "tone + weak noise" """
    i = np.arange(2 * n, dtype=np.float64)
    rng = np.random.default_rng(n)
    return ((np.sin(0.05 * i) + 1e-3 * rng.normal(size=2 * n)).astype(np.float32),
            (np.sin(0.05 * i[:n] + 2.0) + 1e-3 * rng.normal(size=n)).astype(np.float32))


def test_planted_is_the_suites_planted():
    from test_gpu_pearson_spectral import planted
    a, b = planted(np.random.default_rng(5), 600, -77, sign=-1.0, noise=1.0), G.planted(np.random.default_rng(5), 600, -77, sign=-1.0, noise=1.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("band_rows", [8, 10])
def test_cells_agree_with_the_fourstep_model(band_rows):
    M2, T = 96, 16
    x = noise_matrix(1, 4 * band_rows, M2, 0.3)
    c, p = G.cells64(x, M2, T, band_rows), mf.band_partials(x, M2, T, band_rows)
    assert np.allclose(c["sum"], p[..., 0], rtol=1e-14, atol=1e-12) and np.allclose(c["sq"], p[..., 1], rtol=1e-14)
    assert np.all(c["abs"] >= np.abs(c["sum"]))


@pytest.mark.parametrize("band_rows", [8, 10])
@pytest.mark.parametrize("offset", [0.0, 1.0, 30.0])
def test_float32_model_of_the_kernels_order_passes_the_cell_check(band_rows, offset):
    """k_fwd_cols_r's order (eight-FMA chain per row pair, tree over RPQ, quad sum) in numpy float32: well inside 16 u.
    Measured: at most 2.3 u on either sum, offsets 0, 1 and 30."""
    M2, T = 480, 16
    x = noise_matrix(7, 6 * band_rows, M2, offset)
    s, q = G.model_cells32(x, M2, band_rows, T)
    w1, w2 = G.check_cells(s, q, G.cells64(x, M2, T, band_rows))
    print("band_rows=%d offset=%g: model's worst cell error %.2f u (sum), %.2f u (squares)" % (band_rows, offset, w1, w2))
    assert w1 <= 4.0 and w2 <= 4.0      # the model's own margin: a correct kernel is nowhere near the limit


def test_cell_check_fails_on_a_perturbed_and_on_swapped_cells():
    M2, T, band_rows = 480, 16, 10
    x = noise_matrix(9, 60, M2)
    ref = G.cells64(x, M2, T, band_rows)
    s, q = G.model_cells32(x, M2, band_rows, T)
    G.check_cells(s, q, ref)
    for which in (0, 1):
        bad = [s.astype(np.float64), q.astype(np.float64)]
        bad[which][3, 11] += 32 * U * (ref["abs"] if which == 0 else ref["sq"])[3, 11]
        with pytest.raises(AssertionError):
            G.check_cells(bad[0], bad[1], ref)
    for a, b in (((2, 5), (2, 6)), ((1, 0), (2, 0))):      # neighbouring tiles, neighbouring bands
        bs, bq = s.copy(), q.copy()
        bs[a], bs[b] = s[b], s[a]
        bq[a], bq[b] = q[b], q[a]
        with pytest.raises(AssertionError):
            G.check_cells(bs, bq, ref)


@pytest.mark.parametrize("lag", [0, 77, -3, -1201])
def test_window_check_fails_on_an_edge_one_sample_short(lag):
    n = 24000
    x, y = G.planted(np.random.default_rng(3), n, lag)
    peak = G.peak_of_lag(lag, n)
    ref = G.window_sums64(x, y, peak)
    names = ("n", "Sx", "Sxx", "Sy", "Syy")
    assert all(v == 0.0 for v in G.check_window(dict(zip(names, ref)), ref))
    _, so, mo, ln = G.seg_of(peak, n)
    for track, off, k in ((x, so, 1), (y, mo, 3)):
        for cut in (off, off + ln - 1):                         # the first sample of the window missing, or the last
            v = float(track[cut])
            if abs(v) < 0.3:
                continue                                        # (a sample too small to show in either sum: not this test's fault)
            short = list(ref)
            short[k] -= v
            short[k + 1] -= v * v
            with pytest.raises(AssertionError):
                G.check_window(dict(zip(names, short)), ref)
    wrong_n = dict(zip(names, ref), n=ref[0] - 1)
    with pytest.raises(AssertionError):
        G.check_window(wrong_n, ref)


def test_list_check_fails_when_a_must_list_lag_is_missing_or_a_stray_is_listed():
    n = 4096
    x, y = tone_pair(n)
    key = G.keys64(G.r64_all(x, y))
    bp = G.B64(x, y, 2 * n)
    m = key.max()
    must = np.nonzero(key >= m - bp)[0]
    wide = np.nonzero(key >= m - 3 * bp)[0]
    assert 2 <= must.size < wide.size < n // 4     # a tonal pair: many near-ties, and lags between B and 3 B
    assert G.check_list(must, key, bp) == (must.size, must.size)
    G.check_list(wide, key, bp)
    for drop in (0, must.size // 2, must.size - 1):
        with pytest.raises(AssertionError):
            G.check_list(np.delete(must, drop), key, bp)
    stray = int(np.argmin(key))
    with pytest.raises(AssertionError):
        G.check_list(np.append(must, stray), key, bp)


def test_exact_check_fails_four_ulp_off_and_the_two_references_agree():
    n = 4096
    x, y = tone_pair(n)
    for k in (0, 1, n - 1, n, 2 * n - 1):
        ref, sa = G.exact_r(x, y, k)
        ref64, sa64 = G.exact_r(x.astype(np.float64), y.astype(np.float64), k)     # the integer route on the same values
        assert float(ref64) == float(ref) and abs(ref64 - ref) <= abs(ref) / 2 ** 53 and float(sa64) == float(sa)
        idx = (np.arange(n) + k) % (2 * n)
        assert abs(float(ref) - float(np.dot(x.astype(np.float64)[idx], y.astype(np.float64)))) <= 1e-12 * float(sa)
        v = float(ref)
        assert G.check_exact(v, ref, sa, n) <= 0.5
        G.check_exact(np.nextafter(v, math.inf), ref, sa, n)
        for off in (4, -4):
            with pytest.raises(AssertionError):
                G.check_exact(v * (1.0 + off * 2.0 ** -52), ref, sa, n)


def test_bound_formula_and_modes():
    """spec_bound64 on a plain pair at 144 000: 7.1e-6 (rb = B carries 6.1e-6 of it); the modes follow asx_spec_pick"""
    n = 144000
    x, y = G.planted(np.random.default_rng(1), n, 5000)
    bound, mode, w = G.predict(x, y, 5000, 2 * n)
    assert 6.5e-6 < bound < 7.7e-6 and mode == G.FAST and w[0] == n
    assert G.spec_bound64(*w, 0.0)[0] < 1.1e-6                      # re-evaluated near-ties: the band sums' share alone
    assert G.spec_bound64(n, 1.0, 0.5 / n, 0.0, 1.0, 0.0)[0] == math.inf   # A <= 0
    assert G.mode_of(5e-6, 2 * n - 10, n) == G.CORR and G.mode_of(5e-6, n + 10, n) == G.DIRECT and G.mode_of(2e-5, 10, n) == G.DIRECT
    assert G.seg_of(G.peak_of_lag(-n, n), n) == (-n, 0, n, 0) and G.seg_of(G.peak_of_lag(-1, n), n) == (-1, 0, 1, n - 1)


@pytest.mark.parametrize("n", [144000, 960000])
@pytest.mark.parametrize("kind", sorted(G.SWEEPS))
def test_sweeps_straddle_the_tolerance(n, kind):
    """each sweep of test_gpu_spectral_inputs.py has at least two pairs under 0.9e-5 and two over 1.1e-5 in the float64 prediction"""
    F = asx().planmath_describe(n)["F"]
    assert F == 2 * n
    pred = [(v, G.predict(s, t, lag, F)[0] / G.TOL) for v, s, t, lag in G.sweep_pairs(n, kind)]
    print("N=%d %s: predicted bound / 1e-5: %s" % (n, kind, "  ".join("%g: %.2f" % p for p in pred)))
    assert sum(b < 0.9 for _, b in pred) >= 2 and sum(b > 1.1 for _, b in pred) >= 2, pred
