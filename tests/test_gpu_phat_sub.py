"""Sub-sample GCC-PHAT on the MI355X (asx_xcorr_phat_sub_f32_dev, asx_xcorr_pool_phat_sub_f32_dev and their Plan methods).

(lag, coef, peak, ret) must be the banded PHAT call's bits; near must be the float64 model's curve (tests/phat_sub_model.py) around
the peak within the PHAT call's measured float32 error, with the peak planted at a row's first and last column, at index 0, at
2N - 1, at lag N - 1 and at lag -N; frac must be the header's rule applied to the call's own near.  N = 144 000 is the smallest
real-column length (300 x 480); N = 960 000 has other row counts and the two-half row form.

No existing PHAT test captures a stream into a graph, so none does here (the call allocates and synchronises nothing, as they)."""
import numpy as np
import pytest

import phat_band_model
import phat_sub_model
from test_gpu_phat import CURVE_TOL
from util import asx

pytestmark = pytest.mark.gpu

N = 144000
LOW = (1, N // 6)         # a lobe several frames wide: the bit-for-bit tests
MID = (1000, N // 2)     # half the spectrum: the planted pairs' |den| is 0.43, against 0.05 under LOW (float64 model)
DEN_MIN = 0.1
assert CURVE_TOL == 2e-7

_tracks, _curves = {}, {}


def track(n, seed=31):
    """2n samples of white noise as float32; computed once per length and never written to"""
    if (n, seed) not in _tracks:
        x = np.random.default_rng(seed).standard_normal(2 * n).astype(np.float32)
        x.setflags(write=False)
        _tracks[n, seed] = x
    return _tracks[n, seed]


def planted(n, lag, sign=1.0):
    """a sample whose correlation with track(n) peaks at `lag` (any lag in [-n, n - 1]): n samples of the track from frame lag on,
    circularly, so that r[lag mod 2n] is the sample's energy"""
    return (sign * np.roll(track(n), -lag)[:n]).astype(np.float32)


def curve(n, lag, sign, band):
    """the float64 r_phat / V of (track(n), planted(n, lag, sign)) under `band`; computed once"""
    key = (n, lag, sign, band)
    if key not in _curves:
        r = phat_band_model.r_phat_band(track(n), planted(n, lag, sign), *band)
        r.setflags(write=False)
        _curves[key] = r
    return _curves[key]


def model(n, lag, sign, band, h, window=None):
    lo, hi = window if window is not None else (None, None)
    return phat_sub_model.model(track(n), planted(n, lag, sign), *band, h, lo, hi, r=curve(n, lag, sign, band))


def bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


def all_bits(out):
    return [np.asarray(a).tobytes() for a in out]


def four(sub):
    """(lag, coef, peak, ret) of a sub call's six results"""
    return sub[0], sub[1], sub[2], sub[5]


def frac_rule(near, h):
    """the header's rule in numpy float64, in its order, over the rows of `near`"""
    ym, y0, yp = near[:, h - 1], near[:, h], near[:, h + 1]
    s = np.where(y0 < 0.0, -1.0, 1.0)
    a, b, c = s * ym, s * y0, s * yp
    den = (a - 2.0 * b) + c
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.clip(0.5 * (a - c) / den, -0.5, 0.5)
    f = np.where(den >= 0.0, 0.0, f)
    return np.where(np.isnan(ym) | np.isnan(y0) | np.isnan(yp), np.nan, f)


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


def outputs(torch, b, h):
    f64 = lambda count: torch.full((count,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    return (torch.full((b,), -99, dtype=torch.int64, device="cuda"), f64(b), f64(b), f64(b), f64(b * (2 * h + 1)),
            torch.full((b,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    return all(a.cpu().tolist() == [(-99 if k == 0 else 7)] * a.numel() for k, a in enumerate(out))


# the lags of the planted pairs: generic ones, then the places where the neighbourhood crosses something
def edge_lags(n, m2):
    return {"generic": 12345, "negative": -54321, "j2 = 0": 7 * m2, "j2 = M2 - 1": 11 * m2 - 1, "index 0": 0, "index 2N - 1": -1,
            "lag N - 1": n - 1, "lag -N": -n}


# ---- E. the four results are the banded call's ----------------------------------------------------------------------------------

def test_the_four_results_are_the_banded_calls(mod):
    """five pairs on a plan of two pairs a group (three groups; the eight pairs of the edge test below run on two lanes): plain pairs under the full band and a narrow one, a
    broadcast sample, per-pair rows with one that is not a window under both bands; h = 1 and h = 8"""
    n = N
    lags = [12345, -54321, 0, -1, 777]
    src = np.stack([np.roll(track(n), 1000 * k) for k in range(5)])
    smp = np.stack([np.roll(src[k], -l)[:n] for k, l in enumerate(lags)])
    rows = np.array([(-n, n - 1), (-60000, -5), (7, 6), (-3, 3), (100, 5000)], dtype=np.int64)
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        for band in ((0, n), LOW):
            for h in (1, 8):
                for what, (s, t, w) in {"plain": (src, smp, None), "broadcast sample": (src, smp[0], None), "rows": (src, smp, rows),
                                        "one row": (src[0], smp, rows[1])}.items():
                    want = plan.xcorr_phat_f32(s, t, w, band=band)
                    got = plan.xcorr_phat_sub_f32(s, t, w, band=band, half_width=h)
                    assert [a.shape for a in got] == [(5,)] * 4 + [(5, 2 * h + 1), (5,)], what
                    assert [a.dtype for a in got] == [np.int64] + [np.float64] * 4 + [np.int32]
                    assert all_bits(four(got)) == all_bits(want), (band, h, what)
                    if what == "plain":
                        assert got[0].tolist() == lags and got[5].tolist() == [0] * 5, (band, h, got[0])
                    if what == "rows":
                        assert int(got[5][2]) == -2 and np.isnan(got[3][2]) and np.isnan(got[4][2]).all(), got
                        assert not np.isnan(np.delete(got[4], 2, axis=0)).any() and not np.isnan(np.delete(got[3], 2)).any()
        # the full band IS the plain PHAT call
        assert all_bits(four(plan.xcorr_phat_sub_f32(src, smp))) == all_bits(plan.xcorr_phat_f32(src, smp))


def test_the_pool_form_is_the_pool_phat_call(mod):
    """one array of clips as both pools (aliased), listed pairs with repeats over three groups, one row outside its pool and one row
    that is not a window: the four results are the pool PHAT call's bits, near and frac those of the strided sub call on the pair
    alone, NaN for the two refused pairs"""
    n, h = N, 2
    clips = np.stack([np.roll(track(n), 3000 * k) for k in range(3)])
    pairs = np.array([[0, 1], [2, 0], [1, 1], [3, 0], [0, 2], [2, 1], [1, 0]], dtype=np.int32)
    rows = np.tile(np.array([(-n, n - 1)], dtype=np.int64), (7, 1))
    rows[5] = (9, 2)
    with mod.Plan(n, 3, 0) as plan:
        for band in ((0, n), LOW):
            want = plan.xcorr_pool_phat_f32(clips, clips[:, :n], pairs, rows, band)
            got = plan.xcorr_pool_phat_sub_f32(clips, clips[:, :n], pairs, rows, band, h)
            assert all_bits(four(got)) == all_bits(want), band
            assert int(got[5][3]) == -4 and int(got[5][5]) == -2
            for k in (3, 5):
                assert np.isnan(got[3][k]) and np.isnan(got[4][k]).all(), (band, k, got)
            for k in (0, 1, 2, 4, 6):
                a, b = pairs[k]
                one = plan.xcorr_phat_sub_f32(clips[a], clips[b, :n][None, :], band=band, half_width=h)
                assert bits(got, k) == bits(one, 0), (band, k)
                assert int(got[0][k]) == 3000 * (int(a) - int(b)), (band, k, got[0][k])
        every = plan.xcorr_pool_phat_sub_f32(clips, clips[:, :n], half_width=1)
        assert [a.shape for a in every] == [(3, 3)] * 4 + [(3, 3, 3), (3, 3)]
        assert all_bits(four(every)) == all_bits(plan.xcorr_pool_phat_f32(clips, clips[:, :n]))


# ---- F, G. near and frac against the float64 model ------------------------------------------------------------------------------

def check_near_and_frac(got, models, h, what):
    lag, coef, peak, frac, near, ret = got
    again = frac_rule(near, h)
    for k, m in enumerate(models):
        err = float(np.max(np.abs(near[k] - m[5])))
        centre = abs(abs(float(near[k][h])) - float(peak[k]))
        den = phat_sub_model.den_of(*m[5][h - 1:h + 2])
        print("phat sub", what, "pair", k, "lag", int(lag[k]), "model", m[1], "max |near - model|", err, "| |centre| - peak |", centre,
              "frac", float(frac[k]), "model", m[4], "diff", abs(float(frac[k]) - m[4]), "den", den)
        assert (int(ret[k]), int(lag[k])) == (m[0], m[1]), (what, k, lag[k], m[:2])
        assert err <= CURVE_TOL, (what, k, err)
        assert centre <= CURVE_TOL, (what, k, near[k][h], peak[k])
        assert abs(float(frac[k]) - float(again[k])) <= 2.0 ** -50, (what, k, frac[k], again[k])
        assert abs(den) >= DEN_MIN, (what, k, den)        # the chosen pairs are well conditioned (float64, no device involved)
        assert abs(float(frac[k]) - m[4]) <= 3.0 * CURVE_TOL / abs(den), (what, k, frac[k], m[4], den)


@pytest.mark.parametrize("h", [1, 8])
def test_near_and_frac_at_the_edges(mod, h):
    """the peak planted at a row's first and last column, at index 0 and 2N - 1, at lag N - 1 and at lag -N (inside a window that
    holds it), and one negative peak (the sample negated: s = -1); the full band and half the spectrum"""
    n = N
    with mod.Plan(n, 4, 0) as plan:
        m1, m2 = plan.split[0], plan.split[1]
        assert plan.layout == "real-column" and m1 * m2 == n
        names = edge_lags(n, m2)
        lags = list(names.values())
        assert (lags[2] % (2 * n)) % m2 == 0 and (lags[3] % (2 * n)) % m2 == m2 - 1
        signs = [1.0, -1.0] + [1.0] * (len(lags) - 2)
        rows = np.tile(np.array([(-n, n - 1)], dtype=np.int64), (len(lags), 1))
        rows[lags.index(-n)] = (-n, -n + 100)
        smp = np.stack([planted(n, l, s) for l, s in zip(lags, signs)])
        for band in ((0, n), MID):
            models = [model(n, l, s, band, h, tuple(int(v) for v in w)) for l, s, w in zip(lags, signs, rows)]
            assert [m[1] for m in models] == lags, (band, [m[1] for m in models])
            assert models[1][5][h] < 0.0                                       # the negated pair's peak is negative
            got = plan.xcorr_phat_sub_f32(track(n), smp, rows, band=band, half_width=h)
            check_near_and_frac(got, models, h, (n, band, h))
            assert float(got[4][1][h]) < 0.0
            assert all_bits(four(got)) == all_bits(plan.xcorr_phat_f32(track(n), smp, rows, band=band))


def test_near_and_frac_in_the_two_half_row_form(mod):
    """N = 960 000: another M1, 2400-point rows in two halves; a row end, index 2N - 1 and a generic lag, h = 8"""
    n, h = 960000, 8
    with mod.Plan(n, 2, 0) as plan:
        m1, m2 = plan.split[0], plan.split[1]
        assert plan.layout == "real-column" and m1 * m2 == n and m1 != 300
        lags = [5 * m2 - 1, -1, 123457]
        smp = np.stack([planted(n, l) for l in lags])
        band = (0, n)
        models = [model(n, l, 1.0, band, h) for l in lags]
        assert [m[1] for m in models] == lags
        got = plan.xcorr_phat_sub_f32(track(n), smp, band=band, half_width=h)
        check_near_and_frac(got, models, h, (n, band, h))
        assert all_bits(four(got)) == all_bits(plan.xcorr_phat_f32(track(n), smp))


# ---- H. special pairs -----------------------------------------------------------------------------------------------------------

def test_a_silent_pair_and_refused_pairs_leave_their_neighbours_alone(mod):
    n, h = N, 3
    lags = [12345, -54321, 777, 40000]
    smp = np.stack([planted(n, l) for l in lags])
    quiet = smp.copy()
    quiet[1] = 0.0
    full = np.tile(np.array([(-n, n - 1)], dtype=np.int64), (4, 1))
    rows = full.copy()
    rows[2] = (5, 4)
    with mod.Plan(n, 2, 0) as plan:
        base = plan.xcorr_phat_sub_f32(track(n), smp, full, band=LOW, half_width=h)
        got = plan.xcorr_phat_sub_f32(track(n), quiet, rows, band=LOW, half_width=h)
        assert (int(got[0][1]), float(got[2][1]), float(got[3][1]), int(got[5][1])) == (0, 0.0, 0.0, -1), got
        assert (got[4][1] == 0.0).all()
        assert int(got[5][2]) == -2 and np.isnan(got[3][2]) and np.isnan(got[4][2]).all()
        for k in (0, 3):
            assert bits(got, k) == bits(base, k), k
        # the seed of a window that does not hold lag 0: the silent pair's neighbourhood is around it, and still zero
        plan.set_lag_window(100, 5000)
        got = plan.xcorr_phat_sub_f32(track(n), quiet[1], band=LOW, half_width=h)
        assert (int(got[0][0]), float(got[2][0]), float(got[3][0])) == (100, 0.0, 0.0) and (got[4][0] == 0.0).all()
        plan.set_lag_window(-n, n - 1)
        # a pool pair outside its pool (-4) beside valid ones
        clips = np.stack([track(n), np.roll(track(n), 500)])
        pairs = np.array([[0, 1], [0, 2], [1, 0]], dtype=np.int32)
        good = plan.xcorr_pool_phat_sub_f32(clips, clips[:, :n], np.array([[0, 1], [0, 0], [1, 0]], dtype=np.int32), None, LOW, h)
        got = plan.xcorr_pool_phat_sub_f32(clips, clips[:, :n], pairs, None, LOW, h)
        assert int(got[5][1]) == -4 and np.isnan(got[3][1]) and np.isnan(got[4][1]).all() and np.isnan(got[2][1])
        for k in (0, 2):
            assert bits(got, k) == bits(good, k), k
        assert got[0].tolist() == [-500, 0, 500]


# ---- I. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals(mod, torch):
    n = N
    smp = np.stack([planted(n, 12345), planted(n, 777)])
    d_src, d_smp = torch.from_numpy(np.array(track(n))).cuda(), torch.from_numpy(smp).cuda()
    with mod.Plan(n, 2, 0) as plan:
        def call(h, out, drop=None, band=MID, pool=False):
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            if pool:
                plan.xcorr_pool_phat_sub_dev(d_src.data_ptr(), 2 * n, 1, d_smp.data_ptr(), n, 2, 0, 0, 0, 2, *band, h, *ptrs)
            else:
                plan.xcorr_phat_sub_dev(d_src.data_ptr(), 0, d_smp.data_ptr(), n, 0, 0, 2, *band, h, *ptrs)
            plan.sync()

        for pool in (False, True):
            for h in (0, 9, -1, 2 ** 20):
                out = outputs(torch, 2, 8)
                with pytest.raises(mod.AsxError, match="half_width"):
                    call(h, out, pool=pool)
                assert untouched(torch, out), (pool, h)
            out = outputs(torch, 2, 2)
            with pytest.raises(mod.AsxError, match="d_frac"):
                call(2, out, drop=3, pool=pool)
            assert untouched(torch, out), pool
            out = outputs(torch, 2, 2)
            with pytest.raises(mod.AsxError, match="not a band"):
                call(2, out, band=(5, 4), pool=pool)
            assert untouched(torch, out), pool
            out = outputs(torch, 2, 2)
            with pytest.raises(mod.AsxError, match="null"):
                call(2, out, drop=1, pool=pool)                       # a NULL d_coef, the banded call's refusal
            assert untouched(torch, out), pool
            # d_near, d_lag and d_peak may be NULL: the others are written, these keep their sentinels
            out = outputs(torch, 2, 2)
            call(2, out, pool=pool)
            whole = [a.cpu().numpy() for a in out]
            out = outputs(torch, 2, 2)
            call(2, out, drop=4, pool=pool)
            part = [a.cpu().numpy() for a in out]
            assert (part[4] == 7.0).all() and all(part[k].tobytes() == whole[k].tobytes() for k in (0, 1, 2, 3, 5)), pool
            assert whole[0].tolist() == [12345, 777] and not (whole[4] == 7.0).any()
    m = 1000  # a length outside the tuned table: a packed plan
    d_s, d_t = torch.zeros(4 * m, dtype=torch.float32, device="cuda"), torch.zeros(2 * m, dtype=torch.float32, device="cuda")
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        for lo, hi in [(10, 100), (0, m)]:
            out = outputs(torch, 2, 1)
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match="real-column"):
                plan.xcorr_phat_sub_dev(d_s.data_ptr(), 2 * m, d_t.data_ptr(), m, 0, 0, 2, lo, hi, 1, *(a.data_ptr() for a in out))
            assert untouched(torch, out)
            out = outputs(torch, 4, 1)
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match="real-column"):
                plan.xcorr_pool_phat_sub_dev(d_s.data_ptr(), 2 * m, 2, d_t.data_ptr(), m, 2, 0, 0, 0, 4, lo, hi, 1, *(a.data_ptr() for a in out))
            assert untouched(torch, out)
