"""Sub-sample GCC-PHAT (asx_xcorr_phat_sub_f32_dev, asx_xcorr_pool_phat_sub_f32_dev), the parts that need no GPU: the C-ABI and the
built library export both calls, the host checks of the Plan methods raise before anything is uploaded, the float64 model of
tests/phat_sub_model.py follows the header's frac rule and finds fractional pure delays, the single-lag sum that k_phat_near
evaluates is the real-column inverse of tests/model_fourstep.py at every index, and the built library holds one k_phat_near."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import model_fourstep as mf
import phat_band_model
import phat_sub_model
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_phat_sub_f32_dev", "asx_xcorr_pool_phat_sub_f32_dev")


# ---- A. surface -----------------------------------------------------------------------------------------------------------------

def test_the_calls_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS and name in hipxcorr.SIGNATURES, name
        assert hasattr(L, name), name
    assert re.search(r"^#define\s+ASX_NEAR_MAX\s+8\s*$", hdr, flags=re.M)
    assert hipxcorr.NEAR_MAX == 8 == phat_sub_model.NEAR_MAX
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_phat_sub_dev", "xcorr_pool_phat_sub_dev", "xcorr_phat_sub_f32", "xcorr_pool_phat_sub_f32"):
        assert callable(getattr(m.Plan, name)), name
    # the int half_width sits behind the band in both signatures, and the pool form's other arguments are the pool PHAT call's
    sig = hipxcorr.SIGNATURES
    for new, old in zip(CALLS, ("asx_xcorr_phat_band_f32_dev", "asx_xcorr_pool_phat_f32_dev")):
        a, b = sig[new][1], sig[old][1]
        assert len(a) == len(b) + 3 and a[:len(b) - 5] == b[:-5] and a[len(b) - 5] is ctypes.c_int, new


def test_the_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("Sub-sample GCC-PHAT")
    text = flat[at:flat.index("#define ASX_NEAR_MAX", at)]
    for phrase in ("bit for bit", "d_frac must not be NULL", "den = (a - 2 b) + c", "clamped to [-0.5, 0.5]", "lag + frac",
                   "float32 rounding", "biased", "0.14", "index 2N - 1 (lag -1) sits beside index 0", "NaN in frac"):
        assert phrase in text, phrase
    sentence = flat[flat.index("Not offered with PHAT:"):]
    sentence = sentence[:sentence.index(".")]
    assert "top-k" in sentence and "double ABI" in sentence, sentence


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_phat_sub_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_pool_phat_sub_dev(self, *a, **kw):
        raise AssertionError("called")


BAD_HALF_WIDTHS = [dict(half_width=0), dict(half_width=9), dict(half_width=1.5), dict(half_width=True), dict(half_width=-1),
                   dict(half_width=None)]
BAD_BANDS = [dict(band=(-1, 5)), dict(band=(0, 17)), dict(band=(5, 4)), dict(band=(1.0, 4)), dict(band=(True, 4)), dict(band=(1, 2, 3))]


def test_the_strided_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32))
    bad = BAD_HALF_WIDTHS + BAD_BANDS + [
        dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
        dict(source=np.zeros((2, 2, 32), np.float32)), dict(source=np.zeros((0, 32), np.float32), sample=np.zeros((0, 16), np.float32)),
        dict(windows=(1.5, 2)), dict(windows=(0, 1, 2)), dict(windows=[[0, 1]] * 3),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_phat_sub_f32(NoDevice(), **args)
    s, t, w, batch, ss, ts, ws, lo, hi, h = hipxcorr.phat_sub_args(16, good["source"], np.zeros(16), (-3, 3), (np.int64(2), 5), np.int32(8))
    assert (batch, ss, ts, ws, lo, hi, h) == (2, 32, 0, 0, 2, 5, 8) and w.tolist() == [-3, 3] and t.dtype == np.float32
    assert type(lo) is int and type(hi) is int and type(h) is int
    assert hipxcorr.phat_sub_args(16, good["source"], good["sample"])[7:] == (0, 16, 1)


def test_the_pool_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((2, 16), np.float32))
    bad = BAD_HALF_WIDTHS + BAD_BANDS + [
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(windows=(1.5, 2)), dict(windows=[[0, 1]] * 3), dict(pairs=[[0, 1]] * 3, windows=[[0, 1]] * 2),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_phat_sub_f32(NoDevice(), **args)
    out = hipxcorr.pool_phat_sub_args(16, good["sources"], good["samples"], [[0, 1], [7, -1]], None, (2, 5), 3)
    assert out[4:] == (2, 0, 2, 5, 3) and out[2].tolist() == [[0, 1], [7, -1]]
    assert hipxcorr.pool_phat_sub_args(16, good["sources"], good["samples"])[4:] == (4, 0, 0, 16, 1)


# ---- B. the model ---------------------------------------------------------------------------------------------------------------

def test_the_frac_rule_in_its_four_cases():
    f = phat_sub_model.frac_of
    nan = float("nan")
    assert math.isnan(f(nan, 1.0, 0.5)) and math.isnan(f(0.5, nan, 0.5)) and math.isnan(f(0.5, 1.0, nan))
    # den >= 0: a flat top, a silent pair, a centre that is a minimum of the magnitude
    assert f(1.0, 1.0, 1.0) == 0.0 and f(0.0, 0.0, 0.0) == 0.0 and f(0.9, 0.5, 0.9) == 0.0 and f(-0.0, -0.0, 0.0) == 0.0
    # an ordinary peak: the vertex of the parabola through (-1, a), (0, b), (1, c)
    assert f(0.5, 1.0, 0.5) == 0.0
    assert f(0.2, 1.0, 0.6) == 0.5 * (0.2 - 0.6) / ((0.2 - 2.0) + 0.6) and 0.0 < f(0.2, 1.0, 0.6) < 0.5
    assert abs(f(0.6, 1.0, 0.2) + f(0.2, 1.0, 0.6)) < 1e-15
    # clamping: a neighbour above the centre (a lag outside the window may exceed the peak)
    assert f(0.0, 1.0, 1.5) == 0.5 and f(1.5, 1.0, 0.0) == -0.5
    # a negative peak goes through s: the mirrored curve has the same vertex
    assert f(-0.2, -1.0, -0.6) == f(0.2, 1.0, 0.6) and f(-0.6, -1.0, -0.2) == f(0.6, 1.0, 0.2)
    assert f(0.2, -1.0, 0.6) == 0.5 * (-0.2 - -0.6) / ((-0.2 - 2.0) + -0.6) and f(0.2, -1.0, 0.6) < 0.0
    assert phat_sub_model.den_of(0.2, 1.0, 0.6) == (0.2 - 2.0) + 0.6 == phat_sub_model.den_of(-0.2, -1.0, -0.6)


def test_near_is_circular_in_index_space():
    r = np.arange(20.0)
    assert phat_sub_model.near_of(r, 0, 2).tolist() == [18.0, 19.0, 0.0, 1.0, 2.0]
    assert phat_sub_model.near_of(r, 19, 1).tolist() == [18.0, 19.0, 0.0]
    assert phat_sub_model.near_of(r, 10, 1).tolist() == [9.0, 10.0, 11.0]      # index N = lag -N beside index N - 1 = lag N - 1


# the bias table of DESIGN.md ("Sub-sample GCC-PHAT"): measured with this model, N = 6000, p = 777, then written down
BIAS = {((0, 6000), 0.1): 0.0510, ((0, 6000), 0.25): 0.1428, ((0, 6000), 0.4): 0.2941,
        ((100, 2000), 0.1): 0.0947, ((100, 2000), 0.25): 0.2395, ((100, 2000), 0.4): 0.3918}


@pytest.mark.parametrize("band", [(0, 6000), (100, 2000)])
@pytest.mark.parametrize("p", [777, -2500, 0, -1, 5999, -6000])
def test_fractional_pure_delays(band, p):
    """circular delays by p + delta, the phase ramp applied in float64: the integer lag is p, frac has delta's sign and lag + frac is
    nearer the truth than the integer lag; delta = 0 gives frac 0 to rounding.  p covers index 0, 2N - 1, N - 1 and N."""
    n = 6000
    for delta in (-0.4, -0.25, 0.0, 0.25, 0.4):
        src, full = phat_sub_model.delayed_pair(n, p, delta)
        r = phat_band_model.r_phat_band(src, full, *band)
        ret, lag, coef, peak, frac, near = phat_sub_model.model(src, full[:n], *band, 2, r=r)
        print("phat sub model band", band, "p", p, "delta", delta, "lag", lag, "peak", peak, "frac", frac, "error", lag + frac - (p + delta))
        assert lag == p and near.shape == (5,) and abs(near[2]) == peak, (band, p, delta, lag)
        assert near.tolist() == r[(p % (2 * n) + np.arange(-2, 3)) % (2 * n)].tolist()
        if delta == 0.0:
            assert abs(frac) < 1e-9 and abs(peak - 1.0) < 1e-12, (band, p, frac, peak)
        else:
            assert math.copysign(1.0, frac) == math.copysign(1.0, delta) and frac != 0.0, (band, p, delta, frac)
            assert abs(lag + frac - (p + delta)) < abs(delta), (band, p, delta, frac)
            assert abs(abs(frac) - BIAS[band, abs(delta)]) < 5e-4, (band, p, delta, frac)


def test_the_bias_table():
    """the third row of the table, and that the figures the header quotes are the table's"""
    n = 6000
    for (band, delta), want in BIAS.items():
        src, full = phat_sub_model.delayed_pair(n, 777, delta)
        got = phat_sub_model.model(src, full[:n], *band, 1, r=phat_band_model.r_phat_band(src, full, *band))[4]
        print("phat sub bias band", band, "delta", delta, "frac", got)
        assert abs(got - want) < 5e-4, (band, delta, got, want)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for want in BIAS.values():
        assert "%.4f" % want in design, want


# ---- C. the single-lag sum ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("whiten", [False, True])
def test_the_single_lag_sum_is_the_inverse_column_pass(whiten):
    """M1 = 12, M2 = 20 (N = 240): every one of the 2N indices, so every row end and index 0 with both neighbours, against
    rlayout_inv_cols of the same Q to 1e-12 of full scale; whitened, Q is what a PHAT row pass leaves (unit bins, F at the peak)"""
    M1, M2 = 12, 20
    N = M1 * M2
    rng = np.random.default_rng(3)
    src = rng.standard_normal(2 * N)
    smp = np.zeros(2 * N)
    smp[:N] = np.roll(src, -37)[:N] + 0.2 * rng.standard_normal(N)
    Cx, Cy = mf.rlayout_fwd_cols(src, M1, M2), mf.rlayout_fwd_cols(smp, M1, M2)
    if not whiten:
        Q = mf.rlayout_rows(Cx, Cy, M1, M2)
    else:
        F = 2 * N
        f = mf.tw(F, np.arange(M1 + 1)[:, None] * np.arange(M2)[None, :])
        P = np.fft.fft(0.5 * Cx * f, axis=1) * np.conj(np.fft.fft(0.5 * Cy * f, axis=1))
        P = P / np.abs(P)
        Q = np.fft.ifft(P, axis=1) * M2 * np.conj(f)
    want = mf.rlayout_inv_cols(Q, M1, M2)
    scale = float(np.max(np.abs(want)))
    if whiten:
        r = phat_band_model.r_phat_band(src, smp[:N], 0, N) * (2 * N)
        assert np.max(np.abs(want - r)) < 1e-9 * scale      # the Q under test is the whitened spectrum's
    got = np.array([phat_sub_model.single_lag(Q, M1, M2, i) for i in range(2 * N)])
    err = float(np.max(np.abs(got - want))) / scale
    print("single-lag sum whitened", whiten, "worst error of full scale", err)
    assert err < 1e-12
    for idx in (0, 2 * N - 1, M2 - 1, M2, N - 1, N, 2 * M1 * M2 - M2):      # both sides of index 0 and of row ends
        for d in (-1, 0, 1):
            i = (idx + d) % (2 * N)
            assert abs(phat_sub_model.single_lag(Q, M1, M2, i) - want[i]) < 1e-12 * scale, (idx, d)


# ---- D. census ------------------------------------------------------------------------------------------------------------------

def test_one_near_kernel_within_its_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = [(n, r) for n, r in names.items() if re.match(r"(void )?k_phat_near\b", n)]
    assert len(mine) == 1, sorted(n for n, _ in mine)
    (n, r), = mine
    assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    assert len([n for n in names if n.startswith("void k_phat_finalize<")]) == 2
