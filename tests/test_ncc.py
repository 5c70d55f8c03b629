"""Normalised cross-correlation (asx_xcorr_ncc_f32_dev, asx_xcorr_ncc_debug_c_dev), the parts that need no GPU: the float64 model of
tests/ncc_model.py is the reference's Pearson coefficient at every lag 0..N-1, the two fixtures defeat the raw search and not the
normalised one, the header says what the call promises, the C-ABI and the built library export both calls, the host checks raise
before anything is uploaded, and the built code object holds the k_ncc_* kernels within their budget."""
import ctypes
import os
import re

import numpy as np
import pytest

import ncc_model
import oracle
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_ncc_f32_dev", "asx_xcorr_ncc_debug_c_dev")
KERNELS = ("k_ncc_sums", "k_ncc_moments", "k_ncc_table", "k_ncc_peak", "k_ncc_finalize", "k_ncc_invalid")


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 1000])
def test_the_models_curve_is_the_references_coefficient_at_every_lag(n):
    """c[l] with r as the exact time-domain sum against pearson_coefficient() of the reference's segments source[l, l + N) and the
    whole sample (src/cross_correlation.c:264-271), at every lag 0..N-1, within 1e-12"""
    src, smp, _ = oracle.synth_pair(23, 4, n, 1)
    c, vx, vy = ncc_model.curve(src, smp)
    assert c.shape == (n,) and vy > 0 and np.all(vx > 0)
    want = np.array([oracle.pearson_coefficient(src[l:l + n], smp) for l in range(n)])
    err = float(np.max(np.abs(c - want)))
    print("ncc model N", n, "worst |c - pearson_coefficient|", err)
    assert err <= 1e-12
    ret, lag, coef, peak = ncc_model.model(src, smp)
    assert ret == 0 and lag == int(np.argmax(np.abs(c))) and coef == want[lag] and peak == float(np.float32(abs(c[lag])))


def test_the_models_rules_at_the_edges():
    n = 16
    src, smp, _ = oracle.synth_pair(23, 5, n, 1)
    full = ncc_model.model(src, smp)
    assert ncc_model.model(src, smp, row=(full[1], full[1])) == full
    assert ncc_model.model(src, smp, row=(0, n - 1)) == full
    for row in ((-1, 5), (0, n), (7, 3)):
        got = ncc_model.model(src, smp, row=row)
        assert got[:2] == (-2, 0) and got[2] != got[2] and got[3] != got[3]
    # no lag competes: a constant sample, a silent source, one frame
    flat = ncc_model.model(src, np.full(n, 0.25, np.float32), row=(3, 9))
    assert flat[:2] == (-1, 3) and flat[3] == 0.0 and flat[2] != flat[2]
    silent = ncc_model.model(np.zeros(2 * n, np.float32), smp, row=(5, 5))
    assert silent[:2] == (-1, 5) and silent[3] == 0.0
    one = ncc_model.model(np.array([1.0, 2.0], np.float32), np.array([3.0], np.float32))
    assert one[:2] == (-1, 0) and one[3] == 0.0
    # a stretch of silence longer than a window: its lags do not compete, the others do
    quiet = src.copy()
    quiet[4:4 + n + 3] = 0.0
    c, vx, vy = ncc_model.curve(quiet, smp)
    ok = ncc_model.competing(c, vx, vy)
    assert not ok[4:8].any() and ok[:2].all() and ok[9:].all()


@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("name", ["a", "b"])
def test_the_fixtures_defeat_the_raw_search_and_not_the_normalised_one(name, p):
    n = 144000
    src, smp, planted = getattr(ncc_model, "fixture_" + name)(n, p)
    o_ret, o_lag, o_coef, o_r, _ = oracle.cross_correlation(src, smp, want_results=True)
    r = np.asarray(o_r, dtype=np.float64)[:n] / (2 * n)
    raw = int(np.argmax(np.abs(r)))
    cv = ncc_model.curve(src, smp, r=r)
    ok = ncc_model.competing(*cv)
    ret, lag, coef, peak = ncc_model.model(src, smp, c=cv)
    second = ncc_model.runner_up(cv[0], ok, lag)
    print("fixture", name, p, "planted", planted, "oracle", o_lag, "raw argmax", raw, "coefficient there",
          oracle.pearson_coefficient(src[raw:raw + n], smp), "ncc", lag, "|c|", peak, "next best", second)
    assert o_lag != planted and raw != planted
    assert (ret, lag) == (0, planted)
    assert peak - second >= 0.2
    assert abs(coef - cv[0][lag]) <= 1e-9


# ---- B. surface -------------------------------------------------------------------------------------------------------------------

def test_the_calls_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS and name in hipxcorr.SIGNATURES, name
        assert hasattr(L, name), name
    assert re.search(r"^#define\s+ASX_NCC_MIN_ENERGY\s+1e-6\s*$", hdr, flags=re.M)
    assert hipxcorr.NCC_MIN_ENERGY == 1e-6 == ncc_model.MIN_ENERGY == m.NCC_MIN_ENERGY
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_ncc_dev", "xcorr_ncc_f32", "ncc_debug_c_dev"):
        assert callable(getattr(m.Plan, name)), name
    assert callable(hipxcorr.ncc_args) and m.ncc_args is hipxcorr.ncc_args
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_f32_dev"][1]
    assert a[5:9] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double] and a[9:] == [ctypes.c_void_p] * 5
    assert hipxcorr.SIGNATURES["asx_xcorr_ncc_debug_c_dev"][1][3] is ctypes.c_double


def test_the_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("Normalised cross-correlation: the strided batch")
    text = flat[at:flat.index("int asx_xcorr_ncc_debug_c_dev", at)]
    for phrase in ("mu = mean of all 2N source frames", "Sx[l] = sum_{n<N} x[l+n]", "an offset costs no digits",
                   "Vx[l] = sum_{n<N} (x[l+n] - mean_l)^2 = Sxx'[l] - Sx'[l]^2 / N", "Sy, Vy = the same over the sample, about its own mean",
                   "c[l] = (r32[l] / s - Sx[l] * Sy / N) / sqrt(Vx[l] * Vy)", "c32[l] = (float) c[l]",
                   "Only the lags 0 <= l <= N-1 exist", "Negative lags are out of scope", "a second correlation",
                   "Vmax = max of Vx[l] over ALL lags 0..N-1, whatever the window", "Vx[l] >= min_energy * Vmax",
                   "ASX_NCC_MIN_ENERGY (1e-6) <= min_energy <= 1", "may fall on either side", "the largest |c32[l]| wins",
                   "the smallest lag among equal float32 values", "There is no signed seed", "lag = the window's lag_min and peak = 0",
                   "NOT the float64 argmax by construction", "bit for bit", "row [lag, lag]", "(double)|c32[lag]|",
                   "-2 for a row that does not satisfy 0 <= lag_min <= lag_max <= N-1", "ret is never 1", "packed ones included",
                   "d_windows == NULL means every lag 0..N-1", "ignored and left as it is", "d_lag may be NULL", "batch == 0 returns 0",
                   "lists nothing and takes no second look", "asx_plan_peak_overflows", "asx_plan_peak_repairs", "asx_plan_pearson_modes",
                   "asx_plan_prune_stats", "asx_plan_qstore_stats", "asx_plan_workspace_bytes unchanged", "never synchronises the host",
                   "independent of the batch size", "inside a stream capture", "at most 1 GiB"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    sentence = text[text.index("Not offered:"):]
    for word in ("negative lags", "pools", "top-k", "fractional lag", "asx_xcorr_curve_f32_dev", "double ABI", "streams", "fused inverse pass"):
        assert word in sentence, word
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    assert "asx_xcorr_ncc_f32_dev" in top[top.index("ret[i] = -2"):top.index("ret = -3")]


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_ncc_dev(self, *a, **kw):
        raise AssertionError("called")


def test_the_checks_come_before_anything_is_uploaded():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32))
    bad = [dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
           dict(source=np.zeros((2, 2, 32), np.float32)), dict(sample=np.float32(0)),
           dict(min_energy=0), dict(min_energy=1e-7), dict(min_energy=1.5), dict(min_energy=float("nan")), dict(min_energy=None),
           dict(min_energy=True), dict(min_energy="1e-3"),
           dict(windows=np.zeros(3, np.int64)), dict(windows=np.zeros((3, 2), np.int64)), dict(windows=np.zeros((2, 3), np.int64)),
           dict(windows=np.zeros((2, 2), np.float64)), dict(windows=np.zeros((2, 2, 2), np.int64))]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.Plan.xcorr_ncc_f32(NoDevice(), **args)
        with pytest.raises((ValueError, TypeError)):
            hipxcorr.ncc_args(16, **args)
    s, t, w, batch, ss, ts, ws, me = hipxcorr.ncc_args(16, good["source"], np.zeros(16), [[0, 3], [2, 15]], np.float32(0.5))
    assert (batch, ss, ts, ws, me) == (2, 32, 0, 1, 0.5) and type(me) is float and w.dtype == np.int64 and t.dtype == np.float32
    assert hipxcorr.ncc_args(16, np.zeros(32), np.zeros(16))[2:] == (None, 1, 0, 0, 0, 1e-3)
    assert hipxcorr.ncc_args(16, good["source"], good["sample"], [0, 15], 1e-6)[6:] == (0, 1e-6)
    assert hipxcorr.ncc_args(16, good["source"], good["sample"], min_energy=1)[7] == 1.0


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_the_ncc_kernels_are_built_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_ncc_", n)}
    assert sorted(re.match(r"(?:void )?(k_ncc_\w+)", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
