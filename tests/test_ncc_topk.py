"""Top-k and pool forms of the normalised cross-correlation (asx_xcorr_ncc_topk_f32_dev, asx_xcorr_pool_ncc_f32_dev,
asx_xcorr_pool_ncc_topk_f32_dev), the parts that need no GPU: fixture C on the float64 model (three copies of the sample, the
quietest of which the raw top 3 never hold), the rule's edges on hand-made curves, the surface (header, binding, exports), the host
checks, and the census of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import ncc_model
import ncc_topk_model as tm
import oracle
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_ncc_topk_f32_dev", "asx_xcorr_pool_ncc_f32_dev", "asx_xcorr_pool_ncc_topk_f32_dev")
KERNELS = ("k_ncctop_scan", "k_ncctop_step")
MARGIN = 0.1   # between consecutive entries of fixture C and down to the fourth (observed: at least 0.13)
NAN = float("nan")


# ---- A. fixture C on the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0, 1, 2])
@pytest.mark.parametrize("n", [5000, 144000])
def test_fixture_c_on_the_model(n, p):
    src, smp, planted = tm.fixture_c(n, p)
    r = ncc_model.r_plain(src, smp)
    cv = ncc_model.curve(src, smp, r=r)
    sep = n // 100
    top = tm.topk(*cv, 4, sep)
    print("fixture c", n, p, "planted", planted, "model", top, "min Vx / Vmax", float(np.min(cv[1]) / np.max(cv[1])))
    assert [e[0] for e in top] == [0] * 4
    assert tuple(e[1] for e in top[:3]) == planted
    for a, b in zip(top[:3], top[1:]):
        assert a[2] - b[2] >= MARGIN, top
    assert ncc_model.ratio_clear(cv[1], ncc_model.DEFAULT_ENERGY)
    # the raw search: the top 3 of |r| under the same separation hold the two louder copies and never the 0.3 copy
    a = np.abs(r)
    raw = []
    for _ in range(3):
        lag = int(np.argmax(a))
        raw.append(lag)
        a[max(0, lag - sep):lag + sep + 1] = -1.0
    print("fixture c", n, p, "raw top 3", raw)
    assert planted[0] in raw and planted[1] in raw
    assert all(abs(lag - planted[2]) > sep for lag in raw), (raw, planted)


# ---- B. the rule's edges on hand-made curves --------------------------------------------------------------------------------------

def keys(*values):
    return np.array(values, dtype=np.float32)


def test_min_separation_zero_leaves_out_the_entries_alone():
    k = keys(0.1, 0.9, 0.8, 0.7, 0.2)
    assert tm.topk_of_keys(k, 3, 0) == [(0, 1, float(k[1])), (0, 2, float(k[2])), (0, 3, float(k[3]))]
    got = tm.topk_of_keys(k, 3, 1)
    assert got[:2] == [(0, 1, float(k[1])), (0, 3, float(k[3]))] and got[2][:2] == (-3, 0) and got[2][2] != got[2][2]


def test_zones_are_clipped_at_the_rows_ends():
    k = keys(0.9, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.95)
    # row [2, 7]: the zone around 7 ends at 7, the one around 2 starts inside the row: lags 0 and 1 never compete
    assert [e[:2] for e in tm.topk_of_keys(k, 3, 2, row=(2, 7))] == [(0, 7), (0, 4), (-3, 0)]
    assert [e[:2] for e in tm.topk_of_keys(k, 4, 1, row=(2, 7))] == [(0, 7), (0, 5), (0, 3), (-3, 0)]
    # a separation past both ends: one entry
    assert [e[:2] for e in tm.topk_of_keys(k, 2, 100)] == [(0, 7), (-3, 0)]


def test_an_empty_set_gives_minus_three_from_there_on():
    k = keys(0.5, 0.4, 0.3)
    got = tm.topk_of_keys(k, 4, 1)
    assert [e[:2] for e in got] == [(0, 0), (0, 2), (-3, 0), (-3, 0)]
    assert all(e[2] != e[2] for e in got[2:])
    # a row narrower than 2 min_separation + 1 around its best lag
    assert [e[0] for e in tm.topk_of_keys(keys(0.1, 0.9, 0.2), 2, 1)] == [0, -3]


def test_a_set_with_no_competing_lag_gives_its_smallest_lag_and_peak_zero():
    k = keys(NAN, NAN, NAN, NAN, NAN, NAN)
    assert tm.topk_of_keys(k, 3, 1) == [(0, 0, 0.0), (0, 2, 0.0), (0, 4, 0.0)]
    assert [e[:2] for e in tm.topk_of_keys(k, 3, 1, row=(1, 4))] == [(0, 1), (0, 3), (-3, 0)]
    # one competing lag: it wins, then the smallest lags left
    k[3] = 0.25
    assert tm.topk_of_keys(k, 3, 1) == [(0, 3, 0.25), (0, 0, 0.0), (0, 5, 0.0)]


def test_equal_values_take_the_smallest_lag():
    k = keys(0.2, 0.7, 0.1, 0.7, 0.1, 0.7)
    assert [e[1] for e in tm.topk_of_keys(k, 3, 1)] == [1, 3, 5]
    assert [e[1] for e in tm.topk_of_keys(k, 2, 0, row=(2, 5))] == [3, 5]


def test_one_frame_and_rows_that_are_not_rows():
    one = tm.topk(*ncc_model.curve(np.array([1.0, 2.0], np.float32), np.array([3.0], np.float32)), 2, 0)
    assert one[0] == (0, 0, 0.0) and one[1][:2] == (-3, 0)
    for row in ((-1, 2), (0, 5), (3, 1)):
        got = tm.topk_of_keys(keys(0.1, 0.2, 0.3, 0.4, 0.5), 3, 0, row=row)
        assert [e[:2] for e in got] == [(-2, 0)] * 3 and all(e[2] != e[2] for e in got)


def test_the_rule_with_k_one_is_the_one_lag_model():
    n = 16
    src, smp, _ = oracle.synth_pair(23, 5, n, 1)
    cv = ncc_model.curve(src, smp)
    for row in (None, (3, 9), (7, 7)):
        ret, lag, _, peak = ncc_model.model(src, smp, row=row, c=cv)
        assert tm.topk(*cv, 1, 5, row=row) == [(0, lag, peak)] and ret == 0


# ---- C. surface -------------------------------------------------------------------------------------------------------------------

def test_the_calls_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS and name in hipxcorr.SIGNATURES, name
        assert hasattr(L, name), name
    assert hasattr(L, "asx_plan_debug_ncc") and "asx_plan_debug_ncc" in hipxcorr.SIGNATURES
    assert "asx_plan_debug_ncc" not in hdr and "asx_plan_debug_ncc" not in hipxcorr.ABI_SYMBOLS
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_ncc_topk_dev", "xcorr_pool_ncc_dev", "xcorr_pool_ncc_topk_dev", "xcorr_ncc_topk_f32", "xcorr_pool_ncc_f32",
                 "xcorr_pool_ncc_topk_f32", "debug_ncc"):
        assert callable(getattr(m.Plan, name)), name
    for name in ("ncc_topk_args", "pool_ncc_args", "pool_ncc_topk_args"):
        assert getattr(m, name) is getattr(hipxcorr, name), name
    vp, sz, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    a = hipxcorr.SIGNATURES["asx_xcorr_ncc_topk_f32_dev"][1]
    assert a[:9] == hipxcorr.SIGNATURES["asx_xcorr_ncc_f32_dev"][1][:9] and a[9:] == [ctypes.c_int, ctypes.c_int64] + [vp] * 5
    b = hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_f32_dev"][1]
    assert b[:11] == hipxcorr.SIGNATURES["asx_xcorr_pool_f32_dev"][1][:11] and b[11:] == [dbl] + [vp] * 5
    c = hipxcorr.SIGNATURES["asx_xcorr_pool_ncc_topk_f32_dev"][1]
    assert c[:12] == b[:12] and c[12:] == [ctypes.c_int, ctypes.c_int64] + [vp] * 5 and sz in c


def test_the_header_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("The K strongest separated lags of the coefficient curve per pair")
    text = flat[at:flat.index("int asx_xcorr_pool_ncc_topk_f32_dev", at)]
    for phrase in ("those of asx_xcorr_ncc_f32_dev, word for word", "Vmax is over all lags 0..N-1, whatever the window and the zones",
                   "Entry j (0-based) of pair i is at index i*k + j of d_lag, d_coef, d_peak and d_ret",
                   "1 <= k <= ASX_TOPK_MAX (8) and min_separation >= 0", "A_0 is the set of lags of the pair's row",
                   "the plan's window is ignored", "|l - lag_i| <= min_separation for an earlier entry i < j",
                   "the largest |c32| among the competing lags of A_j wins", "the smallest lag among equal float32 values",
                   "there is no signed seed", "peak = (double)|c32[lag]|", "row [lag, lag]", "-1 for a NaN coefficient",
                   "lag = the smallest lag of A_j, peak = 0", "The zone around that lag is taken like any other",
                   "entry j and every later entry are (0, NaN, peak NaN, -3)", "(0, NaN, NaN, -2) in all k entries",
                   "ret is never 1", "k = 1 launches exactly asx_xcorr_ncc_f32_dev", "Entry 0 is always bit for bit the k = 1 result",
                   "float32 argmax of each pass", "d_lag may be NULL", "batch == 0 returns 0", "asynchronous and capturable",
                   "the upper half of the group's r", "at most 7 zones",
                   "Everything before `batch` means what it means in asx_xcorr_pool_f32_dev", "Real-column plans only",
                   "once per call", "bit for bit those of asx_xcorr_ncc_f32_dev for that pair alone on the same plan",
                   "the bank gives the same float32 Q, so the same r32, and the moment trees are fixed by N",
                   "(0, NaN, NaN, -4)", "It takes precedence over -2", "nothing outside the pools is read",
                   "every refusal of asx_xcorr_pool_f32_dev", "16N bytes per source track, plus the chunk sums", "grows like the bank",
                   "never inside a stream capture", "not counted in asx_plan_workspace_bytes",
                   "k = 1 launches exactly asx_xcorr_pool_ncc_f32_dev",
                   "bit for bit those of asx_xcorr_ncc_topk_f32_dev for that pair alone on the same plan",
                   "(0, NaN, NaN, -4) in all k entries; it takes precedence over -2 and -3", "asx_pool_closure_dev",
                   "a pair whose true lag is negative has no entry to offer"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    for name in CALLS[::2]:
        assert name in top[top.index("ret = -3"):top.index("ret = -5")], name
    assert "asx_xcorr_pool_ncc_f32_dev" in top[top.index("ret = -4"):top.index("ret = -5")]
    ncc = flat[flat.index("Normalised cross-correlation: the strided batch"):at]
    assert "asx_xcorr_ncc_topk_f32_dev" in ncc[ncc.index("Not offered:"):]


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def _called(self, *a, **kw):
        raise AssertionError("called")

    xcorr_ncc_topk_dev = xcorr_pool_ncc_dev = xcorr_pool_ncc_topk_dev = _called


def test_the_checks_come_before_anything_is_uploaded():
    asx()
    from audiosync_amd import hipxcorr
    strided = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32), k=3, min_separation=2)
    pools = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((3, 16), np.float32))
    option = [dict(k=0), dict(k=9), dict(k=True), dict(k=2.0), dict(min_separation=-1), dict(min_separation=1.5)]
    energy = [dict(min_energy=0), dict(min_energy=1e-7), dict(min_energy=1.5), dict(min_energy=float("nan")), dict(min_energy=None),
              dict(min_energy=True)]
    cases = [(hipxcorr.Plan.xcorr_ncc_topk_f32, hipxcorr.ncc_topk_args, strided,
              option + energy + [dict(source=np.zeros(31, np.float32)), dict(windows=np.zeros((3, 2), np.int64))]),
             (hipxcorr.Plan.xcorr_pool_ncc_f32, hipxcorr.pool_ncc_args, pools,
              energy + [dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((0, 16), np.float32)),
                        dict(pairs=np.zeros((2, 3), np.int32)), dict(pairs=np.zeros((2, 2))), dict(windows=np.zeros((5, 2), np.int64))]),
             (hipxcorr.Plan.xcorr_pool_ncc_topk_f32, hipxcorr.pool_ncc_topk_args, dict(pools, k=2, min_separation=0),
              option + energy + [dict(samples=np.zeros((3, 15), np.float32)), dict(pairs=[[0, 2 ** 31]])])]
    for method, args_of, good, bad in cases:
        for kw in bad:
            args = dict(good)
            args.update(kw)
            with pytest.raises((ValueError, TypeError)):
                method(NoDevice(), **args)
            with pytest.raises((ValueError, TypeError)):
                args_of(16, **args)
    got = hipxcorr.ncc_topk_args(16, strided["source"], np.zeros(16), 3, np.int64(2), [[0, 3], [2, 15]], 0.5)
    assert got[3:] == (2, 32, 0, 1, 0.5, 3, 2) and type(got[9]) is int and got[2].dtype == np.int64 and got[1].dtype == np.float32
    s, t, pr, w, batch, ws, me = hipxcorr.pool_ncc_args(16, pools["sources"], pools["samples"])
    assert (pr, w, batch, ws, me) == (None, None, 6, 0, 1e-3) and type(me) is float
    assert hipxcorr.pool_ncc_topk_args(16, pools["sources"], pools["samples"], 8, 0, [[1, 2]], [0, 15], 1e-6)[4:] == (1, 0, 1e-6, 8, 0)


# ---- D. census --------------------------------------------------------------------------------------------------------------------

def test_the_new_kernels_need_no_private_segment():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = {n: r for n, r in names.items() if re.match(r"(void )?k_ncc", n)}
    found = sorted(re.match(r"(?:void )?(k_ncc\w+)", n).group(1) for n in mine)
    for k in KERNELS + ("k_ncc_peak",):
        assert found.count(k) == 1, (k, found)
    for n, r in mine.items():
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
