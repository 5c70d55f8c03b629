"""The lag track (asx_xcorr_track_f32_dev, asx_xcorr_pool_track_f32_dev), the parts that need no GPU: the float64 model of
tests/track_model.py adds up over its segments to the curve model's r, cuts the segments by the b_s rule, picks peaks and fits the line
as the header states; the header says what the calls promise; the C-ABI and the built library export both calls; the host checks of the
Plan methods raise before anything is uploaded; and the built code object holds two k_track_dots and one k_track_fit within their
budget."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import curve_model
import oracle
import track_model
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_track_f32_dev", "asx_xcorr_pool_track_f32_dev")


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, segments, h", [(1000, 8, 9), (999, 8, 3), (1000, 64, 2), (16, 16, 1)])
def test_the_segments_add_up_to_the_curve_models_r(n, segments, h):
    """both sides are correctly rounded sums of the same exact products: they differ by the roundings of the S segment values and of
    their sum, which the segments' tolerances cover many times over"""
    src, smp, _ = oracle.synth_pair(11, 2, n, 1)
    for lag in (0, -1, n - 1, -n, n // 3):
        r, tol = track_model.track_r(src, smp, lag, h, segments)
        assert r.shape == tol.shape == (segments, 2 * h + 1)
        for j, idx in enumerate(track_model.indices(lag, n, h)):
            want, sum_abs = curve_model.r_at(src, smp, idx)
            assert abs(math.fsum(r[:, j]) - want) <= math.fsum(tol[:, j]), (lag, j)
            assert math.fsum(tol[:, j]) <= curve_model.tolerance(n, sum_abs) * (1 + 1e-12)
    assert track_model.indices(0, n, 2) == [2 * n - 2, 2 * n - 1, 0, 1, 2]
    assert track_model.indices(-n, n, 1) == [n - 1, n, n + 1]


@pytest.mark.parametrize("n, segments", [(999, 8), (1000, 64), (1000, 1), (64, 64), (144000, 16)])
def test_the_segment_bounds(n, segments):
    b = track_model.bounds(n, segments)
    assert b[0] == 0 and b[-1] == n and len(b) == segments + 1
    assert b == [int(np.int64(s) * np.int64(n) // np.int64(segments)) for s in range(segments + 1)]
    lens = [b[s + 1] - b[s] for s in range(segments)]
    assert min(lens) >= 1 and max(lens) - min(lens) <= 1 and sum(lens) == n
    t = track_model.times(n, segments)
    for s in range(segments):
        assert t[s] == float(np.mean(np.arange(b[s], b[s + 1]))) and t[s] * 2 == b[s] + b[s + 1] - 1
    if (n, segments) == (999, 8):
        assert b == [0, 124, 249, 374, 499, 624, 749, 874, 999]
    if (n, segments) == (1000, 64):
        assert b[:5] == [0, 15, 31, 46, 62] and lens.count(16) == 40 and lens.count(15) == 24
    with pytest.raises(AssertionError):
        track_model.bounds(n, 65)
    with pytest.raises(AssertionError):
        track_model.bounds(3, 4)


@pytest.mark.parametrize("a, rho", [(0.25, 40e-6), (-3.5, -1e-4), (0.0, 0.0), (12.0, 3e-3)])
def test_an_exact_line_gives_its_slope(a, rho):
    n, segments = 144000, 16
    t = track_model.times(n, segments)
    off = [a + rho * x for x in t]
    w = list(np.random.default_rng(3).uniform(0.5, 2.0, segments))
    used = [True] * segments
    f = track_model.fit(t, off, w, used)
    td, tl, tr = track_model.fit_tolerances(t, off, w, used, f, segments)
    assert abs(f["drift"] - rho) <= td and abs(f["lag0"] - a) <= tl and f["rms2"] <= tr, (f, td, tl, tr)
    assert td < 1e-3 * max(abs(rho), 1e-6) and f["count"] == segments
    # a segment that is not used plays no part, whatever it holds
    used[5], off[5], w[5] = False, 1e9, 1e9
    g = track_model.fit(t, off, w, used)
    assert abs(g["drift"] - rho) <= td and g["count"] == segments - 1


def test_peaks_edges_ties_and_too_few_segments():
    h = 2
    rule = track_model.seg_rule
    assert rule([0.0] * 5, h) == (-2.0, 0.0, False)                         # all zero: d = -h, an edge
    assert rule([5.0, 1.0, 1.0, 1.0, 1.0], h) == (-2.0, 5.0, False)         # the lower edge
    assert rule([1.0, 1.0, 1.0, 1.0, -5.0], h) == (2.0, 5.0, False)         # the upper edge, by |r|
    assert rule([0.0, 3.0, 1.0, -3.0, 0.0], h)[:2] == (-1.0 + track_model.phat_sub_model.frac_of(0.0, 3.0, 1.0), 3.0)   # smallest d wins
    off, w, used = rule([0.0, 1.0, -4.0, 2.0, 0.0], h)
    assert used and w == 4.0 and off == 0.0 + track_model.phat_sub_model.frac_of(1.0, -4.0, 2.0) and abs(off) <= 0.5
    assert rule([0.0, 1.0, 4.0, float("nan"), 0.0], h)[2] is False           # an interior peak, a value that is not finite
    assert rule([0.0, float("inf"), 4.0, 1.0, 0.0], h)[2] is False
    seg, used = track_model.seg_of([[0.0, 1.0, 4.0, 1.0, 0.0], [0.0] * 5, [9.0, 1.0, 4.0, 1.0, 0.0]], h)
    assert used.tolist() == [True, False, False] and seg.tolist() == [[0.0, 4.0], [-2.0, 0.0], [-2.0, 9.0]]
    t = track_model.times(30, 3)
    f = track_model.fit(t, seg[:, 0], seg[:, 1], used)
    assert f["count"] == 1 and all(math.isnan(f[k]) for k in ("drift", "lag0", "rms"))
    f = track_model.fit(t, seg[:, 0], seg[:, 1], [False] * 3)
    assert f["count"] == 0 and math.isnan(f["drift"])
    f = track_model.fit(t, [1.0, 7.0, 2.0], [1.0, 1.0, 3.0], [True, False, True])
    assert f["count"] == 2 and abs(f["drift"] - 1.0 / (t[2] - t[0])) < 1e-15 and f["rms"] < 1e-12


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
    assert re.search(r"^#define\s+ASX_TRACK_HALF_MAX\s+64\s*$", hdr, flags=re.M)
    assert re.search(r"^#define\s+ASX_TRACK_SEG_MAX\s+64\s*$", hdr, flags=re.M)
    assert hipxcorr.TRACK_HALF_MAX == 64 == track_model.HALF_MAX and hipxcorr.TRACK_SEG_MAX == 64 == track_model.SEG_MAX
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_track_dev", "xcorr_pool_track_dev", "xcorr_track_f32", "xcorr_pool_track_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert callable(hipxcorr.track_args) and callable(hipxcorr.pool_track_args)
    # (batch, entries, d_center, half_width, segments) then five float64 / int32 outputs and the stream, in both
    for name in CALLS:
        a = hipxcorr.SIGNATURES[name][1]
        assert a[-11:-6] == [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int], name
        assert a[-6:] == [ctypes.c_void_p] * 6, name


def test_the_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("A lag track: the exact r per time segment around given lags, and a drift fit")
    text = flat[at:flat.index("int asx_xcorr_pool_track_f32_dev", at)]
    for phrase in ("packed ones included", "a stride of 0 broadcasts", "1 <= entries <= ASX_TOPK_MAX", "e = i * entries + j",
                   "1 <= half_width <= ASX_TRACK_HALF_MAX", "1 <= segments <= min(ASX_TRACK_SEG_MAX, N)",
                   "b_s = floor(s * N / S) in 64-bit integers", "t_s = (b_s + b_{s+1} - 1) / 2",
                   "d_r[(e * S + s) * n + (d + h)] = r_s[d]", "signed and unnormalised", "circular in index space",
                   "len_s * 2^-53 * sum |products of its terms|", "add up to the curve call's r[(p + d) mod 2N]",
                   "d_seg[(e * S + s) * 2 + {0, 1}] = {off_s, w_s}", "a strict >", "the smallest d wins ties",
                   "an all-zero segment gives -h", "off_s = (double)m_s + frac", "off_s = -h or +h exactly", "d_seg may be NULL",
                   "a caller can fit robustly themselves", "d_used[e] = the number of used segments",
                   "d_fit[e * 3 + {0, 1, 2}] = {drift, lag0, rms}", "in ascending s", "drift = Sty / Stt", "lag0 = ybar - drift * tbar",
                   "With fewer than two used segments all three are NaN", "a wide curve with no fit",
                   "n + center + lag0 + drift * n", "1e6 * drift is the clock offset in ppm", "a segment smears by drift * N / S frames",
                   "-2 for a centre outside [-N, N-1]", "used = 0", "reads nothing", "bit for bit", "batch == 0 returns 0",
                   "allocates nothing", "never synchronises the host", "touches no counter and no bank", "asx_plan_set_qstore",
                   "one-stream-at-a-time", "of the plan's max_batch", "fixed by N, S and h alone", "-4 for an entry", "over -2",
                   "never touches, fills or grows the bank", "Real-column plans only"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    minus2 = top[top.index("ret[i] = -2"):top.index("ret = -3")]
    minus4 = top[top.index("ret = -4"):]
    for name in CALLS:
        assert name in minus2 and (name in minus4) == name.startswith("asx_xcorr_pool"), name


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_track_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_pool_track_dev(self, *a, **kw):
        raise AssertionError("called")


BAD_OPTIONS = [dict(half_width=0), dict(half_width=65), dict(half_width=1.5), dict(half_width=True), dict(half_width=-1),
               dict(half_width=None), dict(half_width=8.0), dict(segments=0), dict(segments=65), dict(segments=17), dict(segments=2.0),
               dict(segments=True), dict(segments=None), dict(segments=-1), dict(entries=0), dict(entries=9), dict(entries=2.0),
               dict(entries=True), dict(entries=None)]


def test_the_strided_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32), centers=np.zeros(2, np.int64), half_width=4,
                segments=4)
    bad = BAD_OPTIONS + [
        dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
        dict(centers=np.zeros(3, np.int64)), dict(centers=np.zeros((2, 2), np.int64)), dict(centers=np.zeros(2, np.float64)),
        dict(centers=np.zeros((2, 3), np.int64), entries=2), dict(centers=np.zeros(2, np.int64), entries=2),
        dict(centers=np.zeros((2, 1, 1), np.int64)), dict(centers=[True, False]), dict(centers=np.int64(0)),
        dict(source=np.zeros(32, np.float32), sample=np.zeros(16, np.float32), centers=np.zeros(0, np.int64)),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_track_f32(NoDevice(), **args)
    out = hipxcorr.track_args(16, good["source"], np.zeros(16), [[3, -4, 5], [0, 1, -16]], np.int32(64), np.int64(16), np.int64(3))
    s, t, c, batch, ss, ts, h, segs, entries = out
    assert (batch, ss, ts, h, segs, entries) == (2, 32, 0, 64, 16, 3) and c.dtype == np.int64 and c.shape == (2, 3) and t.dtype == np.float32
    assert type(h) is int and type(segs) is int and type(entries) is int
    assert hipxcorr.track_args(16, np.zeros(32), np.zeros(16), [1, 2, 3], 1, 1)[3:] == (3, 0, 0, 1, 1, 1)
    # segments may not exceed N, whatever TRACK_SEG_MAX says
    assert hipxcorr.track_args(64, np.zeros(128), np.zeros(64), [0], 1, 64)[7] == 64
    with pytest.raises(ValueError):
        hipxcorr.track_args(63, np.zeros(126), np.zeros(63), [0], 1, 64)


def test_the_pool_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((3, 16), np.float32), centers=np.zeros((2, 3), np.int64),
                half_width=4, segments=4)
    bad = BAD_OPTIONS + [
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(centers=np.zeros(6, np.int64)), dict(centers=np.zeros((3, 2), np.int64)), dict(centers=np.zeros((2, 3), np.float32)),
        dict(pairs=[[0, 1]] * 4, centers=np.zeros((2, 3), np.int64)), dict(centers=np.zeros((2, 3, 2), np.int64)),
        dict(centers=np.zeros((2, 3), np.int64), entries=2),
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_track_f32(NoDevice(), **args)
    out = hipxcorr.pool_track_args(16, good["sources"], good["samples"], [[5, 6], [7, 8]], 33, 16, [[0, 1], [7, -1]], 2)
    assert out[4:] == (2, 33, 16, 2) and out[2].tolist() == [[0, 1], [7, -1]] and out[3].tolist() == [[5, 6], [7, 8]]
    assert hipxcorr.pool_track_args(16, good["sources"], good["samples"], np.zeros((2, 3, 4), np.int32), 1, 1, entries=4)[4:] == (6, 1, 1, 4)
    assert hipxcorr.pool_track_args(16, good["sources"], good["samples"], good["centers"], 1, 1)[2] is None


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_two_track_kernels_and_the_fit_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = sorted((n, r) for n, r in names.items() if re.match(r"(void )?k_track_dots\b", n))
    assert len(mine) == 2 and "AsxAtList" in mine[0][0] and "AsxAtPitch" in mine[1][0], [n for n, _ in mine]
    fit = [(n, r) for n, r in names.items() if re.match(r"(void )?k_track_fit\b", n)]
    assert len(fit) == 1, [n for n, _ in fit]
    for n, r in mine + fit:
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    assert len([n for n in names if re.match(r"(void )?k_curve_dots\b", n)]) == 2
