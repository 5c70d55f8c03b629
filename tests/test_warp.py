"""The warped correlation (asx_xcorr_warp_f32_dev, asx_xcorr_pool_warp_f32_dev), the parts that need no GPU: the float64 model of
tests/warp_model.py is the curve model on the line (0, 0) and the curve at c + b on an integer b, rounds its shift as the header
states and lines up one contiguous range of frames; a planted drifting pair has a coefficient of 1 along its line and next to none at
any constant lag; the header says what the calls promise; the C-ABI and the built library export both calls; the host checks of the
Plan methods raise before anything is uploaded; and the built code object holds two k_warp_dots and one k_warp_final within their
budget."""
import ctypes
import os
import re

import numpy as np
import pytest

import curve_model
import lag_window_model
import oracle
import warp_model
from test_kernel_resources import READELF, demangled, kernels_of
from util import ROOT, asx, graft

CALLS = ("asx_xcorr_warp_f32_dev", "asx_xcorr_pool_warp_f32_dev")


# ---- A. the model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 999, 16])
def test_the_line_0_0_is_the_curve_model_and_the_reference_segment(n):
    src, smp, _ = oracle.synth_pair(11, 2, n, 1)
    for lag in (0, -1, n - 1, -n, n // 3, -(n // 4)):
        got = warp_model.warp(src, smp, lag, 0.0, 0.0, 2)
        r, tol, coef, frac = curve_model.curve(src, smp, lag, 2)
        assert got["r"].tobytes() == r.tobytes() and got["tol"].tobytes() == tol.tobytes(), lag
        assert got["frac"] == frac or (np.isnan(frac) and np.isnan(got["frac"]))
        # V is the reference's segment for the lag: the sample's frames [t0, t1) against the source's [s0, s1)
        _, (s0, s1), (t0, t1) = lag_window_model.wrap(curve_model.index_of(lag, n), n)
        lo, hi = warp_model.valid_range(n, lag, 0.0, 0.0)
        assert hi - lo == s1 - s0 == t1 - t0 == got["len"], (lag, lo, hi)
        if hi > lo:
            assert (lo, hi) == (t0, t1) and lo + lag == s0
            assert abs(got["coef"] - coef[2]) <= got["tol_coef"], (lag, got["coef"], coef[2])
        else:
            assert np.isnan(got["coef"]) and np.isnan(coef[2])


def test_an_integer_b_is_the_curve_at_c_plus_b():
    n = 1000
    src, smp, _ = oracle.synth_pair(12, 2, n, 1)
    for lag, b in ((5, 3.0), (-1, 4.0), (0, -7.0), (n - 3, 2.0), (-n + 1, -1.0), (n // 3, -float(n // 2))):
        got = warp_model.warp(src, smp, lag, 0.0, b, 3)
        target = lag + int(b)
        assert (warp_model.shifts(n, 0.0, b) == int(b)).all()
        if -n <= target <= n - 1:
            r, tol, _, frac = curve_model.curve(src, smp, target, 3, coef=False)
            assert got["r"].tobytes() == r.tobytes() and got["frac"] == frac, (lag, b)
        else:                                                # circular in index space: lag n - 1 and b = 2 meet index n + 1
            want = [curve_model.r_at(src, smp, (curve_model.index_of(lag, n) + int(b) + d) % (2 * n))[0] for d in range(-3, 4)]
            assert got["r"].tolist() == want, (lag, b)


def test_the_shift_rounds_as_the_header_states():
    assert warp_model.shifts(4, 0.0, -2.5).tolist() == [-2] * 4          # floor(-2.5 + 0.5): a half goes up
    assert warp_model.shifts(4, 0.0, 2.5).tolist() == [3] * 4
    assert warp_model.shifts(5, 0.25, 0.25).tolist() == [0, 1, 1, 1, 1]  # 0.25, 0.5, 0.75, 1.0, 1.25 + 0.5, floored
    assert warp_model.shifts(3, -0.5, 0.0).tolist() == [0, 0, -1]
    for n, a, b in ((144000, 2.0 ** -6, 72000.0), (144000, -2.0 ** -6, -72000.0), (1000, 12.0 / 1000, 0.25), (999, -12.0 / 999, -0.75)):
        k = warp_model.shifts(n, a, b)
        assert k.dtype == np.int64
        want = [int(np.floor((np.float64(b) + np.float64(a) * np.float64(i)) + 0.5)) for i in (0, 1, n // 2, n - 1)]
        assert [int(k[i]) for i in (0, 1, n // 2, n - 1)] == want
        step = np.diff(k)
        assert (np.diff(np.arange(n) + k) >= 0).all() and set(np.unique(np.abs(step)).tolist()) <= {0, 1}
        # four consecutive frames hold at most one step; a sweep of 1024 frames spans at most 17
        s = np.abs(step)
        assert (s[:-2] + s[1:-1] + s[2:]).max() <= 1
        assert max(abs(int(k[min(i + 1023, n - 1)] - k[i])) for i in range(0, n, 97)) <= 17
    assert warp_model.valid_line(1000, 2.0 ** -6, -1000.0) and warp_model.valid_line(1000, 0.0, 0.0)
    for a, b in ((np.nextafter(2.0 ** -6, 1.0), 0.0), (0.0, 1000.5), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0),
                 (0.0, -float("inf")), (-0.016, 0.0)):
        assert not warp_model.valid_line(1000, a, b), (a, b)


@pytest.mark.parametrize("n", [1000, 999])
def test_v_is_contiguous_and_as_long_as_stated(n):
    assert warp_model.valid_range(n, -n, 0.0, 0.0) == (0, 0)              # u_n = n - N < 0 for every frame
    assert warp_model.valid_range(n, -n, 0.0, 3.0) == (n - 3, n)          # ... and a positive shift brings the last ones in
    assert warp_model.valid_range(n, n - 1, 0.0, 0.0) == (0, n)           # u_n = n + N - 1 <= 2N - 2
    assert warp_model.valid_range(n, n - 1, 0.0, 3.0) == (0, n - 2)       # u_n = n + N + 2 < 2N: n < N - 2
    lo, hi = warp_model.valid_range(n, n - 1, 2.0 ** -6, n / 2)           # u_n = n + N - 1 + k_n, k_n about N / 2 + n / 64
    k = warp_model.shifts(n, 2.0 ** -6, n / 2)
    assert lo == 0 and hi + n - 1 + k[hi] >= 2 * n > hi - 1 + n - 1 + k[hi - 1]
    lo, hi = warp_model.valid_range(n, -n, -(2.0 ** -6), -n / 2)          # nothing lines up: u_n < 0 throughout
    assert (lo, hi) == (0, 0)
    for lag in range(-n, n, 37):
        for a, b in ((12.0 / n, 0.25), (-12.0 / n, -0.75), (2.0 ** -6, n / 2), (-(2.0 ** -6), -n / 2)):
            lo, hi = warp_model.valid_range(n, lag, a, b)                  # (asserts that V is contiguous)
            assert 0 <= lo <= hi <= n


@pytest.mark.parametrize("n", [1000, 999, 144000])
def test_a_planted_pair_has_its_coefficient_along_the_line_only(n):
    for l0, a, b in warp_model.planted_cases(n)[::1 if n < 144000 else 3]:
        src, smp = warp_model.planted(n, l0, a, b)
        c, length, tol = warp_model.coef(src, smp, l0, a, b)
        lo, hi = warp_model.valid_range(n, l0, a, b)
        assert length == hi - lo >= n // 2 and c >= 1.0 - tol and tol < 1e-8, (n, l0, a, b, c, tol)
        flat = max(curve_model.coef_at(src, smp, i) for i in curve_model.neighbours(l0, n, 8))
        print("planted N", n, "l0", l0, "line", (a, b), "coef along the line", c, "best constant lag within +-8", flat)
        assert flat <= 0.25, (n, l0, a, b, flat)


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
    assert hdr.index("int asx_xcorr_pool_track_f32_dev") < hdr.index("int asx_xcorr_warp_f32_dev") < hdr.index("int asx_xcorr_pool_warp_f32_dev")
    d = re.search(r"^#define\s+ASX_WARP_DRIFT_MAX\s+(\S+)", hdr, flags=re.M)
    assert d and float(d.group(1)) == 2.0 ** -6 == hipxcorr.WARP_DRIFT_MAX == warp_model.DRIFT_MAX
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_warp_dev", "xcorr_pool_warp_dev", "xcorr_warp_f32", "xcorr_pool_warp_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert callable(hipxcorr.warp_args) and callable(hipxcorr.pool_warp_args)
    # (batch, entries, d_center, d_line, line_stride, half_width) then five outputs and the stream, in both
    for name in CALLS:
        a = hipxcorr.SIGNATURES[name][1]
        assert a[-12:-6] == [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], name
        assert a[-6:] == [ctypes.c_void_p] * 6, name
    assert len(hipxcorr.SIGNATURES[CALLS[0]][1]) == 17 and len(hipxcorr.SIGNATURES[CALLS[1]][1]) == 20


def test_the_header_says_what_the_issue_asks_it_to_say():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    at = flat.index("A warped correlation: the exact r and the Pearson coefficient along a drift line")
    text = flat[at:flat.index("int asx_xcorr_pool_warp_f32_dev", at)]
    for phrase in ("packed ones included", "a stride of 0 broadcasts", "1 <= entries <= ASX_TOPK_MAX", "e = i * entries + j",
                   "1 <= half_width <= ASX_NEAR_MAX", "a = d_line[e * line_stride]", "b = d_line[e * line_stride + 1]",
                   "3 passes the track call's d_fit straight in", "2 is a packed array of lines", "0 is one line for every entry",
                   "1 is refused", "read when the kernels run", "k_n = floor((b + a * (double)n) + 0.5)", "no fused multiply-add",
                   "np.floor((b + a * n) + 0.5)", "|a| <= ASX_WARP_DRIFT_MAX and |b| <= N", "n + k_n is non-decreasing",
                   "at most one step", "at most 17 steps", "source[(n + p + d + k_n) mod 2N] * sample[n]", "never negative",
                   "signed and unnormalised", "circular in index space", "N * 2^-53 * sum |products of its terms|",
                   "the parabola rule of asx_xcorr_phat_sub_f32_dev", "u_n = n + c + k_n", "0 <= u_n < 2N", "one contiguous range",
                   "d_len[e] = |V|", "d_len may be NULL", "src/cross_correlation.c:256-271", "src/cross_correlation.c:74-116",
                   "the exact pairwise merge", "NaN when V is empty or a side is constant", "-1 when the coefficient is NaN",
                   "feed asx_results_to_ms_dev as they stand", "-2 for a centre outside [-N, N-1]", "-5 for a line that is not valid",
                   "fewer than two used segments", "-2 takes precedence over -5", "len = 0", "reads nothing", "bit for bit",
                   "line_stride == 1", "batch == 0 returns 0", "allocates nothing", "never synchronises the host",
                   "touches no counter and no bank", "asx_plan_set_qstore", "one-stream-at-a-time", "of the plan's max_batch",
                   "interpolation between frames (nearest frame only", "a coefficient for d != 0", "a piecewise path",
                   "-4 for an entry", "over -2, which is over -5", "never touches, fills or grows the bank", "Real-column plans only"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    minus5 = top[top.index("ret = -5"):]
    assert top.index("ret = -4") < top.index("ret = -5")
    for name in CALLS:
        assert name in minus5, name


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def xcorr_warp_dev(self, *a, **kw):
        raise AssertionError("called")

    def xcorr_pool_warp_dev(self, *a, **kw):
        raise AssertionError("called")


BAD_OPTIONS = [dict(half_width=0), dict(half_width=9), dict(half_width=1.5), dict(half_width=True), dict(half_width=-1),
               dict(half_width=None), dict(half_width=8.0), dict(entries=0), dict(entries=9), dict(entries=2.0), dict(entries=True),
               dict(entries=None)]


def test_the_strided_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32), centers=np.zeros(2, np.int64),
                lines=np.zeros((2, 2)), half_width=4)
    bad = BAD_OPTIONS + [
        dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)), dict(source=np.zeros((3, 32), np.float32)),
        dict(centers=np.zeros(3, np.int64)), dict(centers=np.zeros(2, np.float64)), dict(centers=np.zeros((2, 2), np.int64)),
        dict(lines=np.zeros(1)), dict(lines=np.zeros(4)), dict(lines=np.zeros((2, 1))), dict(lines=np.zeros((2, 4))),
        dict(lines=np.zeros((3, 2))), dict(lines=np.zeros((2, 2, 2))), dict(lines=np.zeros((2, 2), np.complex128)),
        dict(lines=[["a", "b"]] * 2), dict(lines=None), dict(lines=np.float64(0.0)),
        dict(centers=np.zeros((2, 3), np.int64), entries=3, lines=np.zeros((2, 2))),      # lines follow the centres' shape
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_warp_f32(NoDevice(), **args)
    out = hipxcorr.warp_args(16, good["source"], np.zeros(16), [[3, -4, 5], [0, 1, -16]], np.zeros((2, 3, 3), np.float32), np.int32(8), np.int64(3))
    s, t, c, ln, batch, ss, ts, ls, h, entries = out
    assert (batch, ss, ts, ls, h, entries) == (2, 32, 0, 3, 8, 3) and c.dtype == np.int64 and c.shape == (2, 3)
    assert ln.dtype == np.float64 and ln.shape == (2, 3, 3) and ln.flags["C_CONTIGUOUS"] and type(ls) is int and type(h) is int
    assert hipxcorr.warp_args(16, np.zeros(32), np.zeros(16), [1, 2, 3], [1e-4, 0.5])[4:] == (3, 0, 0, 0, 1, 1)      # one line for all
    assert hipxcorr.warp_args(16, np.zeros(32), np.zeros(16), [1, 2, 3], [1e-4, 0.5, 0.1])[7] == 0                   # one fit for all
    assert hipxcorr.warp_args(16, np.zeros(32), np.zeros(16), [1, 2, 3], np.zeros((3, 2)))[7] == 2
    # the values of a line are not checked on the host: it comes back with ret -5
    assert hipxcorr.warp_args(16, np.zeros(32), np.zeros(16), [1], [[float("nan"), 1e9]])[7] == 2


def test_the_pool_method_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((3, 16), np.float32), centers=np.zeros((2, 3), np.int64),
                lines=np.zeros((2, 3, 2)), half_width=4)
    bad = BAD_OPTIONS + [
        dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)), dict(sources=np.zeros((0, 32), np.float32)),
        dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]), dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)),
        dict(centers=np.zeros(6, np.int64)), dict(centers=np.zeros((3, 2), np.int64)), dict(centers=np.zeros((2, 3), np.float32)),
        dict(lines=np.zeros((6, 2))), dict(lines=np.zeros((2, 3, 1))), dict(lines=np.zeros((2, 3))), dict(lines=np.zeros(1)),
        dict(pairs=[[0, 1]] * 4, centers=np.zeros(4, np.int64)),                          # lines still [2, 3, 2]
    ]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_warp_f32(NoDevice(), **args)
    out = hipxcorr.pool_warp_args(16, good["sources"], good["samples"], [[5, 6], [7, 8]], np.zeros((2, 2, 3)), [[0, 1], [7, -1]], 8, 2)
    assert out[5:] == (2, 3, 8, 2) and out[2].tolist() == [[0, 1], [7, -1]] and out[3].tolist() == [[5, 6], [7, 8]]
    out = hipxcorr.pool_warp_args(16, good["sources"], good["samples"], good["centers"], [0.0, 0.0])
    assert out[2] is None and out[5:] == (6, 0, 1, 1)


# ---- C. census --------------------------------------------------------------------------------------------------------------------

def test_two_warp_kernels_and_the_final_within_their_budget():
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    names = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    mine = sorted((n, r) for n, r in names.items() if re.match(r"(void )?k_warp_dots\b", n))
    assert len(mine) == 2 and "AsxAtList" in mine[0][0] and "AsxAtPitch" in mine[1][0], [n for n, _ in mine]
    final = [(n, r) for n, r in names.items() if re.match(r"(void )?k_warp_final\b", n)]
    assert len(final) == 1, [n for n, _ in final]
    assert len([n for n in names if re.match(r"(void )?k_warp_", n)]) == 3
    for n, r in mine + final:
        print(n, r)
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
    assert len([n for n in names if re.match(r"(void )?k_curve_dots\b", n)]) == 2
    assert len([n for n in names if re.match(r"(void )?k_track_dots\b", n)]) == 2
