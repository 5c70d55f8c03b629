"""The sliding-window calls (curve, track, warp) at the lengths their block and sweep arithmetic tells apart.

k_curve_dots, k_track_dots and k_warp_dots share one sweep (csrc/xcorr_kernels.hip: sweep_samples, sweep_fill, sweep_dots) of
ASX_CURVE_SWEEP = 1024 frames, over asx_curve_blocks / asx_track_blocks / asx_warp_blocks blocks per entry.  The three files that
test those calls run at N = 1000, 999 and 144 000: one partial sweep in one block, or whole sweeps in blocks of equal chunks.  Here:

    N = 1, 2, 3, 7            2N < 2h + 1: the stretch wraps the source more than once; N < 4: no 16-byte load is legal; a track
                              with S = N (segments of one frame) and with h = 64 (eight lag tiles); warp lines (0, +-N)
    N = 1023, 1024, 1025, 1027  a sweep short by one; exactly one; one full sweep and a tail of 1 and of 3 frames
    N = 4099                  four full sweeps and a 3-frame tail in one block that writes its own results
    N = 120 011               curve and warp both take 2 blocks (chunk 60 008, the second block 60 003 frames); track with S = 1,
                              h = 8 takes 2 blocks per segment
    N = 1 440 000             curve 31 blocks (chunk 46 452, last 46 440), warp 22 blocks (chunk 65 456, last 65 424), track S = 7
                              (segment bounds that are no multiples of 4), h = 1, 4 blocks per segment

test_the_partition_is_the_one_this_file_covers asserts those block counts and chunks, from the rule of asx_pearson_blocks and
against the library's own functions, so that a change of the partition fails here instead of silently changing what is covered.

The assertions are those of test_gpu_curve.py, test_gpu_track.py and test_gpu_warp.py: every r within len * 2^-53 * sum |products|
of the float64 model's math.fsum (len = N, or the segment's length; the first-order bound of any float64 summation order, derived
and not measured); frac and seg the header's rule on the call's own r, bit for bit; the track's fit within
track_model.fit_tolerances; the warp's coef within warp_model.tol_coef and len = |V|; the coefficient curve within 1e-5 of
curve_model.coef_at and bit for bit the windowed call at [l, l] under the direct form.  Invariants at every length: an entry's bytes
depend on neither its batch nor its place in it (alone against sixth of nine on a plan with max_batch = 2); the track with S = 1,
h = 8 is the curve call's r byte for byte; the warp on the line (0, 0) is the curve call (byte for byte where both take one block,
within the sum of both tolerances otherwise); on packed plans a pair at a float-aligned but not 16-byte aligned address gives the
aligned call's bytes, in all three calls.  At N = 1 440 000 the model runs at h = 1 for two centres (it takes 0.3 s per value
there); every centre still runs on the device for the rules and the invariants.  Nothing else is left out: at every other length
the model covers every centre, every column of r and of the coefficient curve, and every warp line of warp_cases.  (The track with
S = 1, h = 8 at the two longest lengths is held to the curve call's bytes, whose r is modelled, not modelled a second time.)

Measured worst |error| / tolerance per length on an MI355X (h = 8; N = 1 440 000: h = 1).  r of the curve call; r of the track
at the length's own (S, h); r and coef of the warp; the warp on (0, 0) against the curve call, of the sum of both tolerances:
    N          curve r    track r (S, h)         warp r     warp coef   warp - curve
    1, 2       0          0 (N, 64)              0          0           the same bytes
    3          0          0 (3, 64)              0          3.7e-3      the same bytes
    7          0          0 (7, 64)              0          2.0e-3      the same bytes
    1023       1.5e-4     7.5e-4 (3, 9)          2.9e-4     1.2e-4      the same bytes
    1024       1.5e-4     7.4e-4 (3, 9)          2.9e-4     3.0e-4      the same bytes
    1025       9.1e-4     4.7e-3 (3, 9)          9.1e-4     1.5e-4      the same bytes
    1027       8.9e-4     4.0e-3 (3, 9)          8.9e-4     3.6e-6      the same bytes
    4099       2.2e-4     1.0e-3 (3, 9)          2.2e-4     1.7e-4      the same bytes
    120 011    2.7e-7     5.2e-5 (5, 9)          2.5e-7     1.8e-4      0 (two blocks either way)
    1 440 000  4.7e-9     5.7e-6 (7, 1)          7.0e-9     1.4e-9      5.8e-9
(at N <= 7 every sum has so few terms that the device's order gives the correctly rounded value; the coefficient curve is within
4.9e-14 of the float64 oracle at every length; the track with S = 1, h = 8 has the curve call's bytes and no figure of its own)
"""
import ctypes
import math

import numpy as np
import pytest

import curve_model
import track_model
import warp_model
from test_gpu_curve import delays, dev_curve, frac_rule, pair, same
from test_gpu_track import check_seg_and_fit, dev_track
from test_gpu_warp import dev_warp
from util import asx

pytestmark = pytest.mark.gpu

TINY = (1, 2, 3, 7)
LENGTHS = TINY + (1023, 1024, 1025, 1027, 4099, 120011, 1440000)
BIG = 1440000
ONE_BLOCK = TINY + (1023, 1024, 1025, 1027, 4099)          # curve, track and warp all take one block per entry (and segment)
# (S, h) of the track per length; (1, 8) everywhere: the curve call's sweep
TRACK = {n: [(n, 64), (1, 8)] for n in TINY}
TRACK.update({n: [(3, 9), (1, 8)] for n in (1023, 1024, 1025, 1027, 4099)})
TRACK.update({120011: [(1, 8), (5, 9)], BIG: [(7, 1), (1, 8)]})
_sums, _coef, _warp = {}, {}, {}


# ---- the partition ----------------------------------------------------------------------------------------------------------------

def pearson_blocks(n):
    return max(1, min(512, (n + 16383) // 16384))             # one block per 16 sweeps of 256 threads x 4 frames, at most 512


def curve_blocks(n):
    return max(1, pearson_blocks(n) * 6 // 17)


def warp_blocks(n):
    return max(1, pearson_blocks(n) * 6 // 23)


def track_blocks(n, segs, h):
    return max(1, curve_blocks(n) // (segs * ((2 * h + 17) // 17)))


def chunks(length, nb):
    """(chunk, frames of the last block that has any) of `length` frames over nb blocks"""
    chunk = ((length + nb - 1) // nb + 3) & ~3
    last = length - (((length + chunk - 1) // chunk) - 1) * chunk
    return chunk, last


def test_the_partition_is_the_one_this_file_covers(mod):
    for n in ONE_BLOCK:
        assert curve_blocks(n) == warp_blocks(n) == 1 and all(track_blocks(n, s, h) == 1 for s, h in TRACK[n]), n
    assert [(-(-n // 1024), n % 1024) for n in (1023, 1024, 1025, 1027, 4099)] == [(1, 1023), (1, 0), (2, 1), (2, 3), (5, 3)]
    n = 120011
    assert (pearson_blocks(n), curve_blocks(n), warp_blocks(n)) == (8, 2, 2) and chunks(n, 2) == (60008, 60003)
    assert track_blocks(n, 1, 8) == 2 and track_blocks(n, 5, 9) == 1
    n = BIG
    assert (pearson_blocks(n), curve_blocks(n), warp_blocks(n)) == (88, 31, 22)
    assert chunks(n, 31) == (46452, 46440) and chunks(n, 22) == (65456, 65424)
    assert track_blocks(n, 7, 1) == 4 and track_blocks(n, 1, 8) == 31
    b = track_model.bounds(n, 7)
    assert b[1:3] == [205714, 411428] and [x % 4 for x in b[1:7]] == [2, 0, 2, 1, 3, 1]   # segments that start at any frame mod 4
    # the library's own functions, where it exports them (C++ names: unsigned f(uint32_t), unsigned f(uint32_t, int, int))
    lib = mod.lib()

    def exported(name):
        assert hasattr(lib, name), ("the library no longer exports %s (its signature or linkage changed): restate how this test "
                                    "reads the block counts, or drop this half if nothing exposes them" % name)
        return getattr(lib, name)
    for name, rule in (("_Z18asx_pearson_blocksj", pearson_blocks), ("_Z16asx_curve_blocksj", curve_blocks),
                       ("_Z15asx_warp_blocksj", warp_blocks)):
        fn = exported(name)
        fn.restype, fn.argtypes = ctypes.c_uint, [ctypes.c_uint32]
        for n in LENGTHS + (1000, 999, 144000):
            assert fn(n) == rule(n), (name, n, fn(n), rule(n))
    fn = exported("_Z16asx_track_blocksjii")
    fn.restype, fn.argtypes = ctypes.c_uint, [ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
    for n in LENGTHS:
        for s, h in TRACK[n]:
            assert fn(n, s, h) == track_blocks(n, s, h), (n, s, h)


# ---- inputs and models ------------------------------------------------------------------------------------------------------------

def planted(n):
    return delays(n)[0]


def centres(n):
    """every lag at the tiny lengths; else 0, -1, N - 1, -N and a planted delay"""
    if n in TINY:
        return list(range(-n, n))
    return [0, -1, n - 1, -n, planted(n)]


def modelled(n):
    """the centres the float64 model is computed for"""
    return centres(n) if n < BIG else [-1, planted(n)]


def model_sums(n, idx, segs=1):
    """the model at one index of pair(n): (r_s [S], tolerance [S]), math.fsum over the exact products of each segment; computed once"""
    if (n, idx, segs) not in _sums:
        src, smp = pair(n)
        prod = src.astype(np.float64)[(np.arange(n) + int(idx)) % (2 * n)] * smp.astype(np.float64)
        b = track_model.bounds(n, segs)
        _sums[n, idx, segs] = ([math.fsum(prod[b[s]:b[s + 1]]) for s in range(segs)],
                               [track_model.tol_r(b[s + 1] - b[s], math.fsum(np.abs(prod[b[s]:b[s + 1]]))) for s in range(segs)])
    return _sums[n, idx, segs]


def model_coef(n, idx):
    if (n, idx) not in _coef:
        _coef[n, idx] = curve_model.coef_at(*pair(n), idx)
    return _coef[n, idx]


def model_warp(n, c, a, b, h):
    if (n, c, a, b, h) not in _warp:
        _warp[n, c, a, b, h] = warp_model.warp(*pair(n), c, a, b, h)
    return _warp[n, c, a, b, h]


def half(n):
    return 1 if n == BIG else 8


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


@pytest.fixture(scope="module")
def plans(mod):
    """one plan per length, max_batch = 2: a call of more than two pairs runs in slices"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = mod.Plan(n, 2, 0, None)
            assert cache[n].layout == ("real-column" if n == BIG else "packed"), (n, cache[n].layout)
        return cache[n]
    yield get
    for plan in cache.values():
        plan.close()


# ---- 1. the curve -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
def test_curve_r_frac_and_coef(plans, n):
    src, smp = pair(n)
    plan, cs, h = plans(n), centres(n), half(n)
    hc = h                                                      # the coefficient curve: every column of the call
    r, coef, frac, ret = plan.xcorr_curve_f32(src, smp, cs, half_width=h)
    assert r.shape == coef.shape == (len(cs), 2 * h + 1) and ret.tolist() == [0] * len(cs)
    worst = 0.0
    for k, c in enumerate(cs):
        if c not in modelled(n):
            continue
        for j, idx in enumerate(curve_model.neighbours(c, n, h)):
            (want,), (tol,) = model_sums(n, idx)
            err = abs(float(r[k, j]) - want)
            worst = max(worst, err / tol if tol else (0.0 if err == 0.0 else math.inf))
            assert err <= tol, (n, h, c, j, float(r[k, j]), want, err, tol)
    assert frac.tobytes() == frac_rule(r, h).tobytes()
    # coef: bit for bit the windowed call's direct form at the row [l, l]; within 1e-5 of the oracle's
    lags = np.array([[curve_model.lag_of(i, n) for i in curve_model.neighbours(c, n, hc)] for c in cs], dtype=np.int64)
    plan.set_pearson(False)
    try:
        wlag, wcoef, wret = plan.xcorr_windowed_f32(src, smp, np.stack([lags.reshape(-1)] * 2, axis=1))
    finally:
        if plan.layout == "real-column":
            plan.set_pearson(True)
    sub = np.ascontiguousarray(coef[:, h - hc:h + hc + 1])
    assert wlag.tolist() == lags.reshape(-1).tolist()
    assert sub.tobytes() == wcoef.reshape(sub.shape).tobytes(), (n, np.argwhere(sub != wcoef.reshape(sub.shape)).tolist())
    worst_coef = 0.0
    for k, c in enumerate(cs):
        if c not in modelled(n):
            continue
        for j, idx in enumerate(curve_model.neighbours(c, n, hc)):
            want = model_coef(n, idx)
            assert np.isnan(sub[k, j]) == np.isnan(want), (n, c, j, float(sub[k, j]), want)
            if not np.isnan(want):
                worst_coef = max(worst_coef, abs(float(sub[k, j]) - want))
    assert worst_coef < 1e-5
    if n >= 1000:
        at = cs.index(planted(n))
        assert r[at, h] > 0.5 * n and abs(float(frac[at])) < 0.5                     # the planted delay is a peak of r
    assert np.isnan(coef[cs.index(-n), h])                                         # lag -N: the empty segment
    print("sweep lengths: curve N", n, "h", h, "worst |error| / tolerance", worst, "worst |coef - oracle|", worst_coef)


# ---- 2. the track -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
def test_track_r_seg_and_fit(plans, n):
    src, smp = pair(n)
    plan, cs = plans(n), centres(n)
    for segs, h in TRACK[n]:
        r, seg, fit, used, ret = plan.xcorr_track_f32(src, smp, cs, h, segs)
        assert r.shape == (len(cs), segs, 2 * h + 1) and seg.shape == (len(cs), segs, 2) and fit.shape == (len(cs), 3)
        assert ret.tolist() == [0] * len(cs)
        worst = 0.0
        todo = modelled(n) if (n < 120011 or (segs, h) != (1, 8)) else []   # (1, 8) at the long lengths: the curve call's bytes below
        for k, c in enumerate(cs):
            if c not in todo:
                continue
            for j, idx in enumerate(track_model.indices(c, n, h)):
                want, tol = model_sums(n, idx, segs)
                for s in range(segs):
                    err = abs(float(r[k, s, j]) - want[s])
                    worst = max(worst, err / tol[s] if tol[s] else (0.0 if err == 0.0 else math.inf))
                    assert err <= tol[s], (n, segs, h, c, s, j, float(r[k, s, j]), want[s], err, tol[s])
        check_seg_and_fit(n, h, segs, r, seg, fit, used, ret)
        if (segs, h) == (1, 8):                                  # one segment, one tile: the curve call's sweep, block for block
            cr = plan.xcorr_curve_f32(src, smp, cs, half_width=8, coef=False)[0]
            assert r[:, 0, :].tobytes() == cr.tobytes(), (n, np.argwhere(r[:, 0, :] != cr).tolist())
        print("sweep lengths: track N", n, "S", segs, "h", h, "worst |error| / tolerance", worst)


# ---- 3. the warp ------------------------------------------------------------------------------------------------------------------

def warp_cases(n):
    """(centre, (a, b)) of the model's entries"""
    cs = centres(n)
    if n in TINY:
        return [(c, l) for c in cs for l in ((0.0, 0.0), (0.0, float(n)), (0.0, -float(n)))]
    far = [(0.0, 0.0), (2.0 ** -6, n / 2), (-(2.0 ** -6), -(n / 2)), (12.0 / n, 0.25)]   # as far from the centre as a valid line goes
    if n <= 4099:
        return [(c, l) for c in cs for l in far]
    if n == BIG:
        return [(-1, far[0]), (planted(n), far[1])]
    return [(cs[i % len(cs)], l) for i, l in enumerate(far + far[1:3])] + [(-n, far[0])]


@pytest.mark.parametrize("n", LENGTHS)
def test_warp_r_frac_coef_and_len(plans, n):
    src, smp = pair(n)
    plan, h = plans(n), half(n)
    todo = warp_cases(n)
    cs = [c for c, _ in todo]
    r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, cs, np.array([l for _, l in todo]), half_width=h)
    assert r.shape == (len(cs), 2 * h + 1)
    worst = worst_coef = 0.0
    for k, (c, (a, b)) in enumerate(todo):
        m = model_warp(n, c, a, b, h)
        for j in range(2 * h + 1):
            err, tol = abs(float(r[k, j]) - m["r"][j]), m["tol"][j]
            worst = max(worst, err / tol if tol else (0.0 if err == 0.0 else math.inf))
            assert err <= tol, (n, h, c, a, b, j, float(r[k, j]), m["r"][j], err, tol)
        assert int(length[k]) == m["len"], (n, c, a, b, int(length[k]), m["len"])
        if np.isnan(m["coef"]):
            assert np.isnan(coef[k]) and int(ret[k]) == -1, (n, c, a, b, float(coef[k]), int(ret[k]))
        else:
            err = abs(float(coef[k]) - m["coef"])
            worst_coef = max(worst_coef, err / m["tol_coef"])
            assert err <= m["tol_coef"] and int(ret[k]) == 0, (n, c, a, b, float(coef[k]), m["coef"], err, m["tol_coef"], int(ret[k]))
    assert frac.tobytes() == frac_rule(r, h).tobytes()
    print("sweep lengths: warp N", n, "h", h, "worst |error| / tolerance of r", worst, "of coef", worst_coef)


@pytest.mark.parametrize("n", LENGTHS)
def test_the_warp_on_the_line_0_0_is_the_curve_call(plans, n):
    src, smp = pair(n)
    plan, cs, h = plans(n), centres(n), half(n)
    r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, cs, [0.0, 0.0], half_width=h)
    cr, cc, cf, cret = plan.xcorr_curve_f32(src, smp, cs, half_width=h)
    assert cret.tolist() == [0] * len(cs)
    worst = 0.0
    if n in ONE_BLOCK:                                           # one block either way: the same sweep, the same bits
        assert r.tobytes() == cr.tobytes() and frac.tobytes() == cf.tobytes(), (n, np.argwhere(r != cr).tolist())
    else:                                                        # the block counts differ (120 011: the same count, another record)
        for k, c in enumerate(cs):
            if c not in modelled(n):
                continue
            for j, idx in enumerate(curve_model.neighbours(c, n, h)):
                err, tol = abs(float(r[k, j]) - float(cr[k, j])), 2 * model_sums(n, idx)[1][0]
                worst = max(worst, err / tol)
                assert err <= tol, (n, c, j, err, tol)
    for k, c in enumerate(cs):
        lo, hi = warp_model.valid_range(n, c, 0.0, 0.0)
        assert int(length[k]) == hi - lo, (n, c)
        if np.isnan(cc[k, h]):                                   # no frame lines up, or a constant side
            assert np.isnan(coef[k]) and int(ret[k]) == -1, (n, c)
            continue
        assert int(ret[k]) == 0, (n, c)
        if c in modelled(n):                                     # the two coefficients within the model's tolerance of each other
            tol = model_warp(n, c, 0.0, 0.0, h)["tol_coef"]
            assert abs(float(coef[k]) - float(cc[k, h])) <= tol, (n, c, float(coef[k]), float(cc[k, h]), tol)
    print("sweep lengths: warp against curve N", n, "worst |difference| / (sum of both tolerances)", worst)


# ---- 4. the invariants ------------------------------------------------------------------------------------------------------------

def nine(n):
    """(sources [9, 2N], samples [9, N], nine valid centres): pair(n, 0) with the centre `c` sixth, pair(n, 1) around it"""
    (s0, t0), (s1, t1) = pair(n, 0), pair(n, 1)
    c = planted(n) if n >= 1000 else -1
    cs = [(7 * i) % (2 * n) - n for i in range(9)]
    cs[5] = c
    return np.stack([s1] * 5 + [s0] + [s1] * 3), np.stack([t1] * 5 + [t0] + [t1] * 3), cs, c


@pytest.mark.parametrize("n", LENGTHS)
def test_an_entry_depends_on_neither_its_batch_nor_its_place(plans, n):
    src, smp, cs, c = nine(n)
    s0, t0 = pair(n, 0)
    plan = plans(n)                                               # max_batch = 2: the nine run in five slices
    alone = plan.xcorr_curve_f32(s0, t0, [c], half_width=8)
    assert same(alone, [a[5:6] for a in plan.xcorr_curve_f32(src, smp, cs, half_width=8)]), n
    for segs, h in TRACK[n]:
        alone = plan.xcorr_track_f32(s0, t0, [c], h, segs)
        assert same(alone, [a[5:6] for a in plan.xcorr_track_f32(src, smp, cs, h, segs)]), (n, segs, h)
    lines = np.array([[0.0, 0.0], [1e-3, 0.5]] * 4 + [[2.0 ** -6, -0.5]])
    line = [-(2.0 ** -6), 0.75]
    lines[5] = line
    alone = plan.xcorr_warp_f32(s0, t0, [c], line, half_width=8)
    assert same(alone, [a[5:6] for a in plan.xcorr_warp_f32(src, smp, cs, lines, half_width=8)]), n
    assert int(alone[4][0]) in (0, -1) and not np.isnan(alone[0]).any()


@pytest.mark.parametrize("n", [n for n in LENGTHS if n != BIG])
def test_a_misaligned_pair_on_a_packed_plan_is_the_aligned_one(plans, torch, n):
    """the 4-byte fall-back of the sweep's 16-byte loads: the same tracks one and three floats into their buffers"""
    s0, t0 = pair(n)
    plan, cs = plans(n), centres(n)
    d_s = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), s0, np.zeros(3, np.float32)])).cuda()
    d_t = torch.from_numpy(np.concatenate([np.zeros(3, np.float32), t0, np.zeros(1, np.float32)])).cuda()
    assert d_s.data_ptr() % 16 == 0 and d_t.data_ptr() % 16 == 0
    d_s, d_t = d_s[1:1 + 2 * n], d_t[3:3 + n]
    assert same(dev_curve(torch, plan, d_s, 0, d_t, 0, len(cs), 1, cs, 8), plan.xcorr_curve_f32(s0, t0, cs, half_width=8)), n
    for segs, h in TRACK[n]:
        assert same(dev_track(torch, plan, d_s, 0, d_t, 0, len(cs), 1, cs, h, segs), plan.xcorr_track_f32(s0, t0, cs, h, segs)), (n, segs, h)
    lines = np.array([[0.0, 0.0], [-(2.0 ** -6), 0.75], [0.0, float(n)]] * len(cs))[:len(cs)]
    assert same(dev_warp(torch, plan, d_s, 0, d_t, 0, len(cs), 1, cs, lines, 2, 8), plan.xcorr_warp_f32(s0, t0, cs, lines, half_width=8)), n
