"""The warped correlation on the MI355X (asx_xcorr_warp_f32_dev, asx_xcorr_pool_warp_f32_dev and their Plan methods).

r must be the float64 model's sum (tests/warp_model.py: math.fsum over the exact products along the line) at every offset across the
line within N * 2^-53 * sum |products| -- the first-order worst case of any float64 summation order; frac must be the header's rule
applied to the call's own r, bit for bit; coef must be the model's two-pass coefficient within warp_model.tol_coef; len must be |V|.
On the line (0, 0) the call must agree with the curve call.  A planted drifting pair must come back with a coefficient of 1 along its
line where the curve call finds at most 0.25 at any constant lag.  Shapes: N = 1000 on a packed plan (25 x 40), N = 999, which no
block size divides, and N = 144 000, the smallest real-column length, where an entry takes two blocks.

Measured worst error / tolerance (h = 1 and 8; the whole table: profiles/warp/cost.txt):
    r                N = 1000: 1.03e-3;  N = 999: 9.7e-4;  N = 144 000: 9.2e-7
    coef             N = 1000: 7.8e-4;   N = 999: 1.8e-4;  N = 144 000: 6.2e-4
    the line (0, 0) against the curve call: r the same bits at N = 1000 and 999 (one block either way), 1.8e-7 of the sum of both
    tolerances at N = 144 000 (two blocks against three); coef 1.8e-6, 8.8e-7 and 1.7e-8 of tol_coef
Planted pairs: coef exactly 1.0 along the line in all fourteen cases; the curve call's best coefficient within +-8 of l0 is 0.097 -
0.154 (N = 1000, 999), 0.088 - 0.116 (N = 144 000, 12 frames) and 0.005 - 0.033 (40 frames).  The track call's own fit of a planted
pair (S = 8, h = 16), fed in as it stands: coef 0.982 (N = 1000) and 0.988 (N = 144 000).
"""
import ctypes

import numpy as np
import pytest

import warp_model
from test_gpu_curve import delays, frac_rule, pair, same
from util import asx

pytestmark = pytest.mark.gpu

SHAPES = {1000: "25x40x8", 144000: None, 999: None}
_model = {}
worst = {"r": 0.0, "coef": 0.0, "curve_r": 0.0, "curve_coef": 0.0}


def lines_of(n):
    return [(0.0, 0.0), (0.0, 3.0), (0.0, -2.5), (12.0 / n, 0.25), (-12.0 / n, -0.25), (2.0 ** -6, n / 2), (-(2.0 ** -6), -n / 2)]


def centres(n):
    return [0, -1, n - 1, -n, delays(n)[0], delays(n)[1]]


def model(n, c, a, b):
    """the model of pair(n) along (a, b) through c at h = 8 (h = 1 is its middle); computed once"""
    if (n, c, a, b) not in _model:
        _model[n, c, a, b] = warp_model.warp(*pair(n), c, a, b, 8)
    return _model[n, c, a, b]


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


def make_plan(mod, n, max_batch=4):
    plan = mod.Plan(n, max_batch, 0, SHAPES[n])
    assert plan.layout == ("real-column" if n == 144000 else "packed"), (n, plan.layout)
    return plan


def outputs(torch, entries, h):
    f64 = lambda count: torch.full((count,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    return (f64(entries * (2 * h + 1)), f64(entries), f64(entries), torch.full((entries,), 7, dtype=torch.int64, device="cuda"),
            torch.full((entries,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    return all(bool((a == 7).all().item()) for a in out)


def dev_warp(torch, plan, d_src, ss, d_smp, ts, batch, entries, centers, lines, ls, h, pool=None, length=True):
    """the raw call on device tensors -> (r [E, 2h + 1], frac [E], coef [E], len [E], ret [E]) as host arrays; lines: the float64
    array d_line points to, ls its stride; pool: (nsources, nsamples, pairs or None); length False: a null d_len"""
    c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.int64).reshape(-1)).cuda()
    ln = torch.from_numpy(np.ascontiguousarray(lines, dtype=np.float64).reshape(-1)).cuda()
    assert c.numel() == batch * entries and ln.numel() >= (batch * entries - 1) * ls + 2
    out = outputs(torch, batch * entries, h)
    ptrs = [a.data_ptr() for a in out]
    if not length:
        ptrs[3] = 0
    torch.cuda.synchronize()
    if pool is None:
        plan.xcorr_warp_dev(d_src.data_ptr(), ss, d_smp.data_ptr(), ts, batch, entries, c.data_ptr(), ln.data_ptr(), ls, h, *ptrs)
    else:
        ns, nm, rows = pool
        d_rows = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        torch.cuda.synchronize()
        plan.xcorr_pool_warp_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ts, nm, 0 if d_rows is None else d_rows.data_ptr(), batch,
                                 entries, c.data_ptr(), ln.data_ptr(), ls, h, *ptrs)
    plan.sync()
    r, fr, cf, le, rt = (a.cpu().numpy() for a in out)
    return r.reshape(-1, 2 * h + 1), fr, cf, le, rt


def check_entry(n, h, c, a, b, r, frac, coef, length, ret):
    """one entry against the model of pair(n)"""
    m = model(n, c, a, b)
    for j in range(2 * h + 1):
        want, tol = m["r"][8 - h + j], m["tol"][8 - h + j]
        err = abs(float(r[j]) - want)
        worst["r"] = max(worst["r"], err / tol)
        assert err <= tol, (n, h, c, a, b, j, float(r[j]), want, err, tol)
    assert np.asarray(frac).tobytes() == frac_rule(r[None, :], h)[0].tobytes(), (n, h, c, a, b, frac)
    assert int(length) == m["len"], (n, h, c, a, b, int(length), m["len"])
    if np.isnan(m["coef"]):
        assert np.isnan(coef) and int(ret) == -1, (n, h, c, a, b, coef, ret)
    else:
        err = abs(float(coef) - m["coef"])
        worst["coef"] = max(worst["coef"], err / m["tol_coef"])
        assert err <= m["tol_coef"] and int(ret) == 0, (n, h, c, a, b, float(coef), m["coef"], err, m["tol_coef"], ret)


# ---- 1. against the model, 2. the line (0, 0) against the curve call ----------------------------------------------------------------

def cases(n):
    """(centre, line) pairs: every centre with every line at the small lengths; at N = 144 000 every line and every centre at least
    once (the model is a few milliseconds per value there)"""
    cs, ls = centres(n), lines_of(n)
    if n < 144000:
        return [(c, l) for c in cs for l in ls]
    return [(cs[i % len(cs)], l) for i, l in enumerate(ls)] + [(cs[3], ls[0]), (cs[3], ls[5]), (cs[2], ls[6])]


@pytest.mark.parametrize("n", [1000, 999, 144000])
def test_r_frac_coef_len_and_ret_against_the_model(mod, n):
    src, smp = pair(n)
    todo = cases(n)
    cs = [c for c, _ in todo]
    ln = np.array([l for _, l in todo])
    worst.update(dict.fromkeys(worst, 0.0))
    with make_plan(mod, n) as plan:
        for h in (1, 8):
            r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, cs, ln, half_width=h)
            assert r.shape == (len(cs), 2 * h + 1) and frac.shape == coef.shape == length.shape == ret.shape == (len(cs),)
            assert length.dtype == np.int64 and ret.dtype == np.int32
            for k, (c, (a, b)) in enumerate(todo):
                check_entry(n, h, c, a, b, r[k], frac[k], coef[k], length[k], ret[k])
            assert -1 in ret.tolist() and 0 in ret.tolist()          # c = -N on the line (0, 0): nothing lines up
    print("warp N", n, "worst error / tolerance", worst)


@pytest.mark.parametrize("n", [1000, 999, 144000])
def test_the_line_0_0_is_the_curve_call(mod, n):
    src, smp = pair(n)
    cs = centres(n) + [1, -n + 1]
    worst.update(dict.fromkeys(worst, 0.0))
    with make_plan(mod, n) as plan:
        for h in (1, 8):
            r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, cs, [0.0, 0.0], half_width=h)
            cr, cc, cf, cret = plan.xcorr_curve_f32(src, smp, cs, half_width=h)
            assert cret.tolist() == [0] * len(cs)
            for k, c in enumerate(cs):
                m = model(n, c, 0.0, 0.0) if (n < 144000 or c in centres(n)[:4]) else None
                if m is not None:                                # r within the sum of both calls' tolerances of each other
                    for j in range(2 * h + 1):
                        err, tol = abs(float(r[k, j]) - float(cr[k, j])), 2 * m["tol"][8 - h + j]
                        worst["curve_r"] = max(worst["curve_r"], err / tol)
                        assert err <= tol, (n, h, c, j, err, tol)
                lo, hi = warp_model.valid_range(n, c, 0.0, 0.0)
                assert int(length[k]) == hi - lo, (n, h, c)
                if np.isnan(cc[k, h]):                           # no frame lines up at c = -N, one at -N + 1: a constant side
                    assert np.isnan(coef[k]) and int(ret[k]) == -1 and hi - lo <= 1, (n, h, c)
                    continue
                assert int(ret[k]) == 0
                if m is not None:
                    err = abs(float(coef[k]) - float(cc[k, h]))
                    worst["curve_coef"] = max(worst["curve_coef"], err / m["tol_coef"])
                    assert err <= m["tol_coef"], (n, h, c, float(coef[k]), float(cc[k, h]), m["tol_coef"])
    print("warp against curve N", n, "worst error / tolerance", worst)


# ---- 3. planted pairs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 999, 144000])
def test_a_planted_pair_has_its_coefficient_along_the_line_only(mod, n):
    with make_plan(mod, n) as plan:
        for l0, a, b in warp_model.planted_cases(n):
            src, smp = warp_model.planted(n, l0, a, b)
            lo, hi = warp_model.valid_range(n, l0, a, b)
            want, count, tol = warp_model.coef(src, smp, l0, a, b)
            assert want == 1.0 and count == hi - lo                          # (sample == source along the line)
            r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, [l0], [a, b], half_width=8)
            flat = plan.xcorr_curve_f32(src, smp, [l0], half_width=8)[1][0]
            print("planted N", n, "l0", l0, "line", (a, b), "coef", float(coef[0]), "1 - coef", 1.0 - float(coef[0]), "tol", tol, "len",
                  int(length[0]), "best constant lag within +-8", float(np.nanmax(flat)))
            assert int(ret[0]) == 0 and int(length[0]) == hi - lo, (n, l0, a, b, ret, length, hi - lo)
            assert float(coef[0]) >= 1.0 - tol, (n, l0, a, b, float(coef[0]), tol)
            assert float(np.nanmax(flat)) <= 0.25, (n, l0, a, b, flat.tolist())
            assert int(np.argmax(np.abs(r[0]))) == 8 and abs(float(frac[0])) < 0.5       # the ridge runs along the line


# ---- 4. line_stride -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_line_strides_and_the_track_calls_fit(mod, torch, n):
    src, smp = pair(n)
    cs = [5, -7, delays(n)[0], delays(n)[1]]
    a, b = 12.0 / n, 0.25
    d_src, d_smp = torch.from_numpy(np.array(src)).cuda(), torch.from_numpy(np.array(smp)).cuda()
    with make_plan(mod, n) as plan:
        fit = np.array([[a, b, 123.0]] * 4)                                # the shape of the track call's d_fit; rms is not read
        three = dev_warp(torch, plan, d_src, 0, d_smp, 0, 4, 1, cs, fit, 3, 8)
        assert three[4].tolist() == [0] * 4
        assert same(three, dev_warp(torch, plan, d_src, 0, d_smp, 0, 4, 1, cs, fit[:, :2], 2, 8))
        assert same(three, dev_warp(torch, plan, d_src, 0, d_smp, 0, 4, 1, cs, [a, b], 0, 8))
        assert same(three, dev_warp(torch, plan, d_src, 0, d_smp, 0, 4, 1, cs, np.array([[a, b, 0, 0, 0]] * 4), 5, 8))
        assert same(three, plan.xcorr_warp_f32(src, smp, cs, fit, half_width=8))          # the Plan method is the raw call
        assert same(three, plan.xcorr_warp_f32(src, smp, cs, [a, b], half_width=8))
        # the track call's own fit of a planted pair, as it stands
        l0, pa, pb = warp_model.planted_cases(n)[0]
        psrc, psmp = warp_model.planted(n, l0, pa, pb)
        centre = l0 + 6
        _, _, tfit, used, tret = plan.xcorr_track_f32(psrc, psmp, [centre], 16, 8)
        assert int(tret[0]) == 0 and int(used[0]) >= 2 and tfit.shape == (1, 3)
        r, frac, coef, length, ret = plan.xcorr_warp_f32(psrc, psmp, [centre], tfit, half_width=8)
        print("track fit N", n, "drift * N", float(tfit[0, 0]) * n, "lag0", float(tfit[0, 1]), "-> coef", float(coef[0]), "len", int(length[0]))
        assert int(ret[0]) == 0 and float(coef[0]) > 0.25
        # ... and the NaN line the track call returns with one segment: -5
        _, _, tfit, used, _ = plan.xcorr_track_f32(psrc, psmp, [centre], 16, 1)
        assert np.isnan(tfit).all()
        assert plan.xcorr_warp_f32(psrc, psmp, [centre], tfit)[4].tolist() == [-5]


# ---- 5. structure -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_an_entry_depends_on_neither_its_batch_nor_the_plan(mod, n):
    s0, t0 = pair(n, 0)
    s1, t1 = pair(n, 1)
    c = delays(n)[1]
    line = [-12.0 / n, -0.25]
    src = np.stack([s1] * 3 + [s0] + [s1])
    smp = np.stack([t1] * 3 + [t0] + [t1])
    cs = [3, -7, n - 1, c, -n]
    ln = [[0.0, 0.0], [1e-3, 2.0], [2.0 ** -6, 1.0], line, [0.0, 0.0]]
    for h in (1, 8):
        got = []
        for max_batch in (1, 4):
            with make_plan(mod, n, max_batch) as plan:
                got.append(plan.xcorr_warp_f32(s0, t0, [c], line, half_width=h))
                got.append(tuple(a[3:4] for a in plan.xcorr_warp_f32(src, smp, cs, ln, half_width=h)))
        for other in got[1:]:
            assert same(got[0], other), (n, h)
        assert int(got[0][4][0]) == 0 and not np.isnan(got[0][0]).any()


@pytest.mark.parametrize("n", [1000, 144000])
def test_broadcast_strides_and_entries(mod, n):
    (s0, t0), (s1, t1) = pair(n, 0), pair(n, 1)
    cs = [delays(n)[0], -5, delays(n)[1] + 5]
    ln = [[12.0 / n, 0.25], [0.0, -2.5], [-(2.0 ** -6), 7.0]]
    with make_plan(mod, n) as plan:
        got = plan.xcorr_warp_f32(s0, np.stack([t0, t1, t0]), cs, ln, half_width=8)                       # source_stride = 0
        assert same(got, plan.xcorr_warp_f32(np.stack([s0] * 3), np.stack([t0, t1, t0]), cs, ln, half_width=8))
        got = plan.xcorr_warp_f32(np.stack([s0, s1, s0]), t1, cs, ln, half_width=8)                       # sample_stride = 0
        assert same(got, plan.xcorr_warp_f32(np.stack([s0, s1, s0]), np.stack([t1] * 3), cs, ln, half_width=8))
        three = plan.xcorr_warp_f32(np.stack([s0, s1]), np.stack([t0, t1]), [cs, cs[::-1]], [ln, ln[::-1]], half_width=8, entries=3)
        assert three[0].shape == (2, 3, 17) and all(a.shape == (2, 3) for a in three[1:])
        for b, (s, t) in enumerate(((s0, t0), (s1, t1))):
            for j in range(3):
                one = plan.xcorr_warp_f32(s, t, [[cs, cs[::-1]][b][j]], [[ln, ln[::-1]][b][j]], half_width=8)
                assert same(one, [a[b, j:j + 1] for a in three]), (b, j)


# ---- 6. the pool form ---------------------------------------------------------------------------------------------------------------

def test_the_pool_form_is_the_strided_form_entry_by_entry(mod, torch):
    n = 144000
    clips = np.stack([pair(n, 0)[0], pair(n, 1)[0], np.roll(pair(n, 0)[0], 321)])
    d_clips = torch.from_numpy(clips).cuda()                                # one pool for both sides: sources and samples alias
    rows = np.array([[0, 1], [2, 0], [1, 1], [2, 2], [0, 2]], dtype=np.int32)
    cs = np.array([[0, 5], [321, -n], [0, n - 1], [-1, 1], [-321, 0]], dtype=np.int64)
    ln = np.array([[[1e-4, -3.0], [0.0, 0.0]], [[0.0, 0.0], [2.0 ** -6, 9.0]], [[12.0 / n, 0.25], [-1e-5, 0.5]], [[0.0, 2.0], [0.0, 0.0]],
                   [[0.0, 0.0], [-12.0 / n, -0.25]]])
    with make_plan(mod, n, 2) as plan:
        ws = plan.workspace_bytes
        for h in (1, 8):
            got = dev_warp(torch, plan, d_clips, 2 * n, d_clips, 2 * n, len(rows), 2, cs, ln, 2, h, pool=(3, 3, rows))
            assert set(got[4].tolist()) <= {0, -1} and plan.debug_bank()[:2] == (0, 0) and plan.workspace_bytes == ws
            for k, (a, b) in enumerate(rows):
                one = dev_warp(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 2, cs[k], ln[k], 2, h)
                assert same(one, [x[2 * k:2 * k + 2] for x in got]), (h, k)
            assert got[0][2, h] > 0.5 * n and got[0][8, h] > 0.5 * n        # clip 2 is clip 0 delayed
        every = dev_warp(torch, plan, d_clips, 2 * n, d_clips, 2 * n, 9, 1, np.zeros(9, np.int64), [1e-5, 1.0], 0, 1, pool=(3, 3, None))
        for a in range(3):
            for b in range(3):
                one = dev_warp(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 1, [0], [1e-5, 1.0], 0, 1)
                assert same(one, [x[3 * a + b:3 * a + b + 1] for x in every]), (a, b)
        # the Plan method is the raw call
        assert same(plan.xcorr_pool_warp_f32(clips, clips[:, :n], cs, ln, pairs=rows, half_width=8, entries=2),
                    [x.reshape((5, 2) + x.shape[1:]) for x in got])


# ---- 7. invalid entries -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_invalid_entries(mod, n):
    s0, t0 = pair(n, 0)
    h = 8
    nan, up = float("nan"), float(np.nextafter(2.0 ** -6, 1.0))
    ok = [1e-4, 0.5]
    with make_plan(mod, n) as plan:
        good = plan.xcorr_warp_f32(s0, t0, list(range(5, 15)), [ok] * 10, half_width=h)
        assert good[4].tolist() == [0] * 10
        cs = [5, n, 7, -n - 1, 9, 10, 11, 12, 13, n]
        ln = [ok, ok, ok, ok, ok, [nan, 0.0], [up, 0.0], [0.0, n + 0.5], ok, [nan, nan]]      # the last: -2 over -5
        got = plan.xcorr_warp_f32(s0, t0, cs, ln, half_width=h)
        assert got[4].tolist() == [0, -2, 0, -2, 0, -5, -5, -5, 0, -2]
        for k in (1, 3, 5, 6, 7, 9):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]) and np.isnan(got[2][k]) and int(got[3][k]) == 0, k
        for k in (0, 2, 4, 8):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        for line in ([-up, 0.0], [0.0, -n - 0.5], [0.0, nan], [float("inf"), 0.0], [0.0, -float("inf")]):
            assert plan.xcorr_warp_f32(s0, t0, [5], line)[4].tolist() == [-5], line
        for c, line in ((5, [2.0 ** -6, float(n)]), (n - 1, [-(2.0 ** -6), -float(n)])):        # the bounds themselves are valid
            assert plan.xcorr_warp_f32(s0, t0, [c], line)[4].tolist() == [0], line
        # nothing lines up: ret -1, len 0, r and frac still written
        r, frac, coef, length, ret = plan.xcorr_warp_f32(s0, t0, [-n, -n], [[0.0, 0.0], [0.0, -3.0]], half_width=h)
        assert ret.tolist() == [-1, -1] and length.tolist() == [0, 0] and np.isnan(coef).all()
        assert not np.isnan(r).any() and not np.isnan(frac).any()
        if plan.layout != "real-column":
            return
        clips = np.stack([s0, pair(n, 1)[0]])
        rows = np.array([[0, 1], [2, 0], [1, 0], [0, -1], [2, 0], [1, 1], [0, 2]], dtype=np.int32)
        inside = np.array([[0, 1], [0, 0], [1, 0], [0, 0], [0, 0], [1, 1], [0, 0]], dtype=np.int32)
        cs = [5, 6, 7, 8, n, 9, 10]                       # row 4: outside its pool AND its centre outside: -4 over -2
        ln = [ok, ok, ok, ok, ok, ok, [nan, 0.0]]         # row 6: outside its pool AND its line not valid: -4 over -5
        good = plan.xcorr_pool_warp_f32(clips, clips[:, :n], cs[:4] + [9, 9, 10], [ok] * 7, pairs=inside, half_width=h)
        got = plan.xcorr_pool_warp_f32(clips, clips[:, :n], cs, ln, pairs=rows, half_width=h)
        assert got[4].tolist() == [0, -4, 0, -4, -4, 0, -4] and good[4].tolist() == [0] * 7
        for k in (1, 3, 4, 6):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]) and np.isnan(got[2][k]) and int(got[3][k]) == 0, k
        for k in (0, 2, 5):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        both = plan.xcorr_pool_warp_f32(clips, clips[:, :n], [5, n, 6, n], [ok, ok, [nan, 0.0], [nan, 0.0]], pairs=inside[:4], half_width=h)
        assert both[4].tolist() == [0, -2, -5, -2]


# ---- 8. refusals, 9. side effects ---------------------------------------------------------------------------------------------------

def test_refusals(mod, torch):
    n = 144000
    s0, t0 = pair(n, 0)
    d_src = torch.from_numpy(np.concatenate([s0, s0[:8]])).cuda()
    d_smp = torch.from_numpy(np.concatenate([t0, t0[:8]])).cuda()
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_l = torch.zeros(6, dtype=torch.float64, device="cuda")
    with make_plan(mod, n) as plan:
        def call(out, pool=False, entries=1, h=1, ls=2, drop=None, src=d_src.data_ptr(), smp=d_smp.data_ptr(), ss=0, ts=0,
                 c=d_c.data_ptr(), line=d_l.data_ptr(), ns=1, nm=1, batch=2, rows=d_c.data_ptr()):
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            if pool:
                plan.xcorr_pool_warp_dev(src, ss, ns, smp, ts, nm, rows, batch, entries, c, line, ls, h, *ptrs)
            else:
                plan.xcorr_warp_dev(src, ss, smp, ts, batch, entries, c, line, ls, h, *ptrs)
            plan.sync()

        def refused(match, **kw):
            out = outputs(torch, 2, 8)
            with pytest.raises(mod.AsxError, match=match):
                call(out, **kw)
            assert untouched(torch, out), kw

        for pool in (False, True):
            for kw in (dict(src=0), dict(smp=0), dict(c=0), dict(line=0), dict(drop=0), dict(drop=1), dict(drop=2), dict(drop=4)):
                refused("null", pool=pool, **kw)
            for e in (0, 9, -1):
                refused("entries", pool=pool, entries=e)
            for h in (0, 9, -1, 2 ** 20):
                refused("half_width", pool=pool, h=h)
            refused("line_stride", pool=pool, ls=1)
            refused("aligned", pool=pool, src=d_src.data_ptr() + 4)
            refused("aligned", pool=pool, smp=d_smp.data_ptr() + 8)
            refused("multiples of 4", pool=pool, ss=2)
            refused("multiples of 4", pool=pool, ts=n + 1)
        refused("every combination", pool=True, rows=0, ns=1, nm=1, batch=2)
        refused("empty pool", pool=True, ns=0)
        refused("empty pool", pool=True, nm=0)
        # a NULL plan (the raw symbol), and batch == 0 returns 0 with nothing written
        out = outputs(torch, 2, 1)
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(a.data_ptr()) for a in out]
        assert mod.lib().asx_xcorr_warp_f32_dev(None, d_src.data_ptr(), 0, d_smp.data_ptr(), 0, 2, 1, d_c.data_ptr(), d_l.data_ptr(), 2, 1,
                                                *ptrs, None) == -1
        assert mod.lib().asx_xcorr_pool_warp_f32_dev(None, d_src.data_ptr(), 0, 1, d_smp.data_ptr(), 0, 1, None, 1, 1, d_c.data_ptr(),
                                                     d_l.data_ptr(), 2, 1, *ptrs, None) == -1
        call(out, batch=0)
        call(out, pool=True, batch=0, rows=0, ns=0, nm=0)
        assert untouched(torch, out)
        # d_len may be NULL: the others are written, it keeps its sentinel
        out = outputs(torch, 2, 1)
        call(out, drop=3)
        assert (out[3].cpu().numpy() == 7).all() and out[4].cpu().tolist() == [0, 0] and not (out[0].cpu().numpy() == 7.0).any()
        assert not (out[1].cpu().numpy() == 7.0).any() and not (out[2].cpu().numpy() == 7.0).any()
    m = 1000
    d_s, d_t = torch.zeros(4 * m + 4, dtype=torch.float32, device="cuda"), torch.zeros(2 * m + 4, dtype=torch.float32, device="cuda")
    with make_plan(mod, m) as plan:
        out = outputs(torch, 4, 1)
        torch.cuda.synchronize()
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.xcorr_pool_warp_dev(d_s.data_ptr(), 2 * m, 2, d_t.data_ptr(), m, 2, 0, 4, 1, d_c.data_ptr(), d_l.data_ptr(), 0, 1,
                                     *(a.data_ptr() for a in out))
        assert untouched(torch, out)
        # a packed plan takes any float-aligned pointer and any stride; silent tracks: r = 0, both sides constant, ret -1
        out = outputs(torch, 2, 1)
        plan.xcorr_warp_dev(d_s.data_ptr() + 4, 2 * m + 1, d_t.data_ptr() + 12, m - 3, 2, 1, d_c.data_ptr(), d_l.data_ptr(), 3, 1,
                            *(a.data_ptr() for a in out))
        plan.sync()
        assert out[4].cpu().tolist() == [-1, -1] and (out[0].cpu().numpy() == 0.0).all() and out[3].cpu().tolist() == [m, m]
        assert out[1].cpu().tolist() == [0.0, 0.0] and np.isnan(out[2].cpu().numpy()).all()
    # a short odd length: one block, a sweep shorter than the stretch is wide
    m = 49
    rng = np.random.default_rng(7)
    src, smp = rng.standard_normal(2 * m).astype(np.float32), rng.standard_normal(m).astype(np.float32)
    with mod.Plan(m, 1, 0) as plan:
        for c, a, b in ((-3, 2.0 ** -6, -0.5), (m - 1, -(2.0 ** -6), 20.0), (-m, 0.01, 30.25)):
            r, frac, coef, length, ret = plan.xcorr_warp_f32(src, smp, [c], [a, b], half_width=8)
            want = warp_model.warp(src, smp, c, a, b, 8)
            assert (np.abs(r[0] - want["r"]) <= want["tol"]).all() and int(length[0]) == want["len"], (c, a, b)
            assert abs(float(coef[0]) - want["coef"]) <= want["tol_coef"] and int(ret[0]) == 0, (c, a, b, coef, want["coef"])


@pytest.mark.parametrize("n", [1000, 144000])
def test_the_call_leaves_the_plan_as_it_was(mod, torch, n):
    src = np.stack([pair(n, 0)[0], pair(n, 1)[0], pair(n, 0)[0]])
    smp = np.stack([pair(n, 0)[1], pair(n, 1)[1], pair(n, 1)[1]])
    ln = [[12.0 / n, 0.25], [0.0, 0.0], [-1e-4, -2.5]]

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes, plan.lag_window, plan.debug_bank())

    with make_plan(mod, n, 2) as plan:
        before = plan.xcorr_batch_f32(src, smp)
        was = state(plan)
        got = plan.xcorr_warp_f32(src, smp, before[0], ln, half_width=8)
        assert state(plan) == was
        plan.set_lag_window(-5, 5)
        plan.set_exact(False)
        assert same(got, plan.xcorr_warp_f32(src, smp, before[0], ln, half_width=8))   # neither the window nor the mode plays a part
        plan.set_exact(True)
        plan.set_lag_window(-n, n - 1)
        assert state(plan) == was
        assert same(before, plan.xcorr_batch_f32(src, smp))
        was = state(plan)                                        # (the batch call counted its Pearson modes)
        d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        assert same(got, dev_warp(torch, plan, d_src, 2 * n, d_smp, n, 3, 1, before[0], ln, 2, 8))
        assert state(plan) == was
    assert got[4].tolist() == [0, 0, 0]
