"""The curve around given lags on the MI355X (asx_xcorr_curve_f32_dev, asx_xcorr_pool_curve_f32_dev and their Plan methods).

r must be the float64 model's sum (tests/curve_model.py: math.fsum over the exact products) at every neighbour of every centre within
N * 2^-53 * sum |source * sample| over that index's terms -- the first-order worst case of any float64 summation order, so it holds
for whatever tree the kernel uses; frac must be the header's rule applied to the call's own r, bit for bit; coef must be, bit for
bit, what the windowed call returns for the row [l, l] under the direct Pearson form.  Shapes: N = 1000 on a packed plan (25 x 40),
N = 144 000, the smallest real-column length, and N = 999, which no block size divides.

Measured worst |error| / tolerance of r per shape (h = 8, the eight centres of case 1):
    N = 1000      1.03e-3
    N = 144 000   1.15e-5
    N = 999       9.7e-4
(the same at h = 1; the coefficient curve is within 7.8e-16 of the float64 oracle at every neighbour).
"""
import ctypes

import numpy as np
import pytest

import curve_model
from util import asx

pytestmark = pytest.mark.gpu

SHAPES = {1000: "25x40x8", 144000: None, 999: None}
_pairs, _r, _coef = {}, {}, {}


def delays(n):
    """three planted delays: a mid positive lag, a mid negative lag and a small one, far apart"""
    return n // 3 + 1, -(n // 4) - 3, 17


def pair(n, seed=0):
    """2n samples of white noise and a sample that holds it at three delays (weights 1, 0.7, 0.5; circular, so a negative delay keeps
    its whole energy) under a little noise, as float32; computed once and never written to"""
    if (n, seed) not in _pairs:
        rng = np.random.default_rng(100 + seed)
        src = rng.standard_normal(2 * n).astype(np.float32)
        d = [x + 5 * seed for x in delays(n)]
        smp = sum(w * np.roll(src, -l)[:n] for w, l in zip((1.0, 0.7, 0.5), d)) + 0.1 * rng.standard_normal(n)
        smp = smp.astype(np.float32)
        src.setflags(write=False)
        smp.setflags(write=False)
        _pairs[n, seed] = (src, smp)
    return _pairs[n, seed]


def model_r(n, seed, idx):
    """(r, tolerance) of the model at one index; computed once"""
    if (n, seed, idx) not in _r:
        v, a = curve_model.r_at(*pair(n, seed), idx)
        _r[n, seed, idx] = (v, curve_model.tolerance(n, a))
    return _r[n, seed, idx]


def model_coef(n, seed, idx):
    if (n, seed, idx) not in _coef:
        _coef[n, seed, idx] = curve_model.coef_at(*pair(n, seed), idx)
    return _coef[n, seed, idx]


def centres(n):
    return [0, 1, -1, n - 1, -n, -n + 1, delays(n)[0], delays(n)[1]]


def frac_rule(r, h):
    """the header's rule in numpy float64, in its order, over the rows of r"""
    ym, y0, yp = r[:, h - 1], r[:, h], r[:, h + 1]
    s = np.where(y0 < 0.0, -1.0, 1.0)
    a, b, c = s * ym, s * y0, s * yp
    den = (a - 2.0 * b) + c
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.clip(0.5 * (a - c) / den, -0.5, 0.5)
    f = np.where(den >= 0.0, 0.0, f)
    return np.where(np.isnan(ym) | np.isnan(y0) | np.isnan(yp), np.nan, f)


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


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
    return (f64(entries * (2 * h + 1)), f64(entries * (2 * h + 1)), f64(entries), torch.full((entries,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    return all(a.cpu().tolist() == [7] * a.numel() for a in out)


def dev_curve(torch, plan, d_src, ss, d_smp, ts, batch, entries, centers, h, pool=None, coef=True):
    """the raw call on device tensors -> (r [E, 2h + 1], coef, frac [E], ret [E]) as host arrays; pool: (nsources, nsamples, pairs or None)"""
    c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.int64).reshape(-1)).cuda()
    assert c.numel() == batch * entries
    out = outputs(torch, batch * entries, h)
    ptrs = [a.data_ptr() for a in out]
    if not coef:
        ptrs[1] = 0
    torch.cuda.synchronize()
    if pool is None:
        plan.xcorr_curve_dev(d_src.data_ptr(), ss, d_smp.data_ptr(), ts, batch, entries, c.data_ptr(), h, *ptrs)
    else:
        ns, nm, rows = pool
        d_rows = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        torch.cuda.synchronize()
        plan.xcorr_pool_curve_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ts, nm, 0 if d_rows is None else d_rows.data_ptr(), batch,
                                  entries, c.data_ptr(), h, *ptrs)
    plan.sync()
    r, co, fr, rt = (a.cpu().numpy() for a in out)
    return r.reshape(-1, 2 * h + 1), co.reshape(-1, 2 * h + 1), fr, rt


# ---- 1. centres -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [1, 8])
@pytest.mark.parametrize("n", list(SHAPES))
def test_r_and_frac_around_the_centres(mod, n, h):
    src, smp = pair(n)
    cs = centres(n)
    with make_plan(mod, n) as plan:
        r, coef, frac, ret = plan.xcorr_curve_f32(src, smp, cs, half_width=h, coef=False)
    assert coef is None and r.shape == (len(cs), 2 * h + 1) and frac.shape == ret.shape == (len(cs),)
    assert ret.tolist() == [0] * len(cs)
    worst = 0.0
    for k, c in enumerate(cs):
        for j, idx in enumerate(curve_model.neighbours(c, n, h)):
            want, tol = model_r(n, 0, idx)
            err = abs(float(r[k, j]) - want)
            worst = max(worst, err / tol)
            assert err <= tol, (n, h, c, j, float(r[k, j]), want, err, tol)
    print("curve r N", n, "h", h, "worst |error| / tolerance", worst)
    assert frac.tobytes() == frac_rule(r, h).tobytes()
    for k, c in enumerate(cs):
        y = [model_r(n, 0, i)[0] for i in curve_model.neighbours(c, n, 1)]
        if abs(curve_model.phat_sub_model.den_of(*y)) > 1e-6 * abs(y[1]):
            assert abs(float(frac[k]) - curve_model.phat_sub_model.frac_of(*y)) < 1e-9, (n, h, c, float(frac[k]))
    # the planted delays are peaks of r: the vertex lies inside the frame
    assert abs(float(frac[6])) < 0.5 and abs(float(frac[7])) < 0.5 and r[6, h] > 0.5 * n and r[7, h] > 0.3 * n


# ---- 2. the coefficient -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_coef_is_the_windowed_calls_direct_form(mod, n):
    src, smp = pair(n)
    h = 8
    cs = centres(n) if n == 1000 else [0, -n, delays(n)[1]]
    with make_plan(mod, n, 16) as plan:
        r, coef, frac, ret = plan.xcorr_curve_f32(src, smp, cs, half_width=h)
        plan.set_pearson(False)
        lags = np.array([[curve_model.lag_of(i, n) for i in curve_model.neighbours(c, n, h)] for c in cs], dtype=np.int64)
        wlag, wcoef, wret = plan.xcorr_windowed_f32(src, smp, np.stack([lags.reshape(-1)] * 2, axis=1))
        if n == 144000:
            plan.set_pearson(True)
        again = plan.xcorr_curve_f32(src, smp, cs, half_width=h)
    assert wlag.tolist() == lags.reshape(-1).tolist()
    assert coef.tobytes() == wcoef.reshape(coef.shape).tobytes()
    assert same(again, (r, coef, frac, ret))                                   # whatever asx_plan_set_pearson says
    worst = 0.0
    for k, c in enumerate(cs):
        for j, idx in enumerate(curve_model.neighbours(c, n, h)):
            want = model_coef(n, 0, idx)
            assert np.isnan(coef[k, j]) == np.isnan(want), (c, j)
            if not np.isnan(want):
                worst = max(worst, abs(float(coef[k, j]) - want))
    print("curve coef N", n, "worst |coef - oracle|", worst)
    assert worst < 1e-5
    at = cs.index(-n)
    assert np.isnan(coef[at, h]) and int(wret[at * (2 * h + 1) + h]) == -1 and int(ret[at]) == 0   # lag -N: the empty segment


# ---- 3. behind a top-k call -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_behind_a_topk_call(mod, n):
    src = np.stack([pair(n, 0)[0], pair(n, 1)[0]])
    smp = np.stack([pair(n, 0)[1], pair(n, 1)[1]])
    with make_plan(mod, n) as plan:
        lag, tcoef, tret = plan.xcorr_topk_f32(src, smp, 3, 8)
        r, coef, frac, ret = plan.xcorr_curve_f32(src, smp, lag, half_width=2, entries=3)
    assert lag.shape == (2, 3) and r.shape == (2, 3, 5) and frac.shape == ret.shape == (2, 3)
    for b in range(2):
        assert lag[b].tolist() == [d + 5 * b for d in delays(n)], lag
        for j in range(3):
            want, tol = model_r(n, b, curve_model.index_of(int(lag[b, j]), n))
            assert abs(float(r[b, j, 2]) - want) <= tol, (b, j)
            assert abs(float(r[b, j, 2])) > abs(float(r[b, j, 1])) and abs(float(r[b, j, 2])) > abs(float(r[b, j, 3]))
    assert ret.tolist() == [[0] * 3] * 2 and tret.tolist() == [[0] * 3] * 2
    # the top-k call's coefficients may be the spectral form's: each within the project's 1e-5 of the reference's, as these are
    assert np.max(np.abs(coef[:, :, 2] - tcoef)) < 2e-5


# ---- 4. strides -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_strides_are_the_materialised_call(mod, torch, n):
    (s0, t0), (s1, t1) = pair(n, 0), pair(n, 1)
    cs = [delays(n)[0], -5, delays(n)[1] + 5]
    with make_plan(mod, n) as plan:
        got = plan.xcorr_curve_f32(s0, np.stack([t0, t1, t0]), cs, half_width=3)            # source_stride = 0
        assert same(got, plan.xcorr_curve_f32(np.stack([s0] * 3), np.stack([t0, t1, t0]), cs, half_width=3))
        got = plan.xcorr_curve_f32(np.stack([s0, s1, s0]), t1, cs, half_width=3)            # sample_stride = 0
        assert same(got, plan.xcorr_curve_f32(np.stack([s0, s1, s0]), np.stack([t1] * 3), cs, half_width=3))
        # overlapping windows of one recording: a hop below 2N
        hop = 4000 if n == 144000 else 10
        rec = np.concatenate([s0, s1[:2 * hop]])
        d_rec, d_t = torch.from_numpy(rec).cuda(), torch.from_numpy(np.array(t0)).cuda()
        got = dev_curve(torch, plan, d_rec, hop, d_t, 0, 3, 1, cs, 3)
        windows = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        d_w = torch.from_numpy(windows).cuda()
        assert same(got, dev_curve(torch, plan, d_w, 2 * n, d_t, 0, 3, 1, cs, 3))
        assert got[3].tolist() == [0, 0, 0] and not np.isnan(got[0]).any()


# ---- 5. batch independence --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000, 999])
def test_an_entry_does_not_depend_on_its_batch(mod, n):
    s0, t0 = pair(n, 0)
    s1, t1 = pair(n, 1)
    c = delays(n)[1]
    src = np.stack([s1] * 5 + [s0] + [s1] * 3)
    smp = np.stack([t1] * 5 + [t0] + [t1] * 3)
    cs = [3, -7, 0, n - 1, -n, c, 1, 2, -1]
    with make_plan(mod, n, 2) as plan:                       # a group of two: the batch of nine runs in five slices
        alone = plan.xcorr_curve_f32(s0, t0, [c], half_width=8)
        batch = plan.xcorr_curve_f32(src, smp, cs, half_width=8)
    assert same(alone, [a[5:6] for a in batch])


# ---- 6. invalid entries -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_invalid_entries(mod, n):
    s0, t0 = pair(n, 0)
    h = 2
    with make_plan(mod, n) as plan:
        good = plan.xcorr_curve_f32(s0, t0, [5, 6, 7, 8], half_width=h)
        got = plan.xcorr_curve_f32(s0, t0, [5, n, 7, -n - 1], half_width=h)
        assert got[3].tolist() == [0, -2, 0, -2]
        for k in (1, 3):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]).all() and np.isnan(got[2][k])
        for k in (0, 2):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        if plan.layout != "real-column":
            return
        clips = np.stack([s0, pair(n, 1)[0]])
        rows = np.array([[0, 1], [2, 0], [1, 0], [0, -1], [2, 0]], dtype=np.int32)
        ok = np.array([[0, 1], [0, 0], [1, 0], [0, 0], [0, 0]], dtype=np.int32)
        cs = [5, 6, 7, 8, n]                                  # the last: outside its pool AND outside [-N, N-1]: -4 over -2
        good = plan.xcorr_pool_curve_f32(clips, clips[:, :n], cs[:4] + [9], ok, half_width=h)
        got = plan.xcorr_pool_curve_f32(clips, clips[:, :n], cs, rows, half_width=h)
        assert got[3].tolist() == [0, -4, 0, -4, -4] and good[3].tolist() == [0] * 5
        for k in (1, 3, 4):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]).all() and np.isnan(got[2][k])
        for k in (0, 2):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        inside = plan.xcorr_pool_curve_f32(clips, clips[:, :n], [5, n], ok[:2], half_width=h)
        assert inside[3].tolist() == [0, -2]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(mod, torch):
    n = 144000
    s0, t0 = pair(n, 0)
    d_src = torch.from_numpy(np.concatenate([s0, s0[:8]])).cuda()
    d_smp = torch.from_numpy(np.concatenate([t0, t0[:8]])).cuda()
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    with make_plan(mod, n) as plan:
        def call(out, pool=False, entries=1, h=1, drop=None, src=d_src.data_ptr(), smp=d_smp.data_ptr(), ss=0, ts=0, c=d_c.data_ptr(),
                 ns=1, nm=1, batch=2, rows=d_c.data_ptr()):
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            if pool:
                plan.xcorr_pool_curve_dev(src, ss, ns, smp, ts, nm, rows, batch, entries, c, h, *ptrs)
            else:
                plan.xcorr_curve_dev(src, ss, smp, ts, batch, entries, c, h, *ptrs)
            plan.sync()

        def refused(match, **kw):
            out = outputs(torch, 16, 8)
            with pytest.raises(mod.AsxError, match=match):
                call(out, **kw)
            assert untouched(torch, out), kw

        for pool in (False, True):
            for kw in (dict(src=0), dict(smp=0), dict(c=0), dict(drop=0), dict(drop=2), dict(drop=3)):
                refused("null", pool=pool, **kw)
            for e in (0, 9, -1):
                refused("entries", pool=pool, entries=e)
            for h in (0, 9, -1, 2 ** 20):
                refused("half_width", pool=pool, h=h)
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
        assert mod.lib().asx_xcorr_curve_f32_dev(None, d_src.data_ptr(), 0, d_smp.data_ptr(), 0, 2, 1, d_c.data_ptr(), 1, *ptrs, None) == -1
        assert mod.lib().asx_xcorr_pool_curve_f32_dev(None, d_src.data_ptr(), 0, 1, d_smp.data_ptr(), 0, 1, None, 1, 1, d_c.data_ptr(), 1,
                                                      *ptrs, None) == -1
        call(out, batch=0)
        call(out, pool=True, batch=0, rows=0, ns=0, nm=0)
        assert untouched(torch, out)
        # d_coef may be NULL: the others are written, it keeps its sentinel
        out = outputs(torch, 2, 1)
        call(out, drop=1)
        assert (out[1].cpu().numpy() == 7.0).all() and out[3].cpu().tolist() == [0, 0] and not (out[0].cpu().numpy() == 7.0).any()
    m = 1000
    d_s, d_t = torch.zeros(4 * m + 4, dtype=torch.float32, device="cuda"), torch.zeros(2 * m + 4, dtype=torch.float32, device="cuda")
    with make_plan(mod, m) as plan:
        out = outputs(torch, 2, 1)
        torch.cuda.synchronize()
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.xcorr_pool_curve_dev(d_s.data_ptr(), 2 * m, 2, d_t.data_ptr(), m, 2, 0, 4, 1, d_c.data_ptr(), 1, *(a.data_ptr() for a in out))
        assert untouched(torch, out)
        # a packed plan takes any float-aligned pointer and any stride
        plan.xcorr_curve_dev(d_s.data_ptr() + 4, 2 * m + 1, d_t.data_ptr() + 12, m - 3, 2, 1, d_c.data_ptr(), 1, *(a.data_ptr() for a in out))
        plan.sync()
        assert out[3].cpu().tolist() == [0, 0] and (out[0].cpu().numpy() == 0.0).all()


def test_a_misaligned_pair_on_a_packed_plan_is_the_aligned_one(mod, torch):
    """the 4-byte fall-back of the kernel's 16-byte loads: the same tracks one and three floats into their buffers"""
    n = 999
    s0, t0 = pair(n, 0)
    cs = [delays(n)[0], -n, 0]
    with make_plan(mod, n) as plan:
        want = plan.xcorr_curve_f32(s0, t0, cs, half_width=8)
        d_s = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), s0])).cuda()
        d_t = torch.from_numpy(np.concatenate([np.zeros(3, np.float32), t0])).cuda()
        got = dev_curve(torch, plan, d_s[1:], 0, d_t[3:], 0, 3, 1, cs, 8)
    assert same(got, want)


# ---- 8. side effects --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_the_call_leaves_the_plan_as_it_was(mod, n):
    src = np.stack([pair(n, 0)[0], pair(n, 1)[0], pair(n, 0)[0]])
    smp = np.stack([pair(n, 0)[1], pair(n, 1)[1], pair(n, 1)[1]])

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes, plan.lag_window)

    with make_plan(mod, n, 2) as plan:
        before = plan.xcorr_batch_f32(src, smp)
        was = state(plan)
        got = plan.xcorr_curve_f32(src, smp, before[0], half_width=8)
        assert state(plan) == was
        plan.set_lag_window(-5, 5)
        plan.set_exact(False)
        assert same(got, plan.xcorr_curve_f32(src, smp, before[0], half_width=8))   # neither the window nor the mode plays a part
        plan.set_exact(True)
        plan.set_lag_window(-n, n - 1)
        assert state(plan) == was
        assert same(before, plan.xcorr_batch_f32(src, smp))
    assert before[0].tolist() == [delays(n)[0], delays(n)[0] + 5, before[0][2]] and got[3].tolist() == [0, 0, 0]


# ---- 9. the pool form -------------------------------------------------------------------------------------------------------------

def test_the_pool_form_is_the_strided_form_entry_by_entry(mod, torch):
    """one pool of three clips as both sources and samples (aliased: a sample is the first N frames of a clip), listed pairs, two
    entries each; then every combination"""
    n = 144000
    clips = np.stack([pair(n, 0)[0], pair(n, 1)[0], np.roll(pair(n, 0)[0], 321)])
    d_clips = torch.from_numpy(clips).cuda()
    rows = np.array([[0, 1], [2, 0], [1, 1], [2, 2], [0, 2]], dtype=np.int32)
    cs = np.array([[0, 5], [321, -n], [0, n - 1], [-1, 1], [-321, 0]], dtype=np.int64)
    with make_plan(mod, n, 2) as plan:
        ws = plan.workspace_bytes
        got = dev_curve(torch, plan, d_clips, 2 * n, d_clips, 2 * n, len(rows), 2, cs, 4, pool=(3, 3, rows))
        assert got[3].tolist() == [0] * 10 and plan.debug_bank()[:2] == (0, 0) and plan.workspace_bytes == ws
        for k, (a, b) in enumerate(rows):
            one = dev_curve(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 2, cs[k], 4)
            assert same(one, [x[2 * k:2 * k + 2] for x in got]), k
        assert got[0][2, 4] > 0.5 * n and got[0][8, 4] > 0.5 * n          # clip 2 is clip 0 delayed: peaks at +-321
        every = dev_curve(torch, plan, d_clips, 2 * n, d_clips, 2 * n, 9, 1, np.zeros(9, np.int64), 1, pool=(3, 3, None))
        for a in range(3):
            for b in range(3):
                one = dev_curve(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 1, [0], 1)
                assert same(one, [x[3 * a + b:3 * a + b + 1] for x in every]), (a, b)
