"""The lag track on the MI355X (asx_xcorr_track_f32_dev, asx_xcorr_pool_track_f32_dev and their Plan methods).

r must be the float64 model's sum (tests/track_model.py: math.fsum over the exact products of a segment) at every lag of every segment
within len_s * 2^-53 * sum |products| -- the first-order worst case of any float64 summation order; seg must be the header's rule
applied to the call's own r, bit for bit; fit must be the model's line through the call's own seg within the model's first-order
tolerances (track_model.fit_tolerances); a planted drift must come back within half a frame over the window; with S = 1 and h = 8
r must be the curve call's r byte for byte (one sweep, the same blocks, the same order).  Shapes: N = 1000 on a
packed plan (25 x 40), N = 999, which no block size divides, and N = 144 000, the smallest real-column length, where S = 1 with h = 8
runs three blocks per segment and the sum kernel and everything else one block per (segment, tile).

Measured worst error / tolerance (h = 8, 9 and 64; the whole table: profiles/track/cost.txt):
    r                N = 1000: 1.0e-3 (S = 1), 1.4e-2 (S = 8), 0.12 (S = 64);  N = 999: 1.1e-3, 1.5e-2, 0.16;
                     N = 144 000: 6.6e-6 (S = 1), 1.1e-4 (S = 16) -- the tolerance shrinks with the segment
    sum over s       5.1e-4 of twice the curve call's tolerance
    drift, lag0      6.0e-4, 4.7e-4 (N = 999, S = 8)
    rms^2            1.2e-3 (N = 1000, S = 8)
Planted drift, drift * N: 11.80 / 11.83 (total 12), -11.84 / -11.84 (total -12), 40.09 / 40.10 (total 40); total 0: 0.0017 / 0.0011
(N = 1000) and 0.0004 / 0.0001 (N = 144 000) -- the float64 model's figures.
"""
import ctypes
import math

import numpy as np
import pytest

import track_model
from test_gpu_curve import delays, pair, same
from util import asx

pytestmark = pytest.mark.gpu

SHAPES = {1000: "25x40x8", 144000: None, 999: None}
SEGS = {1000: (1, 8, 64), 999: (1, 8, 64), 144000: (1, 16)}
_rows = {}
worst = {"r": 0.0, "sum": 0.0, "drift": 0.0, "lag0": 0.0, "rms2": 0.0}


def model_rows(n, idx):
    """the model at one index of pair(n): {S: (r_s [S], tolerance [S])} for every S of SEGS[n]; computed once"""
    if (n, idx) not in _rows:
        src, smp = pair(n)
        prod = src.astype(np.float64)[(np.arange(n) + int(idx)) % (2 * n)] * smp.astype(np.float64)
        p, a = prod.tolist(), np.abs(prod).tolist()
        out = {}
        for segs in SEGS[n]:
            b = track_model.bounds(n, segs)
            out[segs] = ([math.fsum(p[b[s]:b[s + 1]]) for s in range(segs)],
                         [track_model.tol_r(b[s + 1] - b[s], math.fsum(a[b[s]:b[s + 1]])) for s in range(segs)])
        _rows[n, idx] = out
    return _rows[n, idx]


def centres(n):
    return [0, -1, n - 1, -n, delays(n)[0], delays(n)[1]]


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


def outputs(torch, entries, h, segs):
    f64 = lambda count: torch.full((count,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda count: torch.full((count,), 7, dtype=torch.int32, device="cuda")  # noqa: E731
    return (f64(entries * segs * (2 * h + 1)), f64(entries * segs * 2), f64(entries * 3), i32(entries), i32(entries))


def untouched(torch, out):
    torch.cuda.synchronize()
    return all(bool((a == 7).all().item()) for a in out)


def dev_track(torch, plan, d_src, ss, d_smp, ts, batch, entries, centers, h, segs, pool=None, seg=True):
    """the raw call on device tensors -> (r [E, S, 2h + 1], seg [E, S, 2], fit [E, 3], used [E], ret [E]) as host arrays; pool:
    (nsources, nsamples, pairs or None); seg False: a null d_seg"""
    c = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.int64).reshape(-1)).cuda()
    assert c.numel() == batch * entries
    out = outputs(torch, batch * entries, h, segs)
    ptrs = [a.data_ptr() for a in out]
    if not seg:
        ptrs[1] = 0
    torch.cuda.synchronize()
    if pool is None:
        plan.xcorr_track_dev(d_src.data_ptr(), ss, d_smp.data_ptr(), ts, batch, entries, c.data_ptr(), h, segs, *ptrs)
    else:
        ns, nm, rows = pool
        d_rows = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        torch.cuda.synchronize()
        plan.xcorr_pool_track_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ts, nm, 0 if d_rows is None else d_rows.data_ptr(), batch,
                                  entries, c.data_ptr(), h, segs, *ptrs)
    plan.sync()
    r, sg, ft, us, rt = (a.cpu().numpy() for a in out)
    return r.reshape(-1, segs, 2 * h + 1), sg.reshape(-1, segs, 2), ft.reshape(-1, 3), us, rt


def check_r(n, h, segs, c, r):
    """one entry's r [S, 2h + 1] against the model"""
    for j, idx in enumerate(track_model.indices(c, n, h)):
        want, tol = model_rows(n, idx)[segs]
        for s in range(segs):
            err = abs(float(r[s, j]) - want[s])
            worst["r"] = max(worst["r"], err / tol[s])
            assert err <= tol[s], (n, h, segs, c, s, j, float(r[s, j]), want[s], err, tol[s])


def check_seg_and_fit(n, h, segs, r, seg, fit, used, ret):
    """the call's own r -> its seg bit for bit, its used, and its fit within the model's tolerances; -> the used counts"""
    t = track_model.times(n, segs)
    counts = []
    for k in range(r.shape[0]):
        assert int(ret[k]) == 0
        want, use = track_model.seg_of(r[k], h)
        assert seg[k].tobytes() == want.tobytes(), (n, h, segs, k, seg[k].tolist(), want.tolist())
        f = track_model.fit(t, want[:, 0], want[:, 1], use)
        assert int(used[k]) == f["count"] == int(use.sum()), (n, h, segs, k)
        counts.append(f["count"])
        if f["count"] < 2:
            assert np.isnan(fit[k]).all(), (n, h, segs, k, fit[k])
            continue
        td, tl, tr = track_model.fit_tolerances(t, want[:, 0], want[:, 1], use, f, segs)
        errs = (abs(float(fit[k, 0]) - f["drift"]), abs(float(fit[k, 1]) - f["lag0"]), abs(float(fit[k, 2]) ** 2 - f["rms2"]))
        for name, e, tol in zip(("drift", "lag0", "rms2"), errs, (td, tl, tr)):
            worst[name] = max(worst[name], e / tol)
            assert e <= tol, (name, n, h, segs, k, e, tol, fit[k].tolist(), f)
    return counts


# ---- 1. r against the model, 2. seg and fit against the rule ----------------------------------------------------------------------

@pytest.mark.parametrize("n, segs", [(n, s) for n in (1000, 999) for s in SEGS[n]])
def test_r_seg_and_fit_at_the_small_lengths(mod, n, segs):
    src, smp = pair(n)
    cs = centres(n)
    worst.update(dict.fromkeys(worst, 0.0))
    with make_plan(mod, n) as plan:
        for h in (8, 9, 64):                                   # one tile, two tiles, eight tiles with a short last one
            r, seg, fit, used, ret = plan.xcorr_track_f32(src, smp, cs, h, segs)
            assert r.shape == (len(cs), segs, 2 * h + 1) and seg.shape == (len(cs), segs, 2) and fit.shape == (len(cs), 3)
            assert used.shape == ret.shape == (len(cs),) and ret.tolist() == [0] * len(cs)
            for k, c in enumerate(cs):
                check_r(n, h, segs, c, r[k])
            counts = check_seg_and_fit(n, h, segs, r, seg, fit, used, ret)
            if segs == 8:
                assert counts[4] == counts[5] == 8, counts       # the planted lags: every segment peaks at the centre
                assert np.abs(seg[4:, :, 0]).max() < 0.5 and abs(fit[4, 0] * n) < 0.5 and fit[4, 2] < 0.5
            if segs == 1:
                assert np.isnan(fit).all() and set(used.tolist()) <= {0, 1}
            if h == 8:                                           # over s the sums add up to the curve call's r
                cr = plan.xcorr_curve_f32(src, smp, cs, half_width=h, coef=False)[0]
                if segs == 1:                                    # one segment, one tile: the curve call's sweep, block for block
                    assert r[:, 0, :].tobytes() == cr.tobytes(), (n, np.argwhere(r[:, 0, :] != cr).tolist())
                for k, c in enumerate(cs):
                    for j, idx in enumerate(track_model.indices(c, n, h)):
                        tol = model_rows(n, idx)[1][1][0]                 # S = 1: the curve call's own tolerance
                        err = abs(math.fsum(r[k, :, j].tolist()) - float(cr[k, j]))
                        worst["sum"] = max(worst["sum"], err / (2 * tol))
                        assert err <= 2 * tol, (n, segs, c, j, err, tol)
    print("track N", n, "S", segs, "worst error / tolerance", worst)


@pytest.mark.parametrize("segs", SEGS[144000])
def test_r_seg_and_fit_at_144000(mod, segs):
    n = 144000
    src, smp = pair(n)
    cs = centres(n)
    worst.update(dict.fromkeys(worst, 0.0))
    with make_plan(mod, n) as plan:
        for h in (8, 9):
            r, seg, fit, used, ret = plan.xcorr_track_f32(src, smp, cs, h, segs)
            for k in (3, 5):                                     # the model for few entries only: lag -N and a planted lag
                check_r(n, h, segs, cs[k], r[k])
            counts = check_seg_and_fit(n, h, segs, r, seg, fit, used, ret)
            assert counts[4] == counts[5] == segs, counts
            if h == 8:
                cr = plan.xcorr_curve_f32(src, smp, cs, half_width=h, coef=False)[0]
                if segs == 1:                                    # three blocks per entry in both calls, added in the same order
                    assert r[:, 0, :].tobytes() == cr.tobytes(), np.argwhere(r[:, 0, :] != cr).tolist()
                for k in (3, 5):
                    for j, idx in enumerate(track_model.indices(cs[k], n, h)):
                        tol = model_rows(n, idx)[1][1][0]
                        err = abs(math.fsum(r[k, :, j].tolist()) - float(cr[k, j]))
                        worst["sum"] = max(worst["sum"], err / (2 * tol))
                        assert err <= 2 * tol, (segs, k, j, err, tol)
        r, seg, fit, used, ret = plan.xcorr_track_f32(src, smp, [-1], 64, segs)    # h = 64 for one entry, across the wrap
        check_r(n, 64, segs, -1, r[0])
        check_seg_and_fit(n, 64, segs, r, seg, fit, used, ret)
    print("track N", n, "S", segs, "worst error / tolerance", worst)


# ---- 3. a planted drift -----------------------------------------------------------------------------------------------------------

def drifting_pair(n, segs, l0, total):
    """white noise and a sample that follows it at the lag l0 + k_s in segment s, k_s = round(total * (b_s + b_{s+1}) / 2 / N)"""
    rng = np.random.default_rng(200)
    src = rng.standard_normal(2 * n).astype(np.float32)
    noise = rng.standard_normal(n)
    b = track_model.bounds(n, segs)
    smp = np.zeros(n)
    for s in range(segs):
        k = int(round(total * (b[s] + b[s + 1]) / 2 / n))
        at = np.arange(b[s], b[s + 1])
        smp[at] = src[(at + l0 + k) % (2 * n)]
    return src, (smp + 0.1 * noise).astype(np.float32)


@pytest.mark.parametrize("n, segs, h, total", [(1000, 8, 16, 12), (999, 8, 16, -12), (144000, 16, 32, 40), (1000, 8, 16, 0), (144000, 16, 32, 0)])
def test_a_planted_drift_comes_back(mod, n, segs, h, total):
    with make_plan(mod, n) as plan:
        for l0 in (n // 3 + 1, -(n // 4) - 3):
            src, smp = drifting_pair(n, segs, l0, total)
            r, seg, fit, used, ret = plan.xcorr_track_f32(src, smp, [l0 + total // 2], h, segs)
            print("track drift N", n, "l0", l0, "total", total, "drift * N", float(fit[0, 0]) * n, "lag0", float(fit[0, 1]), "rms", float(fit[0, 2]))
            assert int(ret[0]) == 0 and int(used[0]) == segs, (l0, used, seg[0].tolist())
            if total:
                assert abs(float(fit[0, 0]) * n - total) < 0.5, (l0, float(fit[0, 0]) * n)
            else:
                assert abs(float(fit[0, 0]) * n) < 0.01, (l0, float(fit[0, 0]) * n)


# ---- 4. structure -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 144000])
def test_an_entry_depends_on_neither_its_batch_nor_the_plan(mod, n):
    s0, t0 = pair(n, 0)
    s1, t1 = pair(n, 1)
    c = delays(n)[1]
    src = np.stack([s1] * 3 + [s0] + [s1])
    smp = np.stack([t1] * 3 + [t0] + [t1])
    cs = [3, -7, n - 1, c, -n]
    for h, segs in ((8, 1), (9, 8)):                             # N = 144 000: three blocks per segment and the sum kernel; one block
        got = []
        for max_batch in (1, 4):
            with make_plan(mod, n, max_batch) as plan:
                got.append(plan.xcorr_track_f32(s0, t0, [c], h, segs))
                got.append(tuple(a[3:4] for a in plan.xcorr_track_f32(src, smp, cs, h, segs)))
        for other in got[1:]:
            assert same(got[0], other), (n, h, segs)
        assert int(got[0][4][0]) == 0 and not np.isnan(got[0][0]).any()


@pytest.mark.parametrize("n", [1000, 144000])
def test_broadcast_strides_and_entries(mod, n):
    (s0, t0), (s1, t1) = pair(n, 0), pair(n, 1)
    cs = [delays(n)[0], -5, delays(n)[1] + 5]
    with make_plan(mod, n) as plan:
        got = plan.xcorr_track_f32(s0, np.stack([t0, t1, t0]), cs, 9, 4)                       # source_stride = 0
        assert same(got, plan.xcorr_track_f32(np.stack([s0] * 3), np.stack([t0, t1, t0]), cs, 9, 4))
        got = plan.xcorr_track_f32(np.stack([s0, s1, s0]), t1, cs, 9, 4)                       # sample_stride = 0
        assert same(got, plan.xcorr_track_f32(np.stack([s0, s1, s0]), np.stack([t1] * 3), cs, 9, 4))
        three = plan.xcorr_track_f32(np.stack([s0, s1]), np.stack([t0, t1]), [cs, cs[::-1]], 9, 4, entries=3)
        assert three[0].shape == (2, 3, 4, 19) and three[1].shape == (2, 3, 4, 2) and three[2].shape == (2, 3, 3) and three[3].shape == (2, 3)
        for b, (s, t) in enumerate(((s0, t0), (s1, t1))):
            for j in range(3):
                one = plan.xcorr_track_f32(s, t, [[cs, cs[::-1]][b][j]], 9, 4)
                assert same(one, [a[b, j:j + 1] for a in three]), (b, j)


def test_the_pool_form_is_the_strided_form_entry_by_entry(mod, torch):
    n = 144000
    clips = np.stack([pair(n, 0)[0], pair(n, 1)[0], np.roll(pair(n, 0)[0], 321)])
    d_clips = torch.from_numpy(clips).cuda()
    rows = np.array([[0, 1], [2, 0], [1, 1], [2, 2], [0, 2]], dtype=np.int32)
    cs = np.array([[0, 5], [321, -n], [0, n - 1], [-1, 1], [-321, 0]], dtype=np.int64)
    with make_plan(mod, n, 2) as plan:
        ws = plan.workspace_bytes
        for h, segs in ((8, 1), (20, 4)):
            got = dev_track(torch, plan, d_clips, 2 * n, d_clips, 2 * n, len(rows), 2, cs, h, segs, pool=(3, 3, rows))
            assert got[4].tolist() == [0] * 10 and plan.debug_bank()[:2] == (0, 0) and plan.workspace_bytes == ws
            for k, (a, b) in enumerate(rows):
                one = dev_track(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 2, cs[k], h, segs)
                assert same(one, [x[2 * k:2 * k + 2] for x in got]), (h, segs, k)
            assert (got[0][2, :, h] > 0.5 * n / segs).all() and (got[0][8, :, h] > 0.5 * n / segs).all()   # clip 2 is clip 0 delayed
        every = dev_track(torch, plan, d_clips, 2 * n, d_clips, 2 * n, 9, 1, np.zeros(9, np.int64), 1, 2, pool=(3, 3, None))
        for a in range(3):
            for b in range(3):
                one = dev_track(torch, plan, d_clips[a], 0, d_clips[b], 0, 1, 1, [0], 1, 2)
                assert same(one, [x[3 * a + b:3 * a + b + 1] for x in every]), (a, b)
        # the Plan method is the raw call
        assert same(plan.xcorr_pool_track_f32(clips, clips[:, :n], cs, 20, 4, pairs=rows, entries=2),
                    [x.reshape((5, 2) + x.shape[1:]) for x in got])


@pytest.mark.parametrize("n", [1000, 144000])
def test_invalid_entries(mod, n):
    s0, t0 = pair(n, 0)
    h, segs = 9, 4
    with make_plan(mod, n) as plan:
        good = plan.xcorr_track_f32(s0, t0, [5, 6, 7, 8], h, segs)
        got = plan.xcorr_track_f32(s0, t0, [5, n, 7, -n - 1], h, segs)
        assert got[4].tolist() == [0, -2, 0, -2] and got[3].tolist() == [good[3][0], 0, good[3][2], 0]
        for k in (1, 3):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]).all() and np.isnan(got[2][k]).all()
        for k in (0, 2):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        if plan.layout != "real-column":
            return
        clips = np.stack([s0, pair(n, 1)[0]])
        rows = np.array([[0, 1], [2, 0], [1, 0], [0, -1], [2, 0]], dtype=np.int32)
        ok = np.array([[0, 1], [0, 0], [1, 0], [0, 0], [0, 0]], dtype=np.int32)
        cs = [5, 6, 7, 8, n]                                  # the last: outside its pool AND outside [-N, N-1]: -4 over -2
        good = plan.xcorr_pool_track_f32(clips, clips[:, :n], cs[:4] + [9], h, segs, pairs=ok)
        got = plan.xcorr_pool_track_f32(clips, clips[:, :n], cs, h, segs, pairs=rows)
        assert got[4].tolist() == [0, -4, 0, -4, -4] and good[4].tolist() == [0] * 5
        for k in (1, 3, 4):
            assert np.isnan(got[0][k]).all() and np.isnan(got[1][k]).all() and np.isnan(got[2][k]).all() and int(got[3][k]) == 0
        for k in (0, 2):
            assert same([a[k] for a in got], [a[k] for a in good]), k
        inside = plan.xcorr_pool_track_f32(clips, clips[:, :n], [5, n], h, segs, pairs=ok[:2])
        assert inside[4].tolist() == [0, -2]


# ---- 5. refusals and side effects -------------------------------------------------------------------------------------------------

def test_refusals(mod, torch):
    n = 144000
    s0, t0 = pair(n, 0)
    d_src = torch.from_numpy(np.concatenate([s0, s0[:8]])).cuda()
    d_smp = torch.from_numpy(np.concatenate([t0, t0[:8]])).cuda()
    d_c = torch.zeros(2, dtype=torch.int64, device="cuda")
    with make_plan(mod, n) as plan:
        def call(out, pool=False, entries=1, h=1, segs=1, drop=None, src=d_src.data_ptr(), smp=d_smp.data_ptr(), ss=0, ts=0,
                 c=d_c.data_ptr(), ns=1, nm=1, batch=2, rows=d_c.data_ptr()):
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            if pool:
                plan.xcorr_pool_track_dev(src, ss, ns, smp, ts, nm, rows, batch, entries, c, h, segs, *ptrs)
            else:
                plan.xcorr_track_dev(src, ss, smp, ts, batch, entries, c, h, segs, *ptrs)
            plan.sync()

        def refused(match, **kw):
            out = outputs(torch, 2, 2, 2)
            with pytest.raises(mod.AsxError, match=match):
                call(out, **kw)
            assert untouched(torch, out), kw

        for pool in (False, True):
            for kw in (dict(src=0), dict(smp=0), dict(c=0), dict(drop=0), dict(drop=2), dict(drop=3), dict(drop=4)):
                refused("null", pool=pool, **kw)
            for e in (0, 9, -1):
                refused("entries", pool=pool, entries=e)
            for h in (0, 65, -1, 2 ** 20):
                refused("half_width", pool=pool, h=h)
            for s in (0, 65, -1, 2 ** 20):
                refused("segments", pool=pool, segs=s)
            refused("aligned", pool=pool, src=d_src.data_ptr() + 4)
            refused("aligned", pool=pool, smp=d_smp.data_ptr() + 8)
            refused("multiples of 4", pool=pool, ss=2)
            refused("multiples of 4", pool=pool, ts=n + 1)
        refused("every combination", pool=True, rows=0, ns=1, nm=1, batch=2)
        refused("empty pool", pool=True, ns=0)
        refused("empty pool", pool=True, nm=0)
        # a NULL plan (the raw symbol), and batch == 0 returns 0 with nothing written
        out = outputs(torch, 2, 1, 1)
        torch.cuda.synchronize()
        ptrs = [ctypes.c_void_p(a.data_ptr()) for a in out]
        assert mod.lib().asx_xcorr_track_f32_dev(None, d_src.data_ptr(), 0, d_smp.data_ptr(), 0, 2, 1, d_c.data_ptr(), 1, 1, *ptrs, None) == -1
        assert mod.lib().asx_xcorr_pool_track_f32_dev(None, d_src.data_ptr(), 0, 1, d_smp.data_ptr(), 0, 1, None, 1, 1, d_c.data_ptr(), 1, 1,
                                                      *ptrs, None) == -1
        call(out, batch=0)
        call(out, pool=True, batch=0, rows=0, ns=0, nm=0)
        assert untouched(torch, out)
        # d_seg may be NULL: the others are written, it keeps its sentinel
        out = outputs(torch, 2, 1, 1)
        call(out, drop=1)
        assert (out[1].cpu().numpy() == 7.0).all() and out[4].cpu().tolist() == [0, 0] and not (out[0].cpu().numpy() == 7.0).any()
        assert np.isnan(out[2].cpu().numpy()).all() and set(out[3].cpu().tolist()) <= {0, 1}
    m = 1000
    d_s, d_t = torch.zeros(4 * m + 4, dtype=torch.float32, device="cuda"), torch.zeros(2 * m + 4, dtype=torch.float32, device="cuda")
    with make_plan(mod, m) as plan:
        out = outputs(torch, 4, 1, 1)
        torch.cuda.synchronize()
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.xcorr_pool_track_dev(d_s.data_ptr(), 2 * m, 2, d_t.data_ptr(), m, 2, 0, 4, 1, d_c.data_ptr(), 1, 1, *(a.data_ptr() for a in out))
        assert untouched(torch, out)
        # a packed plan takes any float-aligned pointer and any stride; an all-zero segment peaks at -h and is not used
        out = outputs(torch, 2, 1, 1)
        plan.xcorr_track_dev(d_s.data_ptr() + 4, 2 * m + 1, d_t.data_ptr() + 12, m - 3, 2, 1, d_c.data_ptr(), 1, 1, *(a.data_ptr() for a in out))
        plan.sync()
        assert out[4].cpu().tolist() == [0, 0] and (out[0].cpu().numpy() == 0.0).all() and out[3].cpu().tolist() == [0, 0]
        assert out[1].cpu().tolist() == [-1.0, 0.0] * 2
    # segments may not exceed N; segments = N is one frame per segment, and 2h + 1 > 2N goes round the circle
    m = 49
    rng = np.random.default_rng(7)
    src, smp = rng.standard_normal(2 * m).astype(np.float32), rng.standard_normal(m).astype(np.float32)
    with mod.Plan(m, 1, 0) as plan:
        d_s, d_t = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        out = outputs(torch, 1, 1, m + 1)
        torch.cuda.synchronize()
        with pytest.raises(mod.AsxError, match="segments"):
            plan.xcorr_track_dev(d_s.data_ptr(), 0, d_t.data_ptr(), 0, 1, 1, d_c.data_ptr(), 1, m + 1, *(a.data_ptr() for a in out))
        assert untouched(torch, out)
        r, seg, fit, used, ret = dev_track(torch, plan, d_s, 0, d_t, 0, 1, 1, [-3], 64, m)
        want, tol = track_model.track_r(src, smp, -3, 64, m)
        assert int(ret[0]) == 0 and (np.abs(r[0] - want) <= tol).all()
        check_seg_and_fit(m, 64, m, r, seg, fit, used, ret)


@pytest.mark.parametrize("n", [1000, 144000])
def test_the_call_leaves_the_plan_as_it_was(mod, torch, n):
    src = np.stack([pair(n, 0)[0], pair(n, 1)[0], pair(n, 0)[0]])
    smp = np.stack([pair(n, 0)[1], pair(n, 1)[1], pair(n, 1)[1]])

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes, plan.lag_window, plan.debug_bank())

    with make_plan(mod, n, 2) as plan:
        before = plan.xcorr_batch_f32(src, smp)
        was = state(plan)
        got = plan.xcorr_track_f32(src, smp, before[0], 20, 8)
        assert state(plan) == was
        plan.set_lag_window(-5, 5)
        plan.set_exact(False)
        assert same(got, plan.xcorr_track_f32(src, smp, before[0], 20, 8))       # neither the window nor the mode plays a part
        plan.set_exact(True)
        plan.set_lag_window(-n, n - 1)
        assert state(plan) == was
        assert same(before, plan.xcorr_batch_f32(src, smp))
        was = state(plan)                                        # (the batch call counted its Pearson modes)
        # the Plan method is the raw call
        d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
        assert same(got, dev_track(torch, plan, d_src, 2 * n, d_smp, n, 3, 1, before[0], 20, 8))
        assert state(plan) == was
    assert got[4].tolist() == [0, 0, 0] and got[3].tolist()[:2] == [8, 8]
