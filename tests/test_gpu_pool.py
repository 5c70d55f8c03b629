"""Listed pairs of two track pools on the MI355X (asx_xcorr_pool_f32_dev, Plan.xcorr_pool_f32, Plan.xcorr_pool_dev).

Every pair must give, bit for bit, what the strided call gives for that pair alone on the same plan (with a row: the windowed call
with that row), in both Pearson forms, in exact and asynchronous mode; an index outside its pool gives (0, NaN, -4) and leaves the
other pairs alone.  The planted pairs are also checked against the float64 oracle."""
import numpy as np
import pytest

import oracle
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
PRODUCTION = (144000, 288000, 480000, 720000, 960000, 1440000)
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    return t


def bits(out, k):
    return [np.asarray(a).reshape(-1)[k].tobytes() for a in out]


def alone(plan, src, smp):
    """the pair alone through the strided path (asx_xcorr_strided_f32_dev, one pair)"""
    return plan.xcorr_broadcast_f32(src, smp[None, :])


def shifted(src, lag, rng, noise=0.1):
    """a sample whose true lag against src is `lag`"""
    n = src.size // 2
    idx = (np.arange(n) + lag % (2 * n)) % (2 * n)
    return (src[idx] + noise * rng.standard_normal(n)).astype(np.float32)


def outputs(torch, batch):
    return (torch.full((batch,), -99, dtype=torch.int64, device="cuda"), torch.full((batch,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((batch,), 7, dtype=torch.int32, device="cuda"))


def pool_dev(plan, torch, d_src, ss, ns, d_smp, ms, nm, pairs, batch, windows=None, ws=0):
    d_pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda() if pairs is not None else None
    d_win = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.int64)).cuda() if windows is not None else None
    lag, coef, ret = outputs(torch, batch)
    torch.cuda.synchronize()
    plan.xcorr_pool_dev(d_src.data_ptr(), ss, ns, d_smp.data_ptr(), ms, nm, d_pairs.data_ptr() if d_pairs is not None else 0,
                        d_win.data_ptr() if d_win is not None else 0, ws, batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr())
    plan.sync()
    return lag.cpu().numpy(), coef.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("spectral", [True, False])
@pytest.mark.parametrize("n", PRODUCTION)
def test_small_matrix_at_every_length(mod, n, spectral):
    """3 sources x 2 samples: planted offsets of both signs, the rest unrelated; every pair equals the strided call alone"""
    rng = np.random.default_rng(n % 1000 + 5)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    l0, l1 = n // 3 + 17, -(n // 5) - 3
    smp = np.stack([shifted(src[0], l0, rng), shifted(src[2], l1, rng)])
    with mod.Plan(n, 8, 0) as plan:
        assert plan.layout == "real-column"
        plan.set_pearson(spectral)
        fills = plan.debug_bank()[2]
        got = plan.xcorr_pool_f32(src, smp)
        assert plan.debug_bank()[:2] == (3, 2) and plan.debug_bank()[2] == fills + 1
        assert got[0].shape == (3, 2)
        for a in range(3):
            for b in range(2):
                assert bits(got, 2 * a + b) == bits(alone(plan, src[a], smp[b]), 0), (n, spectral, a, b)
        for (a, b), lag in (((0, 0), l0), ((2, 1), l1)):
            o_ret, o_lag, o_coef = oracle.cross_correlation(src[a], smp[b])
            assert (int(got[2][a, b]), int(got[0][a, b])) == (o_ret, o_lag) == (0, lag), (n, a, b)
            assert abs(float(got[1][a, b]) - o_coef) < COEF_TOL
        assert abs(float(got[1][1, 0])) < 0.1   # an unrelated pair


def test_explicit_list_aliases_and_overlapping_windows(mod, torch):
    """arbitrary order and duplicates; one pool of clips as both sources and samples; a source pool of overlapping windows"""
    n, hop = 144000, 36000
    rng = np.random.default_rng(17)
    rec = rng.standard_normal(2 * n + 5 * hop).astype(np.float32)          # windows k * hop .. k * hop + 2N, k = 0..5
    nwin = 6
    clips = np.stack([np.concatenate([shifted(rec[k * hop:k * hop + 2 * n], (-1) ** k * (1000 + 7 * k), rng),
                                      rng.standard_normal(n).astype(np.float32)]) for k in range(4)])   # [4, 2N]
    pairs = np.array([[3, 1], [0, 0], [0, 0], [5, 2], [1, 3], [2, 2], [4, 0], [0, 3]], dtype=np.int32)
    d_rec = torch.from_numpy(rec).cuda()
    d_clips = torch.from_numpy(clips).cuda()
    with mod.Plan(n, 8, 0) as plan:
        # windows of the recording (stride hop) against the clips read as samples (their first N frames, stride 2N)
        got = pool_dev(plan, torch, d_rec, hop, nwin, d_clips, 2 * n, 4, pairs, len(pairs))
        for i, (a, b) in enumerate(pairs):
            want = alone(plan, rec[a * hop:a * hop + 2 * n], clips[b, :n])
            assert bits(got, i) == bits(want, 0), (i, a, b)
        assert bits(got, 1) == bits(got, 2)
        for k in range(4):
            i = [j for j, (a, b) in enumerate(pairs) if a == k and b == k]
            for j in i:
                assert int(got[0][j]) == (-1) ** k * (1000 + 7 * k) and int(got[2][j]) == 0
        # all-pairs of one pool: the same buffer as sources (2N) and samples (its first N frames)
        allp = np.array([[a, b] for a in range(4) for b in range(4) if a != b][::-1], dtype=np.int32)
        got = pool_dev(plan, torch, d_clips, 2 * n, 4, d_clips, 2 * n, 4, allp, len(allp))
        for i, (a, b) in enumerate(allp):
            assert bits(got, i) == bits(alone(plan, clips[a], clips[b, :n]), 0), (i, a, b)


def test_per_pair_windows_match_the_windowed_call(mod):
    n = 288000
    rng = np.random.default_rng(23)
    src = rng.standard_normal((2, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[0], 5000, rng) + 0.6 * shifted(src[0], -9000, rng), shifted(src[1], -777, rng)])
    pairs = np.array([[0, 0], [0, 0], [1, 1], [0, 1], [1, 1]], dtype=np.int32)
    rows = np.array([[-n, n - 1], [-20000, -1000], [-800, -700], [3, 2], [10, 20]], dtype=np.int64)   # row 3 is not a window
    with mod.Plan(n, 8, 0) as plan:
        got = plan.xcorr_pool_f32(src, smp, pairs, rows)
        for i, (a, b) in enumerate(pairs):
            want = plan.xcorr_windowed_f32(src[a], smp[b][None, :], rows[i])
            assert bits(got, i) == bits(want, 0), (i, rows[i])
        assert (int(got[0][0]), int(got[0][1]), int(got[0][2]), int(got[2][3])) == (5000, -9000, -777, -2)
        # one row for every pair
        got = plan.xcorr_pool_f32(src, smp, pairs, np.array([-800, 6000], dtype=np.int64))
        for i, (a, b) in enumerate(pairs):
            assert bits(got, i) == bits(plan.xcorr_windowed_f32(src[a], smp[b][None, :], (-800, 6000)), 0), i


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_several_launch_groups(mod, monkeypatch, lanes):
    """group 3, one and two lanes: consecutive groups share slots; the bank is filled once per call"""
    monkeypatch.setenv("ASX_LANES", lanes)
    n = 144000
    rng = np.random.default_rng(29)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    lags = [(k * 37717) % n - n // 2 for k in range(4)]
    smp = np.stack([shifted(src[k % 3], lags[k], rng, 0.3) for k in range(4)])
    pairs = np.array([[k % 3, k % 4] for k in range(10)] + [[0, 3], [0, 3]], dtype=np.int32)
    with mod.Plan(n, 3, 0) as plan:
        assert plan.group == 3
        f0 = plan.debug_bank()[2]
        got = plan.xcorr_pool_f32(src, smp, pairs)
        assert plan.debug_bank()[2] == f0 + 1
        for i, (a, b) in enumerate(pairs):
            assert bits(got, i) == bits(alone(plan, src[a], smp[b]), 0), (lanes, i)
            if a == b % 3:
                assert int(got[0][i]) == lags[b]
        full = plan.xcorr_pool_f32(src, smp)
        assert plan.debug_bank()[2] == f0 + 2
        for a in range(3):
            for b in range(4):
                assert bits(full, 4 * a + b) == bits(alone(plan, src[a], smp[b]), 0), (lanes, a, b)


def periodic_pools(n):
    base = np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32)
    per = np.tile(base, 2 * n // 8)             # 2N/8 exactly tied peaks: a pair of it with a cut of it overflows
    rng = np.random.default_rng(8)
    src = np.stack([per, rng.standard_normal(2 * n).astype(np.float32)])
    smp = np.stack([per[:n], per[8:n + 8], per[3:n + 3], rng.standard_normal(n).astype(np.float32)])
    return src, smp


def test_overflowing_pairs(mod):
    """the periodic track: the second look runs on the listed pairs, the counters and bits equal the strided call's, ret = 1 in the
    asynchronous mode"""
    n = 144000
    src, smp = periodic_pools(n)
    pairs = np.array([[1, 3], [0, 0], [0, 1], [1, 0], [0, 2], [0, 3], [0, 0]], dtype=np.int32)
    with mod.Plan(n, 8, 0) as plan:
        assert plan.peak_capacity < 2 * n
        want = []
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        for a, b in pairs:
            want.append(alone(plan, src[a], smp[b]))
        w_over, w_rep = plan.peak_overflows() - o0, plan.peak_repairs() - r0
        assert w_over >= 3 and w_rep == w_over
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        got = plan.xcorr_pool_f32(src, smp, pairs)
        assert (plan.peak_overflows() - o0, plan.peak_repairs() - r0) == (w_over, w_rep)
        for i in range(len(pairs)):
            assert bits(got, i) == bits(want[i], 0), i
        o_ret, o_lag, _ = oracle.cross_correlation(src[0], smp[0])
        assert (int(got[2][1]), int(got[0][1]), float(got[1][1])) == (o_ret, o_lag, 1.0)
        plan.set_exact(False)
        try:
            want = [alone(plan, src[a], smp[b]) for a, b in pairs]
            o0, r0 = plan.peak_overflows(), plan.peak_repairs()
            got = plan.xcorr_pool_f32(src, smp, pairs)
            assert plan.peak_overflows() - o0 == w_over and plan.peak_repairs() == r0
            assert int((got[2] == 1).sum()) == w_over and got[2][1] == 1
            for i in range(len(pairs)):
                assert bits(got, i) == bits(want[i], 0), i
        finally:
            plan.set_exact(True)


def test_invalid_rows(mod):
    """indices outside their pools give (0, NaN, -4), next to ordinary and overflowing pairs, which stay as they are alone"""
    n = 144000
    src, smp = periodic_pools(n)
    rng = np.random.default_rng(31)
    src = np.concatenate([src, rng.standard_normal((1, 2 * n)).astype(np.float32)])
    smp = np.concatenate([smp, shifted(src[2], 4321, rng)[None, :]])
    ns, nm = src.shape[0], smp.shape[0]
    bad = [[-1, 0], [ns, 0], [0, nm], [0, -1], [INT32_MAX, 1], [1, INT32_MAX], [-2 ** 31, -2 ** 31]]
    good = [[0, 0], [2, 4], [1, 3]]
    pairs = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2], bad[4], good[0], bad[5], bad[6]], dtype=np.int32)
    is_bad = np.array([list(p) in bad for p in pairs.tolist()])
    rows = np.tile(np.array([[-n, n - 1]], dtype=np.int64), (len(pairs), 1))
    rows[2] = (5, 4)                                   # -4 takes precedence over -2
    rows[3] = (4000, 5000)
    with mod.Plan(n, 4, 0) as plan:
        want = {tuple(p): alone(plan, src[p[0]], smp[p[1]]) for p in good}
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        got = plan.xcorr_pool_f32(src, smp, pairs)
        assert (plan.peak_overflows() - o0, plan.peak_repairs() - r0) == (2, 2)   # pairs 0 and 8: (0, 0) twice
        for i, p in enumerate(pairs.tolist()):
            if is_bad[i]:
                assert int(got[0][i]) == 0 and np.isnan(got[1][i]) and int(got[2][i]) == -4, (i, p)
            else:
                assert bits(got, i) == bits(want[tuple(p)], 0), (i, p)
        assert int(got[0][3]) == 4321
        got = plan.xcorr_pool_f32(src, smp, pairs, rows)
        for i, p in enumerate(pairs.tolist()):
            if is_bad[i]:
                assert (int(got[0][i]), int(got[2][i])) == (0, -4) and np.isnan(got[1][i]), (i, p)
            else:
                assert bits(got, i) == bits(plan.xcorr_windowed_f32(src[p[0]], smp[p[1]][None, :], rows[i]), 0), (i, p)


def test_bad_arguments_leave_the_outputs_alone(mod, torch, monkeypatch):
    n = 144000
    rng = np.random.default_rng(37)
    d_src = torch.from_numpy(rng.standard_normal(3 * 2 * n).astype(np.float32)).cuda()
    d_smp = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    d_pairs = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    lag, coef, ret = outputs(torch, 6)
    L, C, R = lag.data_ptr(), coef.data_ptr(), ret.data_ptr()
    S, T, P = d_src.data_ptr(), d_smp.data_ptr(), d_pairs.data_ptr()

    def rejected(plan, *args):
        with pytest.raises(mod.AsxError):
            plan.xcorr_pool_dev(*args)
        torch.cuda.synchronize()
        assert (lag == -99).all() and (coef == 7.0).all() and (ret == 7).all()

    with mod.Plan(n, 4, 0) as plan:
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, L, 0, R)              # no coefficients
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, L, C, 0)              # no ret
        rejected(plan, 0, 2 * n, 3, T, n, 2, P, 0, 0, 4, L, C, R)              # no sources
        rejected(plan, S, 2 * n, 3, 0, n, 2, P, 0, 0, 4, L, C, R)              # no samples
        rejected(plan, S, 2 * n, 0, T, n, 2, P, 0, 0, 4, L, C, R)              # empty source pool
        rejected(plan, S, 2 * n, 3, T, n, 0, P, 0, 0, 4, L, C, R)              # empty sample pool
        rejected(plan, S + 4, 2 * n, 3, T, n, 2, P, 0, 0, 4, L, C, R)          # not 16-byte aligned
        rejected(plan, S, 2 * n + 2, 2, T, n, 2, P, 0, 0, 4, L, C, R)          # stride not a multiple of 4
        rejected(plan, S, 2 * n, 3, T, n, 2, 0, 0, 0, 5, L, C, R)              # implicit product of 3 x 2 is 6 pairs
        plan.xcorr_pool_dev(S, 2 * n, 3, T, n, 2, P, 0, 0, 0, L, C, R)         # batch 0: nothing
        plan.sync()
        assert (lag == -99).all() and (ret == 7).all()
    monkeypatch.setenv("ASX_LAYOUT", "packed")
    with mod.Plan(n, 4, 0) as plan:
        assert plan.layout == "packed"
        rejected(plan, S, 2 * n, 3, T, n, 2, P, 0, 0, 4, L, C, R)


def test_other_calls_after_a_pool_call(mod, torch):
    """a strided broadcast call and a contiguous call after a pool call return what they return on a plan that never made one"""
    n = 480000
    rng = np.random.default_rng(41)
    src = rng.standard_normal((3, 2 * n)).astype(np.float32)
    smp = np.stack([shifted(src[k], 1000 * (k + 1) * (-1) ** k, rng) for k in range(3)])
    with mod.Plan(n, 4, 0) as fresh:
        w_bc = fresh.xcorr_broadcast_f32(src[0], smp)
        w_ct = fresh.xcorr_batch_f32(src, smp)
    with mod.Plan(n, 4, 0) as plan:
        pool = plan.xcorr_pool_f32(src, smp)
        bc = plan.xcorr_broadcast_f32(src[0], smp)
        ct = plan.xcorr_batch_f32(src, smp)
        pool2 = plan.xcorr_pool_f32(src, smp)
    for i in range(3):
        assert bits(bc, i) == bits(w_bc, i) and bits(ct, i) == bits(w_ct, i), i
        assert bits(pool, 3 * i + i) == bits(w_ct, i), i
        assert bits(pool, 3 * 0 + i) == bits(w_bc, i), i
    for a, b in zip(pool, pool2):
        assert a.tobytes() == b.tobytes()


def test_a_bank_no_device_can_hold(mod, torch):
    """A pool call that names more tracks than any device holds (2^31 - 1 sources, the most the entry point accepts: a bank of about
    3.7e15 bytes) fails before anything is launched, names the bank, and leaves the plan without one -- the old bank is released
    before the new one is asked for -- and the next call builds it again and returns what it returned before"""
    n = 144000
    rng = np.random.default_rng(43)
    d_src = torch.from_numpy(rng.standard_normal(2 * 2 * n).astype(np.float32)).cuda()
    d_smp = torch.from_numpy(rng.standard_normal(2 * n).astype(np.float32)).cuda()
    with mod.Plan(n, 4, 0) as plan:
        assert plan.layout == "real-column"
        first = pool_dev(plan, torch, d_src, 2 * n, 2, d_smp, n, 2, None, 4)
        assert plan.debug_bank() == (2, 2, 1)
        with pytest.raises(mod.AsxError, match="bank"):   # (the exception's text is asx_last_error's)
            pool_dev(plan, torch, d_src, 2 * n, INT32_MAX, d_smp, n, 2, [[0, 0]], 1)
        assert plan.debug_bank() == (0, 0, 1)
        again = pool_dev(plan, torch, d_src, 2 * n, 2, d_smp, n, 2, None, 4)
        assert plan.debug_bank() == (2, 2, 2)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
