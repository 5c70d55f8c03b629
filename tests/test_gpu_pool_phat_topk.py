"""Top-k GCC-PHAT over track pools on the MI355X (asx_xcorr_pool_phat_topk_f32_dev, Plan.xcorr_pool_phat_topk_f32): k = 1 is the pool
PHAT call; every pair is the strided PHAT top-k call on that pair alone, listed over several launch groups and as every combination;
indices outside the pools; the refusals; and end to end, the tables of four clips with a shared hum and an echo each through
asx_pool_closure_dev."""
import numpy as np
import pytest

import closure_model as cm
import phat_topk_model
from test_gpu_closure import assert_same
from test_gpu_pool import shifted
from util import asx

pytestmark = pytest.mark.gpu

N = 144000
INT32_MAX = 2 ** 31 - 1
BANDS = [(0, N), (1, N // 6)]


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


def all_bits(out):
    return [np.ascontiguousarray(a).tobytes() for a in out]


def entry_bits(out, i, k):
    """the k entries of pair i of outputs of any shape [..., k]"""
    return [np.ascontiguousarray(np.asarray(a).reshape(-1, k)[i]).tobytes() for a in out]


def alone(plan, src, smp, k, sep, band, windows=None):
    """the pair alone through the strided PHAT top-k call"""
    return plan.xcorr_phat_topk_f32(src, smp[None, :], k, sep, windows, band)


def is_refused(out, i, k, code):
    lag, coef, peak, ret = (np.asarray(a).reshape(-1, k)[i] for a in out)
    return lag.tolist() == [0] * k and ret.tolist() == [code] * k and np.isnan(coef).all() and np.isnan(peak).all()


def outputs(torch, b):
    return (torch.full((b,), -99, dtype=torch.int64, device="cuda"), torch.full((b,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((b,), 7.0, dtype=torch.float64, device="cuda"), torch.full((b,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    b = out[0].numel()
    return [a.cpu().tolist() for a in out] == [[-99] * b, [7.0] * b, [7.0] * b, [7] * b]


@pytest.fixture(scope="module")
def pools():
    """3 sources and 3 samples: sample b hears source b over two paths (noise 0.1), so every pair (b, b) has two entries that stand
    out and every other pair ranks the noise floor"""
    rng = np.random.default_rng(53)
    src = rng.standard_normal((3, 2 * N)).astype(np.float32)
    smp = np.stack([shifted(src[b], 4000 * (b + 1) * (-1) ** b, rng) + 0.6 * shifted(src[b], -9000 + 700 * b, rng) for b in range(3)])
    return src, smp.astype(np.float32)


@pytest.mark.parametrize("band", BANDS)
def test_k1_is_the_pool_phat_call(mod, pools, band):
    src, smp = pools
    pairs = np.array([[2, 2], [0, 1], [7, 0], [1, 1], [0, 0]], dtype=np.int32)
    rows = np.array([(-N, N - 1), (-500, 500), (0, 0), (3, 2), (100, 9000)], dtype=np.int64)
    with mod.Plan(N, 2, 0) as plan:
        for pr, w in ((None, None), (pairs, None), (pairs, rows)):
            want = plan.xcorr_pool_phat_f32(src, smp, pr, w, band)
            got = plan.xcorr_pool_phat_topk_f32(src, smp, 1, 300, pr, w, band)
            assert got[0].shape == want[0].shape + (1,) and all_bits(got) == all_bits(want), (band, pr is None, w is None)
            three = plan.xcorr_pool_phat_topk_f32(src, smp, 3, 300, pr, w, band)
            assert all_bits([a[..., 0] for a in three]) == all_bits(want), (band, pr is None, w is None)


@pytest.mark.parametrize("band", BANDS)
def test_every_pair_is_the_strided_call_on_that_pair_alone(mod, pools, band):
    """11 listed pairs on a plan of four pairs a group (two full groups and a partial one), with repeats, out of order, a row that is
    not a window and a row that two zones use up; then d_pairs == NULL over the 3 x 3 pool"""
    src, smp = pools
    k, sep = 3, 250
    pairs = np.array([[2, 2], [0, 0], [0, 0], [1, 2], [1, 1], [2, 0], [0, 1], [2, 2], [1, 1], [0, 2], [2, 1]], dtype=np.int32)
    rows = np.tile(np.array([[-N, N - 1]], dtype=np.int64), (len(pairs), 1))
    rows[2] = (3900, 4400)
    rows[3] = (9, 8)
    rows[4] = (-9000, -7000)
    with mod.Plan(N, 4, 0) as plan:
        assert plan.group == 4
        fills = plan.debug_bank()[2]
        for windows in (None, rows):
            got = plan.xcorr_pool_phat_topk_f32(src, smp, k, sep, pairs, windows, band)
            assert got[0].shape == (len(pairs), k)
            for i, (a, b) in enumerate(pairs):
                want = alone(plan, src[a], smp[b], k, sep, band, None if windows is None else windows[i])
                assert entry_bits(got, i, k) == entry_bits(want, 0, k), (band, windows is None, i, a, b)
            assert got[0][1].tolist()[:2] == [4000, -9000] and got[0][4].tolist()[:2] == [-8000, -8300], got[0]
        assert plan.debug_bank()[2] == fills + 2                      # the bank is filled once per pool call, whatever k is
        assert is_refused(got, 3, k, -2)
        # the row 3900..4400: the path at 4000, one of the 150 lags its zone leaves, whose zone takes the rest
        assert got[3][2].tolist() == [0, 0, -3] and got[0][2][0] == 4000 and 4250 < got[0][2][1] <= 4400 and got[0][2][2] == 0, [a[2] for a in got]
        assert np.isnan(got[1][2][2]) and np.isnan(got[2][2][2])
        every = plan.xcorr_pool_phat_topk_f32(src, smp, k, sep, band=band)
        assert every[0].shape == (3, 3, k)
        for a in range(3):
            for b in range(3):
                assert entry_bits(every, 3 * a + b, k) == entry_bits(alone(plan, src[a], smp[b], k, sep, band), 0, k), (band, a, b)


def test_indices_outside_the_pools(mod, pools):
    """-1, nsources, nsamples and INT32_MAX give (0, NaN, NaN, -4) in all k entries, one of them over a row that is not a window and
    one over a row that runs out; every other pair is what the same call returns without the bad rows"""
    src, smp = pools
    k, sep, band = 4, 300, (1, N // 6)
    bad = [[-1, 0], [3, 0], [0, 3], [0, -1], [INT32_MAX, 1], [1, INT32_MAX]]
    good = [[0, 0], [2, 2], [1, 1]]
    pairs = np.array([good[0], bad[0], bad[1], good[1], bad[2], bad[3], good[2], bad[4], good[1], bad[5]], dtype=np.int32)
    is_bad = np.array([p in bad for p in pairs.tolist()])
    rows = np.tile(np.array([[-N, N - 1]], dtype=np.int64), (len(pairs), 1))
    rows[2] = (5, 4)                                   # -4 takes precedence over -2
    rows[4] = (10, 12)                                 # ... and over -3
    rows[6] = (7, 6)                                   # a pair inside its pools whose row is not a window: -2
    with mod.Plan(N, 4, 0) as plan:
        for windows in (None, rows):
            got = plan.xcorr_pool_phat_topk_f32(src, smp, k, sep, pairs, windows, band)
            ref = plan.xcorr_pool_phat_topk_f32(src, smp, k, sep, pairs[~is_bad], None if windows is None else windows[~is_bad], band)
            j = 0
            for i, p in enumerate(pairs.tolist()):
                if is_bad[i]:
                    assert is_refused(got, i, k, -4), (i, p, [a[i] for a in got])
                else:
                    assert entry_bits(got, i, k) == entry_bits(ref, j, k), (i, p)
                    j += 1
            assert got[0][3].tolist()[:2] == [12000, -7600] and got[3][3].tolist() == [0] * k
            if windows is not None:
                assert is_refused(got, 6, k, -2), [a[6] for a in got]


def test_refusals(mod, torch, pools):
    src, smp = pools
    k = 3
    d_src, d_smp = torch.from_numpy(np.concatenate([src.ravel(), src[0][:8]])).cuda(), torch.from_numpy(smp).cuda()
    d_pairs = torch.tensor([[0, 0], [1, 1]], dtype=torch.int32, device="cuda")
    with mod.Plan(N, 2, 0) as plan:
        good = dict(src=d_src.data_ptr(), ss=2 * N, ns=3, smp=d_smp.data_ptr(), ts=N, nm=3, pairs=d_pairs.data_ptr(), batch=2, lo=100,
                    hi=1000, k=k, sep=10)
        bad = [("k = 0", dict(k=0)), ("k = 9", dict(k=9)), ("negative", dict(sep=-1)), ("not a band", dict(lo=5, hi=4)),
               ("not a band", dict(hi=N + 1)), ("null", dict(src=0)), ("null", dict(smp=0)), ("null", dict(drop=1)),
               ("null", dict(drop=3)), ("aligned", dict(src=d_src.data_ptr() + 4)), ("multiples of 4", dict(ss=6)),
               ("empty pool", dict(ns=0)), ("every combination", dict(pairs=0, batch=5))]
        for text, change in bad:
            a = dict(good)
            a.update(change)
            out = outputs(torch, 9 * k)
            ptrs = [t.data_ptr() for t in out]
            if "drop" in a:
                ptrs[a["drop"]] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_pool_phat_topk_dev(a["src"], a["ss"], a["ns"], a["smp"], a["ts"], a["nm"], a["pairs"], 0, 0, a["batch"], a["lo"],
                                              a["hi"], a["k"], a["sep"], *ptrs)
            assert untouched(torch, out), (text, change)
        out = outputs(torch, 9 * k)
        plan.xcorr_pool_phat_topk_dev(good["src"], 2 * N, 3, good["smp"], N, 3, good["pairs"], 0, 0, 0, 100, 1000, k, 10,
                                      *(t.data_ptr() for t in out))     # batch == 0
        assert untouched(torch, out)
    m = 1000  # a length outside the tuned table: a packed plan
    d_s, d_t = torch.zeros(4 * m, dtype=torch.float32, device="cuda"), torch.zeros(2 * m, dtype=torch.float32, device="cuda")
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        out = outputs(torch, 4 * k)
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.xcorr_pool_phat_topk_dev(d_s.data_ptr(), 2 * m, 2, d_t.data_ptr(), m, 2, 0, 0, 0, 4, 0, m, k, 10, *(t.data_ptr() for t in out))
        assert untouched(torch, out)


def test_end_to_end_through_closure(mod):
    """four clips cut from one noise recording at planted offsets, each with the shared 50 Hz hum and an echo of its own (the decoy
    lags): all pairs with k = 3 through the pool call, then asx_pool_closure_dev.  The device's tables, fed to tests/closure_model.py,
    reproduce the device's closure outputs byte for byte, and the offsets are the planted ones.  The seed was pinned on the CPU
    models alone (tests/test_phat_topk.py: seeds 20270, 20271 and 20272 were looked at, all three place the clips)."""
    C, k = 4, phat_topk_model.E2E_K
    clips = phat_topk_model.e2e_clips()
    with mod.Plan(N, C * C, 0) as plan:
        lag, coef, peak, ret = plan.xcorr_pool_phat_topk_f32(clips, clips[:, :N], k, phat_topk_model.E2E_SEP)
    assert lag.shape == (C, C, k) and (peak[:, :, 0] > 0.2).all() and (np.diff(peak, axis=2) <= 0).all(), peak
    got = mod.pool_closure(lag, coef, ret, phat_topk_model.E2E_TOL, 1, votes=True)
    assert_same(got, cm.closure(lag, coef, ret, phat_topk_model.E2E_TOL, 1), "device tables")
    phat_topk_model.check_e2e(lag, ret, got)
