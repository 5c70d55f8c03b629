"""The host-array methods of Plan on the MI355X: each returns, bit for bit (the coefficient's float64 bits included), what its _dev
twin writes into torch buffers from the same inputs.  A real-column plan at N = 144 000 (the smallest production length), three
pairs in one launch group, with a shared 1-D operand, [B, 2] window rows, k = 2 and a band from band_bins; a packed plan at
N = 1000 for the methods packed plans support.  One plan per length."""
import numpy as np
import pytest

import oracle
from util import asx

pytestmark = pytest.mark.gpu

B, K, SEP = 3, 2, 100
RESULTS = (np.int64, np.float64, np.int32)
PHAT_RESULTS = (np.int64, np.float64, np.float64, np.int32)


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


def inputs(n):
    pairs = [oracle.synth_pair(4242, k, n, 1) for k in range(B)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    lags = [int(p[2]) for p in pairs]
    # a row round each planted lag, one of them the whole range
    rows = np.array([(max(-n, lags[0] - 50), min(n - 1, lags[0] + 50)), (-n, n - 1), (max(-n, lags[2] - 7), min(n - 1, lags[2] + 900))],
                    dtype=np.int64)
    return src, smp, rows


class Twin:
    """runs a _dev method on device copies of host arrays and brings back what it wrote"""

    def __init__(self, torch, plan):
        self.torch, self.plan = torch, plan

    def run(self, method, host_inputs, make_args, shape, dtypes):
        """make_args(*input pointers) -> the method's arguments up to the result pointers, which follow"""
        t = self.torch
        dev = [None if a is None else t.from_numpy(np.ascontiguousarray(a)).cuda() for a in host_inputs]
        kind = {np.int64: t.int64, np.float64: t.float64, np.int32: t.int32}
        out = [t.zeros(shape, dtype=kind[d], device="cuda") for d in dtypes]
        t.cuda.synchronize()
        method(*make_args(*[0 if d is None else d.data_ptr() for d in dev]), *[o.data_ptr() for o in out])
        self.plan.sync()
        return tuple(o.cpu().numpy() for o in out)


def same(got, want, dtypes, shape):
    assert len(got) == len(want) == len(dtypes)
    for g, w, d in zip(got, want, dtypes):
        assert g.dtype == w.dtype == d and g.shape == w.shape == shape, (g.dtype, g.shape, shape)
        assert g.tobytes() == w.tobytes(), (g, w)


def test_real_column_host_methods_return_what_their_dev_twins_write(mod, torch):
    from audiosync_amd.hipxcorr import position_rows
    n = 144000
    src, smp, rows = inputs(n)
    lo, hi = mod.band_bins(n, 48000.0, 300.0, 3400.0)
    hop = 48000
    rec = np.concatenate([src[0], src[1][:2 * hop]])
    listed = np.array([[2, 0], [0, 1], [1, 1]], dtype=np.int32)
    with mod.Plan(n, B, 0) as plan:
        assert plan.layout == "real-column" and plan.group == B
        tw = Twin(torch, plan)
        # one track against many: the shared source is 1-D
        same(plan.xcorr_broadcast_f32(src[0], smp),
             tw.run(plan.xcorr_strided_dev, (src[0], smp), lambda s, t: (s, 0, t, n, B), (B,), RESULTS), RESULTS, (B,))
        same(plan.xcorr_windowed_f32(src, smp, rows),
             tw.run(plan.xcorr_windowed_dev, (src, smp, rows), lambda s, t, w: (s, 2 * n, t, n, w, 1, B), (B,), RESULTS), RESULTS, (B,))
        same(plan.xcorr_windowed_f32(src, smp[1], rows[1]),
             tw.run(plan.xcorr_windowed_dev, (src, smp[1], rows[1]), lambda s, t, w: (s, 2 * n, t, 0, w, 0, B), (B,), RESULTS), RESULTS, (B,))
        # windows of one recording, every lag and by position
        same(plan.xcorr_windows_f32(rec, smp[0], hop),
             tw.run(plan.xcorr_strided_dev, (rec, smp[0]), lambda s, t: (s, hop, t, 0, 3), (3,), RESULTS), RESULTS, (3,))
        k0, k1, prow = position_rows(n, hop, 3, 0, 2 * hop)
        assert (k0, k1) == (0, 3)
        same(plan.xcorr_windows_f32(rec, smp[0], hop, positions=(0, 2 * hop)),
             tw.run(plan.xcorr_windowed_dev, (rec, smp[0], prow), lambda s, t, w: (s, hop, t, 0, w, 1, 3), (3,), RESULTS), RESULTS, (3,))
        # top-k with the plan's window and with rows
        same(plan.xcorr_topk_f32(src, smp, K, SEP),
             tw.run(plan.xcorr_topk_dev, (src, smp, None), lambda s, t, w: (s, 2 * n, t, n, w, 0, B, K, SEP), (B, K), RESULTS), RESULTS, (B, K))
        same(plan.xcorr_topk_f32(src[0], smp, K, SEP, rows),
             tw.run(plan.xcorr_topk_dev, (src[0], smp, rows), lambda s, t, w: (s, 0, t, n, w, 1, B, K, SEP), (B, K), RESULTS), RESULTS, (B, K))
        # GCC-PHAT, whole and banded: four results
        same(plan.xcorr_phat_f32(src, smp),
             tw.run(plan.xcorr_phat_dev, (src, smp, None), lambda s, t, w: (s, 2 * n, t, n, w, 0, B), (B,), PHAT_RESULTS), PHAT_RESULTS, (B,))
        same(plan.xcorr_phat_f32(src[0], smp, rows),
             tw.run(plan.xcorr_phat_dev, (src[0], smp, rows), lambda s, t, w: (s, 0, t, n, w, 1, B), (B,), PHAT_RESULTS), PHAT_RESULTS, (B,))
        same(plan.xcorr_phat_band_f32(src, smp, lo, hi),
             tw.run(plan.xcorr_phat_band_dev, (src, smp, None), lambda s, t, w: (s, 2 * n, t, n, w, 0, B, lo, hi), (B,), PHAT_RESULTS),
             PHAT_RESULTS, (B,))
        same(plan.xcorr_phat_band_f32(src, smp[2], lo, hi, rows),
             tw.run(plan.xcorr_phat_band_dev, (src, smp[2], rows), lambda s, t, w: (s, 2 * n, t, 0, w, 1, B, lo, hi), (B,), PHAT_RESULTS),
             PHAT_RESULTS, (B,))
        # pools: listed pairs with rows, and every combination of one source with three samples ([S, R] results)
        same(plan.xcorr_pool_f32(src, smp[:2], listed, rows),
             tw.run(plan.xcorr_pool_dev, (src, smp[:2], listed, rows), lambda s, t, p, w: (s, 2 * n, B, t, n, 2, p, w, 1, B), (B,), RESULTS),
             RESULTS, (B,))
        same(plan.xcorr_pool_f32(src[:1], smp),
             tw.run(plan.xcorr_pool_dev, (src[:1], smp, None, None), lambda s, t, p, w: (s, 2 * n, 1, t, n, B, p, w, 0, B), (1, B), RESULTS),
             RESULTS, (1, B))
        same(plan.xcorr_pool_topk_f32(src, smp[:2], K, SEP, listed, rows[0]),
             tw.run(plan.xcorr_pool_topk_dev, (src, smp[:2], listed, rows[0]),
                    lambda s, t, p, w: (s, 2 * n, B, t, n, 2, p, w, 0, B, K, SEP), (B, K), RESULTS), RESULTS, (B, K))
        same(plan.xcorr_pool_topk_f32(src[:1], smp, K, SEP),
             tw.run(plan.xcorr_pool_topk_dev, (src[:1], smp, None, None),
                    lambda s, t, p, w: (s, 2 * n, 1, t, n, B, p, w, 0, B, K, SEP), (1, B, K), RESULTS), RESULTS, (1, B, K))


def test_packed_host_methods_return_what_their_dev_twins_write(mod, torch):
    n = 1000
    src, smp, rows = inputs(n)
    with mod.Plan(n, B, 0) as plan:
        assert plan.layout == "packed" and plan.group == B
        tw = Twin(torch, plan)
        same(plan.xcorr_broadcast_f32(src, smp[0]),
             tw.run(plan.xcorr_strided_dev, (src, smp[0]), lambda s, t: (s, 2 * n, t, 0, B), (B,), RESULTS), RESULTS, (B,))
        same(plan.xcorr_windowed_f32(src, smp, rows),
             tw.run(plan.xcorr_windowed_dev, (src, smp, rows), lambda s, t, w: (s, 2 * n, t, n, w, 1, B), (B,), RESULTS), RESULTS, (B,))
        same(plan.xcorr_topk_f32(src, smp, K, 10, rows),
             tw.run(plan.xcorr_topk_dev, (src, smp, rows), lambda s, t, w: (s, 2 * n, t, n, w, 1, B, K, 10), (B, K), RESULTS), RESULTS, (B, K))
        same(plan.xcorr_topk_f32(src, smp, K, 10),
             tw.run(plan.xcorr_topk_dev, (src, smp, None), lambda s, t, w: (s, 2 * n, t, n, w, 0, B, K, 10), (B, K), RESULTS), RESULTS, (B, K))
