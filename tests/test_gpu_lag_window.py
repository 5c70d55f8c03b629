"""Lag window of the peak search on the MI355X (asx_plan_set_lag_window, asx_stream_set_lag_window, audiosync_set_max_lag_ms).

Every case is checked against tests/lag_window_model.py: the reference's max_abs_index (src/cross_correlation.c:52-67) over the
in-window elements of the oracle's float64 results[], the reference's segments and pearson_coefficient -- lag and ret exactly,
the coefficient within 1e-5.  The full window must change nothing, bit for bit."""
import sys

import numpy as np
import pytest

import oracle
from lag_window_model import model
from util import asx, graft

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
PRODUCTION = (144000, 288000, 480000, 720000, 960000, 1440000)


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def check(got, want, what):
    lag, coef, ret = got
    w_ret, w_lag, w_coef = want
    assert (int(ret), int(lag)) == (w_ret, w_lag), (what, got, want)
    if w_ret == 0:
        assert abs(float(coef) - w_coef) < COEF_TOL, (what, got, want)


def bits(*arrays):
    return [np.asarray(a).tobytes() for a in arrays]


def decoy_pair(n, a, b, seed):
    """a source of noise; the sample a strong copy of it at lag a plus a weaker copy at lag b (r[k] = sum source[(i + k) mod 2N]
    sample[i]: a copy at index k puts a peak at k)"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(2 * n).astype(np.float32)
    i = np.arange(n)
    ka, kb = a % (2 * n), b % (2 * n)
    smp = (src[(i + ka) % (2 * n)] + 0.6 * src[(i + kb) % (2 * n)] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    return src, smp


@pytest.mark.parametrize("n", PRODUCTION)
def test_full_window_is_a_no_op(mod, n):
    """[-N, N-1] set explicitly, or a window set and the full one restored: the bits of a plan that never had a window, through
    the batch, the broadcast form and the double ABI, both Pearson forms"""
    src0, smp0, _ = oracle.synth_pair(91, 0, n, 1)
    src1, smp1, _ = oracle.synth_pair(91, 1, n, 1)
    src, smp = np.stack([src0, src1]), np.stack([smp0, smp1])

    def run(plan):
        out = []
        for spectral in (True, False):
            plan.set_pearson(spectral)
            out += bits(*plan.xcorr_batch_f32(src, smp))
            out += bits(*plan.xcorr_broadcast_f32(src0, smp))
        out.append(repr(plan.xcorr_f64(src0.astype(np.float64), smp0.astype(np.float64))))
        return out

    with mod.Plan(n, 2, 0) as plan:
        assert plan.lag_window == (-n, n - 1)
        ref = run(plan)
        plan.set_lag_window(-n, n - 1)
        assert run(plan) == ref
        plan.set_lag_window(-n // 7, n // 5)
        plan.xcorr_batch_f32(src, smp)
        plan.set_lag_window(-n, n - 1)
        assert run(plan) == ref


def test_stream_full_window_is_a_no_op(mod):
    n = 144000
    src, smp, _ = oracle.synth_pair(92, 0, n, 1)
    out = []
    for window in (None, (-10 ** 12, 10 ** 12), (-n, n - 1)):
        st = mod.Stream(n, 0)
        try:
            if window:
                st.set_lag_window(*window)
            st.append(src.astype(np.float64), smp.astype(np.float64))
            out.append(st.xcorr(n))
        finally:
            st.close()
    assert out[0] == out[1] == out[2], out


DECOYS = [  # (a = the strong copy, b = the weaker one, window that holds b and not a)
    (5000, 20000, (10000, 30000)),          # positive lags
    (-5000, -20000, (-30000, -10000)),      # negative lags
    (30000, -3000, (-10000, 10000)),        # straddling 0
]


@pytest.mark.parametrize("layout", ["real-column", "packed", "non-smooth"])
def test_decoy_outside_the_window(mod, monkeypatch, layout):
    n = 7000 * 7 if layout == "non-smooth" else 144000       # 2N = 98 000 = 2^4 5^3 7^2: embedded in a longer transform
    if layout == "packed":
        monkeypatch.setenv("ASX_LAYOUT", "packed")
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == ("real-column" if layout == "real-column" else "packed"), plan.layout
        for k, (a, b, (lo, hi)) in enumerate(DECOYS):
            src, smp = decoy_pair(n, a, b, k)
            r = oracle.cross_correlation(src, smp, want_results=True)[3]
            full = model(src, smp, r=r)
            assert full[1] == a
            plan.set_lag_window(-n, n - 1)
            lag, coef, ret = plan.xcorr_batch_f32(src, smp)
            check((lag[0], coef[0], ret[0]), full, ("full", a, b))
            want = model(src, smp, lo, hi, r=r)
            assert want[1] == b
            plan.set_lag_window(lo, hi)
            lag, coef, ret = plan.xcorr_batch_f32(src, smp)
            check((lag[0], coef[0], ret[0]), want, ("window", lo, hi))
            r64 = plan.xcorr_f64(src.astype(np.float64), smp.astype(np.float64))
            check((r64[1], r64[2], r64[0]), want, ("f64", lo, hi))


@pytest.mark.parametrize("layout", ["real-column", "packed"])
def test_seed_rule(mod, monkeypatch, layout):
    n = 144000
    if layout == "packed":
        monkeypatch.setenv("ASX_LAYOUT", "packed")
    src, _ = decoy_pair(n, 0, 0, 5)
    i = np.arange(n)
    with mod.Plan(n, 1, 0) as plan:
        # a silent sample: the seed's lag, and the NaN coefficient gives ret = -1
        zero = np.zeros(n, dtype=np.float32)
        for lo, hi in ((100, 200), (-200, -100), (-n, -n), (n - 1, n - 1), (-50, 60)):
            plan.set_lag_window(lo, hi)
            want = model(src, zero, lo, hi)
            lag, coef, ret = plan.xcorr_batch_f32(src, zero)
            assert want[:2] == (-1, 0 if lo < 0 <= hi else lo), (lo, hi, want)
            assert (int(ret[0]), int(lag[0])) == want[:2], (lo, hi)
        # a large NEGATIVE r at the seed loses to a smaller positive |r| later in the window
        s0 = 1000
        smp = (-src[(i + s0) % (2 * n)] + 0.3 * src[(i + s0 + 50) % (2 * n)]).astype(np.float32)
        r = oracle.cross_correlation(src, smp, want_results=True)[3]
        assert r[s0] < 0 and abs(r[s0]) > abs(r[s0 + 50])
        plan.set_lag_window(s0, s0 + 100)
        want = model(src, smp, s0, s0 + 100, r=r)
        assert want[1] == s0 + 50
        lag, coef, ret = plan.xcorr_batch_f32(src, smp)
        check((lag[0], coef[0], ret[0]), want, "negative seed")
        # one-lag windows, the two ends of the range included
        for l in (s0, s0 + 50, -n, n - 1, -1, 0):
            plan.set_lag_window(l, l)
            want = model(src, smp, l, l, r=r)
            assert want[1] == l
            lag, coef, ret = plan.xcorr_batch_f32(src, smp)
            check((lag[0], coef[0], ret[0]), want, ("one lag", l))


@pytest.mark.parametrize("n", [144000, 480000])
def test_unchanged_peak_means_unchanged_bits(mod, n):
    pairs = [oracle.synth_pair(93, p, n, 1) for p in range(4)]
    src = np.stack([p[0] for p in pairs])
    smp = np.stack([p[1] for p in pairs])
    with mod.Plan(n, 4, 0) as plan:
        for spectral in (True, False):
            plan.set_pearson(spectral)
            plan.set_lag_window(-n, n - 1)
            full = plan.xcorr_batch_f32(src, smp)
            for lo, hi in ((-n // 3, n // 3), (-n, n // 2), (-n // 2, n - 1)):
                plan.set_lag_window(lo, hi)
                got = plan.xcorr_batch_f32(src, smp)
                for p in range(4):
                    r = oracle.cross_correlation(src[p], smp[p], want_results=True)[3]
                    want = model(src[p], smp[p], lo, hi, r=r)
                    if want[1] == model(src[p], smp[p], r=r)[1]:
                        assert [got[k][p].tobytes() for k in range(3)] == [full[k][p].tobytes() for k in range(3)], (spectral, lo, hi, p)
                    else:
                        check((got[0][p], got[1][p], got[2][p]), want, (spectral, lo, hi, p))


def test_exact_under_the_window(mod):
    """a source periodic in 8 frames: exactly tied peaks every 8 lags, more of them inside the window than the plan's list holds"""
    n = 48000
    base = np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32)
    per = np.tile(base, 2 * n // 8)
    smp = per[:n].copy()
    # r exactly: integer products, periodic in 8
    r8 = np.array([np.dot(np.roll(base, -k).astype(np.float64), base.astype(np.float64)) for k in range(8)]) * (n // 8)
    r = r8[np.arange(2 * n) % 8]
    lo, hi = 1003, 40000
    want = model(per, smp, lo, hi, r=r)
    assert want[1] == 1008
    with mod.Plan(n, 1, 0) as plan:
        assert (hi - lo) // 8 > plan.peak_capacity
        plan.set_lag_window(lo, hi)
        rep0 = plan.peak_repairs()
        lag, coef, ret = plan.xcorr_batch_f32(per, smp)
        check((lag[0], coef[0], ret[0]), want, "exact")
        assert plan.peak_repairs() > rep0
        r64 = plan.xcorr_f64(per.astype(np.float64), smp.astype(np.float64))
        check((r64[1], r64[2], r64[0]), want, "exact f64")
        import torch
        d_src = torch.from_numpy(per).cuda()
        d_smp = torch.from_numpy(smp).cuda()
        d_lag = torch.full((1,), -99, dtype=torch.int64, device="cuda")
        d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
        d_ret = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.set_exact(False)
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), 1, d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
        assert int(d_ret[0]) == 1 and lo <= int(d_lag[0]) <= hi
        plan.set_exact(True)
        # debug_r: the whole of r comes back, the lag is the window's
        d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
        assert (int(d_ret[0]), int(d_lag[0])) == (0, 1008)
        got_r = d_r.cpu().numpy().astype(np.float64) / plan.fft_len   # the device's r is F times the plain sum
        assert np.max(np.abs(got_r - r)) <= 1e-5 * np.max(np.abs(r))


def test_strided_forms_equal_contiguous_calls_with_the_window(mod):
    n, hop, batch = 144000, 36000, 6
    rng = np.random.default_rng(11)
    rec = rng.standard_normal(2 * n + hop * (batch - 1)).astype(np.float32)
    smp = (rec[200000: 200000 + n] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    with mod.Plan(n, batch, 0) as plan:
        for lo, hi in ((-n // 4, n // 4), (20000, 90000)):
            plan.set_lag_window(lo, hi)
            got = plan.xcorr_windows_f32(rec, smp, hop)
            srcs = np.stack([rec[k * hop: k * hop + 2 * n] for k in range(batch)])
            smps = np.stack([smp] * batch)
            want = plan.xcorr_batch_f32(srcs, smps)
            assert bits(*got) == bits(*want), (lo, hi)
            got_b = plan.xcorr_broadcast_f32(srcs[0], smps)
            want_b = plan.xcorr_batch_f32(np.stack([srcs[0]] * batch), smps)
            assert bits(*got_b) == bits(*want_b), (lo, hi)
            for k in range(batch):
                check((want[0][k], want[1][k], want[2][k]), model(srcs[k], smp, lo, hi), (lo, hi, k))


def test_stream_window_at_every_prefix_length(mod):
    nmax = PRODUCTION[-1]
    src, smp = decoy_pair(nmax, 100000, -30000, 21)
    lo, hi = -60000, 60000
    st = mod.Stream(nmax, 0)
    try:
        st.set_lag_window(lo, hi)
        st.append(src.astype(np.float64), smp.astype(np.float64))
        for n in PRODUCTION:
            ret, lag, coef = st.xcorr(n)
            want = model(src[:2 * n], smp[:n], max(lo, -n), min(hi, n - 1))
            check((lag, coef, ret), want, n)
    finally:
        st.close()


def test_argument_checks(mod):
    n = 48000
    with mod.Plan(n, 1, 0) as plan:
        plan.set_lag_window(-10, 10)
        for lo, hi in ((-n - 1, 0), (0, n), (5, 4), (-n - 5, n + 5)):
            with pytest.raises(mod.AsxError):
                plan.set_lag_window(lo, hi)
            assert plan.lag_window == (-10, 10)
    st = mod.Stream(n, 0)
    try:
        with pytest.raises(mod.AsxError):
            st.set_lag_window(3, 2)
    finally:
        st.close()


def test_driver_max_lag(mod):
    graft.build()
    sys.path.insert(0, graft.PKG_DIR)
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    import audiosync
    rng = np.random.default_rng(0)
    source = rng.uniform(-1, 1, 2 * 30 * 48000)
    sample = 0.5 * source[240000: 240000 + 30 * 48000] + 0.01 * rng.uniform(-1, 1, 30 * 48000)   # 5 s
    try:
        assert audiosync.get_max_lag() == 0
        audiosync.set_max_lag(10000)
        assert audiosync.get_max_lag() == 10000
        audiosync.set_feed(source, sample, 0)
        lag_ms, ok = audiosync.run("max lag 10 s")
        assert ok is True and lag_ms == 5000
        audiosync.set_max_lag(2000)
        audiosync.set_feed(source, sample, 0)
        lag_ms, ok = audiosync.run("max lag 2 s")
        assert ok is False or abs(lag_ms) <= 2000
    finally:
        audiosync.set_max_lag(0)
