"""GCC-PHAT on the MI355X (asx_xcorr_phat_f32_dev, asx_xcorr_phat_debug_r_dev, Plan.xcorr_phat_f32) against the float64 model of
tests/phat_model.py: the lag is the model's, the coefficient the direct form's at that lag, the peak height and the whole curve
within the measured float32 error; scaling, broadcast, windows, silent pairs, the counters the call must leave alone, refusals."""
import numpy as np
import pytest

import oracle
import phat_model
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
# max |d_r / F - model| over all 2N lags (test_curve).  Measured on an MI355X over that test's four pairs: 2.2e-8 at N = 144 000 (pairs
# 0 and 1: 2.17e-8, 4.7e-9), 3.2e-8 at N = 960 000 (3.20e-8, 8.9e-9) -- in every pair the largest error sits at the peak itself, half
# a float32 ulp of a value near 0.5.  Asserted at four times the measured maximum, 1.3e-7, rounded up to one significant digit (the
# spread between boxes and pairs: the peak heights of the other tests' pairs came out up to 6.5e-8 from the model's); the hard cap
# is 1e-5.  The model's peak stands at least 0.06 above every other lag on these inputs, so neither can hide a wrong lag.
CURVE_TOL = 2e-7
assert CURVE_TOL <= 1e-5
SEED = 77
SHIFTS = (3, 0, 3, 0, 3)

_pairs, _models = {}, {}


def pair(n, k):
    """pair k of the generator at length n, noise shift 3 or 0 by k: (source, sample, planted lag); computed once"""
    if (n, k) not in _pairs:
        _pairs[n, k] = oracle.synth_pair(SEED, k, n, SHIFTS[k % len(SHIFTS)])
    return _pairs[n, k]


def curve(n, k):
    """the float64 r_phat / F of pair(n, k); computed once and never written to"""
    if (n, k) not in _models:
        r = phat_model.r_phat(*pair(n, k)[:2])
        r.setflags(write=False)
        _models[n, k] = r
    return _models[n, k]


def stacked(n, ks):
    return np.stack([pair(n, k)[0] for k in ks]), np.stack([pair(n, k)[1] for k in ks])


def bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


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


def check_pair(got, k, n, what, model=None):
    lag, coef, peak, ret = (a[k] for a in got)
    src, smp, _ = pair(n, what[-1]) if model is None else (None, None, None)
    m = model if model is not None else phat_model.model(src, smp, r=curve(n, what[-1]))
    print("phat", what, "lag", int(lag), "model", m[1], "peak", float(peak), "model", m[3], "diff", abs(float(peak) - m[3]))
    assert (int(ret), int(lag)) == (m[0], m[1]), (what, lag, coef, peak, ret, m)
    assert abs(float(coef) - m[2]) < COEF_TOL, (what, coef, m)
    assert abs(float(peak) - m[3]) <= CURVE_TOL, (what, peak, m)


@pytest.mark.parametrize("n", [144000, 480000, 960000])
def test_parity_over_several_launch_groups(mod, n):
    """480-point rows, 1200-point rows, the two-half form; max_batch 2 and five pairs: three launch groups"""
    src, smp = stacked(n, range(5))
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        plan.set_pearson(False)
        got = plan.xcorr_phat_f32(src, smp)
        for k in range(5):
            check_pair(got, k, n, (n, k))
            assert int(got[0][k]) == pair(n, k)[2]
        rows = np.stack([got[0], got[0]], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, rows)
        assert lag.tolist() == got[0].tolist() and ret.tolist() == got[3].tolist()
        assert coef.tobytes() == got[1].tobytes(), (coef, got[1])
        plan.set_pearson(True)  # the coefficient is the direct form's whatever the plan's setting
        again = plan.xcorr_phat_f32(src, smp)
        assert [a.tobytes() for a in again] == [a.tobytes() for a in got]


def test_parity_600_row_columns(mod):
    n = 1440000
    src, smp, planted = pair(n, 0)
    with mod.Plan(n, 1, 0) as plan:
        got = plan.xcorr_phat_f32(src, smp)
    check_pair(got, 0, n, (n, 0))
    assert int(got[0][0]) == planted


@pytest.mark.parametrize("n", [144000, 960000])
def test_curve(mod, torch, n):
    """the debug call: r_phat of all 2N lags against the float64 model"""
    worst = 0.0
    with mod.Plan(n, 1, 0) as plan:
        for k in (0, 1):
            src, smp, _ = pair(n, k)
            d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
            d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
            d_lag = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
            d_peak = torch.zeros(1, dtype=torch.float64, device="cuda")
            d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            plan.phat_debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(),
                                  d_peak.data_ptr(), d_ret.data_ptr())
            plan.sync()
            r = d_r.cpu().numpy().astype(np.float64) / (2.0 * n)
            err = float(np.max(np.abs(r - curve(n, k))))
            worst = max(worst, err)
            print("phat curve n", n, "pair", k, "max |d_r / F - model|", err)
            got = tuple(a.cpu().numpy() for a in (d_lag, d_coef, d_peak, d_ret))
            check_pair(got, 0, n, (n, k))
            # the peak is the float32 argmax of the curve the call itself returns
            idx = int(got[0][0]) % (2 * n)
            assert float(got[2][0]) == abs(float(d_r[idx].item())) / (2.0 * n)
            assert np.max(np.abs(r)) == abs(r[idx])
            assert err <= CURVE_TOL, (n, k, err)
    print("phat curve n", n, "worst", worst)


def test_hum(mod):
    """a 50 Hz tone in both tracks: the raw correlation's peak leaves the planted lag, the PHAT peak stays"""
    n = phat_model.HUM_N
    pairs = [phat_model.hum_pair(p) for p in range(3)]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 3, 0) as plan:
        plain = plan.xcorr_broadcast_f32(src, smp)
        got = plan.xcorr_phat_f32(src, smp)
    for p in range(3):
        assert int(plain[0][p]) != pairs[p][2], (p, plain[0], pairs[p][2])
        assert int(got[0][p]) == pairs[p][2] and int(got[3][p]) == 0, (p, got, pairs[p][2])
        assert float(got[2][p]) > 0.2, got


def test_range_and_sign(mod):
    """both tracks times 2^40 and 2^-40 (exact in float32): |Q|^2 leaves the float32 range, |Q| does not; a negated sample"""
    n = 144000
    src, smp = stacked(n, range(5))
    with mod.Plan(n, 2, 0) as plan:
        base = plan.xcorr_phat_f32(src, smp)
        for e in (40, -40):
            s = np.float32(2.0 ** e)
            assert np.all(np.isfinite(src * s)) and np.all((src * s != 0) == (src != 0))
            got = plan.xcorr_phat_f32(src * s, smp * s)
            assert got[0].tolist() == base[0].tolist() and got[3].tolist() == [0] * 5, (e, got)
            for k in range(5):
                m = phat_model.model(*pair(n, k)[:2], r=curve(n, k))
                print("phat scaled 2^%d" % e, k, "peak", float(got[2][k]), "model", m[3], "diff", abs(float(got[2][k]) - m[3]))
                assert abs(float(got[2][k]) - m[3]) <= CURVE_TOL, (e, k, got[2][k], m)
                assert abs(float(got[1][k]) - m[2]) < COEF_TOL, (e, k, got[1][k], m)
        neg = plan.xcorr_phat_f32(src, -smp)
        assert neg[0].tolist() == base[0].tolist() and neg[3].tolist() == [0] * 5, neg
        for k in range(5):
            assert float(neg[1][k]) < 0 < float(base[1][k]) and abs(float(neg[1][k]) + float(base[1][k])) < COEF_TOL
            assert abs(float(neg[2][k]) - float(base[2][k])) <= CURVE_TOL


def test_broadcast_and_strides(mod, torch):
    """stride 0 for either operand and an overlapping hop: the bits of the call on materialised contiguous pairs"""
    n = 144000
    src, smp = stacked(n, range(3))
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_phat_f32(np.broadcast_to(src[0], (3, 2 * n)), smp)
        got = plan.xcorr_phat_f32(src[0], smp)                       # source stride 0
        assert [a.tobytes() for a in got] == [a.tobytes() for a in want]
        want = plan.xcorr_phat_f32(src, np.broadcast_to(smp[1], (3, n)))
        got = plan.xcorr_phat_f32(src, smp[1])                       # sample stride 0
        assert [a.tobytes() for a in got] == [a.tobytes() for a in want]
        assert int(got[0][1]) == pair(n, 1)[2]
        hop = 1000
        rec = np.concatenate([src[2], src[0][:2 * hop]])
        wins = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        want = plan.xcorr_phat_f32(wins, np.broadcast_to(smp[2], (3, n)))
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(smp[2].copy()).cuda()
        out = (torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda"),
               torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_phat_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, 0, 0, 3, *(a.data_ptr() for a in out))
        plan.sync()
        assert [a.cpu().numpy().tobytes() for a in out] == [a.tobytes() for a in want]
        assert want[0].tolist() == [pair(n, 2)[2] - k * hop for k in range(3)], want[0]


def test_windows(mod):
    """the plan's window and per-pair rows that leave the planted lag out; a full row; a row that is not a window"""
    n = 144000
    src, smp = stacked(n, range(5))
    planted = [pair(n, k)[2] for k in range(5)]
    with mod.Plan(n, 2, 0) as plan:
        free = plan.xcorr_phat_f32(src, smp)
        rows = []
        for k, l in enumerate(planted):                               # a row on the other side of lag 0 from the planted lag,
            rows.append((-n // 3 - k, -5) if l >= 0 else (7, n // 3 + k))  # so every row leaves it out
        rows[2] = (-n, n - 1)                                         # full: the no-window bits
        rows[3] = (5, 4)                                              # not a window
        rows = np.array(rows, dtype=np.int64)
        got = plan.xcorr_phat_f32(src, smp, rows)
        for k in (0, 1, 4):
            lo, hi = (int(v) for v in rows[k])
            m = phat_model.model(*pair(n, k)[:2], lo, hi, r=curve(n, k))
            assert not lo <= planted[k] <= hi and m[1] != planted[k]
            check_pair(got, k, n, ("rows", k), model=m)
        assert bits(got, 2) == bits(free, 2)
        assert (int(got[0][3]), int(got[3][3])) == (0, -2) and np.isnan(got[1][3]) and np.isnan(got[2][3]), got
        valid = np.array([tuple(r) if k != 3 else (-n, n - 1) for k, r in enumerate(rows)], dtype=np.int64)
        ref = plan.xcorr_phat_f32(src, smp, valid)
        for k in (0, 1, 2, 4):
            assert bits(got, k) == bits(ref, k), k
        # the plan's window, d_windows == NULL: pair 0's row for every pair
        lo, hi = (int(v) for v in rows[0])
        plan.set_lag_window(lo, hi)
        win = plan.xcorr_phat_f32(src, smp)
        assert plan.lag_window == (lo, hi)
        for k in range(5):
            check_pair(win, k, n, ("window", k), model=phat_model.model(*pair(n, k)[:2], lo, hi, r=curve(n, k)))
        assert bits(win, 0) == bits(got, 0)
        # rows replace the plan's window and leave it alone
        full = plan.xcorr_phat_f32(src, smp, np.array([-n, n - 1], dtype=np.int64))
        assert [a.tobytes() for a in full] == [a.tobytes() for a in free] and plan.lag_window == (lo, hi)


def test_silent_pair_counters_and_a_plain_call_after(mod, torch):
    n = 144000
    src, smp = stacked(n, range(5))
    quiet = smp.copy()
    quiet[1] = 0.0
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()

    def plain(plan):
        out = (torch.zeros(5, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"),
               torch.zeros(5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), 5, *(a.data_ptr() for a in out))
        plan.sync()
        return [a.cpu().numpy().tobytes() for a in out]

    def counters(plan):
        return plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats()

    with mod.Plan(n, 2, 0) as fresh:
        want_plain = plain(fresh)
    with mod.Plan(n, 2, 0) as plan:
        plain(plan)                                                   # the counters hold something to begin with
        before = counters(plan)
        assert before[2] != (0, 0, 0) and before[3][1] > 0, before
        for exact in (True, False):
            plan.set_exact(exact)
            base = plan.xcorr_phat_f32(src, smp)
            got = plan.xcorr_phat_f32(src, quiet)
            assert (int(got[0][1]), float(got[2][1]), int(got[3][1])) == (0, 0.0, -1) and np.isnan(got[1][1]), got
            for k in (0, 2, 3, 4):
                assert bits(got, k) == bits(base, k), k
            plan.set_lag_window(100, 5000)                            # the seed of a window that does not hold lag 0
            got = plan.xcorr_phat_f32(src, quiet)
            assert (int(got[0][1]), float(got[2][1]), int(got[3][1])) == (100, 0.0, -1), got
            plan.set_lag_window(-n, n - 1)
            plan.xcorr_phat_f32(src[0], smp)
            plan.xcorr_phat_f32(src, smp, np.array([(-9, 9), (3, 2), (-n, n - 1), (0, 0), (-n, -n)], dtype=np.int64))
        plan.set_exact(True)
        assert counters(plan) == before
        assert plain(plan) == want_plain


def test_refusals(mod, torch):
    n = 144000
    src, smp = stacked(n, range(2))
    d_src = torch.from_numpy(np.concatenate([src.ravel(), src[0][:8]])).cuda()
    d_smp = torch.from_numpy(smp).cuda()

    def outputs():
        return (torch.full((2,), -99, dtype=torch.int64, device="cuda"), torch.full((2,), 7.0, dtype=torch.float64, device="cuda"),
                torch.full((2,), 7.0, dtype=torch.float64, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda"))

    def untouched(out):
        torch.cuda.synchronize()
        return [a.cpu().tolist() for a in out] == [[-99, -99], [7.0, 7.0], [7.0, 7.0], [7, 7]]

    with mod.Plan(n, 2, 0) as plan:
        cases = [("null", (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n), 1),
                 ("aligned", (d_src.data_ptr() + 4, 2 * n, d_smp.data_ptr(), n), None),
                 ("multiples of 4", (d_src.data_ptr(), 6, d_smp.data_ptr(), n), None)]
        for text, (ps, ss, pm, ms), drop in cases:
            out = outputs()
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0                                        # a NULL d_coef
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_phat_dev(ps, ss, pm, ms, 0, 0, 2, *ptrs)
            assert untouched(out), text
        assert mod.lib().asx_xcorr_phat_f32_dev(plan._h, d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, None, 0, 0, None,
                                                outputs()[1].data_ptr(), None, outputs()[3].data_ptr(), None) == 0  # batch == 0
        out = outputs()
        d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        with pytest.raises(mod.AsxError, match="null"):
            plan.phat_debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), out[0].data_ptr(), 0, out[2].data_ptr(),
                                  out[3].data_ptr())
        assert untouched(out)
    m = 1000
    d_s, d_t = torch.zeros(4 * m, dtype=torch.float32, device="cuda"), torch.zeros(2 * m, dtype=torch.float32, device="cuda")
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        out = outputs()
        torch.cuda.synchronize()
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.xcorr_phat_dev(d_s.data_ptr(), 2 * m, d_t.data_ptr(), m, 0, 0, 2, *(a.data_ptr() for a in out))
        assert untouched(out)
        d_r = torch.zeros(2 * m, dtype=torch.float32, device="cuda")
        with pytest.raises(mod.AsxError, match="real-column"):
            plan.phat_debug_r_dev(d_s.data_ptr(), d_t.data_ptr(), d_r.data_ptr(), *(a.data_ptr() for a in out))
        assert untouched(out)
