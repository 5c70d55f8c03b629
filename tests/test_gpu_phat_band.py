"""Band-limited GCC-PHAT on the MI355X (asx_xcorr_phat_band_f32_dev, asx_xcorr_phat_band_debug_r_dev, Plan.xcorr_phat_band_f32) against
the float64 model of tests/phat_band_model.py: the whole curve for bands that single out a bin, a row, a mirror and a half of the row
kernels' layout; low-passed pairs, which the band is for; the full band, which is the PHAT call; broadcast, windows, a silent track,
the counters the call must leave alone, refusals.  Lengths: the smallest of each row form (480-point rows, 1200 in one piece, the
two-half form)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import phat_band_model
from util import ROOT, asx

pytestmark = pytest.mark.gpu

LENGTHS = [144000, 480000, 960000]
COEF_TOL = 1e-5
# max |d_r / V - model| over all 2N lags, every band of test_curve, pairs 0 and 1, against the float64 model.  Measured on an MI355X,
# the larger of the two pairs, at N = 144 000 / 480 000 / 960 000:
#   [0, 0] 1.1e-16 / 1.1e-16 / 6.0e-8     [1, 1] 7.0e-7 / 4.5e-7 / 5.5e-7     [N, N] 6.0e-8 / 0 / 0     [M1, M1] 3.7e-7 / 3.7e-7 / 4.2e-7
#   [2 M1 - 1, 2 M1 + 1] 3.7e-7 / 4.5e-7 / 3.5e-7     [N - 1, N] 3.5e-7 / 3.9e-7 / 5.9e-7     [12345, N/3 + 7] 3.0e-8 / 6.7e-8 / 4.9e-8
#   [0, N - 1] 1.3e-8 / 2.0e-8 / 3.2e-8     [1, N] 1.3e-8 / 2.0e-8 / 3.2e-8
# The bands of a few bins are the worst: with V = 2 or 3 the curve is a cosine of magnitude near 1 at EVERY lag, so every lag carries
# the float32 error of a value near 1 (the twiddles of three passes), where a wide band's curve is near zero but at its peak.  Asserted
# at four times the measured maximum, 7.0e-7 -> 2.8e-6, rounded up to one significant digit; the hard cap is 1e-5.  An error of the
# layout (a wrong digit, a missed mirror, the wrong half) is of order 1 in these bands.  The peak heights of the low-passed pairs came
# out at most 1.0e-7 from the model's.
CURVE_TOL = 3e-6
assert CURVE_TOL <= 1e-5
SEED = 77
SHIFTS = (3, 0, 3, 0, 3)

_pairs, _units, _low = {}, {}, {}


def pair(n, k):
    """pair k of the generator at length n, noise shift 3 or 0 by k: (source, sample, planted lag); computed once"""
    if (n, k) not in _pairs:
        _pairs[n, k] = oracle.synth_pair(SEED, k, n, SHIFTS[k % len(SHIFTS)])
    return _pairs[n, k]


def curve(n, k, lo, hi):
    """the float64 banded r_phat / V of pair(n, k): the whitened spectrum is computed once per pair, the band costs one inverse"""
    if (n, k) not in _units:
        s, t, _ = pair(n, k)
        q = np.fft.rfft(s.astype(np.float64)) * np.conj(np.fft.rfft(t.astype(np.float64), 2 * n))
        mag = np.abs(q)
        unit = np.divide(q, mag, out=np.zeros_like(q), where=mag > 0)
        unit.setflags(write=False)
        _units[n, k] = unit
    unit = _units[n, k].copy()
    unit[:lo] = 0.0
    unit[hi + 1:] = 0.0
    return np.fft.irfft(unit, 2 * n) * (2.0 * n / phat_band_model.votes(n, lo, hi))


def lowpass(n, p):
    """phat_band_model.lowpass_pair(p, n) and its model under the band [1, n/6]: ((source, sample, planted), (ret, lag, coef, peak),
    how far the model's peak stands above every other lag); computed once"""
    if (n, p) not in _low:
        src, smp, planted = phat_band_model.lowpass_pair(p, n)
        r = phat_band_model.r_phat_band(src, smp, 1, n // 6)
        m = phat_band_model.model(src, smp, 1, n // 6, r=r)
        rest = np.abs(r)
        rest[m[1] % (2 * n)] = 0.0
        _low[n, p] = (src, smp, planted), m, m[3] - float(rest.max())
    return _low[n, p]


def stacked(n, ks):
    return np.stack([pair(n, k)[0] for k in ks]), np.stack([pair(n, k)[1] for k in ks])


def bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


def all_bits(out):
    return [np.asarray(a).tobytes() for a in out]


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


def outputs(torch, b):
    return (torch.full((b,), -99, dtype=torch.int64, device="cuda"), torch.full((b,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((b,), 7.0, dtype=torch.float64, device="cuda"), torch.full((b,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    b = out[0].numel()
    return [a.cpu().tolist() for a in out] == [[-99] * b, [7.0] * b, [7.0] * b, [7] * b]


@pytest.mark.parametrize("n", LENGTHS)
def test_curve(mod, torch, n):
    """the debug call, band by band: r_phat of all 2N lags against the float64 model.  A wrong digit order, a missed mirror or a wrong
    half is an error of order 1 here.  Bin 0, bin 1, bin N; a whole row's first bins (M1: row M1; 2 M1 +- 1: rows 2 M1 - 1 -> the
    mirror of row 1, 0, 1 with k2 = 1); the top two; a band with both ends inside rows; all but bin N; all but bin 0."""
    worst = {}
    with mod.Plan(n, 1, 0) as plan:
        m1 = plan.split[0]
        assert plan.layout == "real-column" and n % m1 == 0
        bands = [(0, 0), (1, 1), (n, n), (m1, m1), (2 * m1 - 1, 2 * m1 + 1), (n - 1, n), (12345, n // 3 + 7), (0, n - 1), (1, n)]
        for k in (0, 1):
            src, smp, planted = pair(n, k)
            d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
            for lo, hi in bands:
                v = phat_band_model.votes(n, lo, hi)
                d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
                out = outputs(torch, 1)
                torch.cuda.synchronize()
                plan.phat_band_debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), lo, hi, d_r.data_ptr(), *(a.data_ptr() for a in out))
                plan.sync()
                r32 = d_r.cpu().numpy()
                want = curve(n, k, lo, hi)
                err = float(np.max(np.abs(r32.astype(np.float64) / v - want)))
                worst[lo, hi] = max(worst.get((lo, hi), 0.0), err)
                lag, coef, peak, ret = (a.cpu().numpy()[0] for a in out)
                idx = int(lag) % (2 * n)
                print("phat band curve n", n, "pair", k, "band", (lo, hi), "V", v, "max |d_r / V - model|", err, "lag", int(lag),
                      "peak", float(peak), "model there", abs(float(want[idx])))
                assert float(peak) == abs(float(r32[idx])) / v, (n, k, lo, hi, peak, r32[idx])
                assert int(ret) == 0
                if hi - lo > 1000:
                    # a wide band: one lag stands out, the float32 argmax of the curve the call itself returns, and it is the model's
                    assert np.max(np.abs(r32)) == abs(r32[idx]) and int(np.argmax(np.abs(r32))) == idx, (n, k, lo, hi)
                    m = phat_band_model.model(src, smp, lo, hi, r=want)
                    assert int(lag) == m[1] == planted, (n, k, lo, hi, lag, m)
                    assert abs(float(coef) - m[2]) < COEF_TOL
                assert err <= CURVE_TOL, (n, k, lo, hi, err)
    print("phat band curve n", n, "worst", max(worst.values()), worst)


@pytest.mark.parametrize("n", LENGTHS)
def test_low_passed_pairs(mod, n):
    """five pairs low-passed at bin N/6 over noise of 1e-4, a plan of max_batch 2 (three launch groups), bins [1, N/6] voting: the
    planted lag, more than four times the peak height of the call in which every bin votes.  The model's peak stands at least 0.0068
    above every other lag at all three lengths (pairs 0..4: 0.0103 0.0068 0.0250 0.0171 0.0256 at N = 144 000, 0.0208 0.0107 0.0151
    0.0222 0.0231 at 480 000, 0.0257 0.0138 0.0091 0.0134 0.0258 at 960 000), hundreds of times the tolerance: no pair was swapped."""
    lows = [lowpass(n, p) for p in range(5)]
    src, smp = np.stack([l[0][0] for l in lows]), np.stack([l[0][1] for l in lows])
    for p, (_, m, above) in enumerate(lows):
        print("phat band low-passed n", n, "pair", p, "model", m, "above the rest", above)
        assert above > 500 * CURVE_TOL, (n, p, above)
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        plan.set_pearson(False)
        got = plan.xcorr_phat_band_f32(src, smp, 1, n // 6)
        full = plan.xcorr_phat_f32(src, smp)
        for p, ((_, _, planted), m, _) in enumerate(lows):
            lag, coef, peak, ret = (a[p] for a in got)
            print("phat band low-passed n", n, "pair", p, "lag", int(lag), "planted", planted, "peak", float(peak), "model", m[3],
                  "diff", abs(float(peak) - m[3]), "every bin voting", float(full[2][p]), int(full[0][p]))
            assert (int(ret), int(lag)) == (0, planted) and m[1] == planted, (n, p, lag, planted, m)
            assert abs(float(peak) - m[3]) <= CURVE_TOL, (n, p, peak, m)
            assert abs(float(coef) - m[2]) < COEF_TOL, (n, p, coef, m)
            assert float(peak) > 4.0 * float(full[2][p]), (n, p, peak, full[2][p])
        rows = np.stack([got[0], got[0]], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(src, smp, rows)
        assert lag.tolist() == got[0].tolist() and ret.tolist() == got[3].tolist()
        assert coef.tobytes() == got[1].tobytes(), (coef, got[1])
        plan.set_pearson(True)  # the coefficient is the direct form's whatever the plan's setting
        assert all_bits(plan.xcorr_phat_band_f32(src, smp, 1, n // 6)) == all_bits(got)


@pytest.mark.parametrize("n", LENGTHS)
def test_the_full_band_is_the_phat_call(mod, n):
    src, smp = stacked(n, range(3))
    rows = np.array([(-n, n - 1), (-n // 3, -5), (7, 6)], dtype=np.int64)
    with mod.Plan(n, 2, 0) as plan:
        assert all_bits(plan.xcorr_phat_band_f32(src, smp, 0, n)) == all_bits(plan.xcorr_phat_f32(src, smp))
        assert all_bits(plan.xcorr_phat_band_f32(src[0], smp, 0, n, rows)) == all_bits(plan.xcorr_phat_f32(src[0], smp, rows))


def test_broadcast_and_strides(mod, torch):
    """stride 0 for either operand and an overlapping hop: the bits of the call on materialised contiguous pairs"""
    n = 144000
    band = (300, n // 4)
    src, smp = stacked(n, range(3))
    with mod.Plan(n, 2, 0) as plan:
        want = plan.xcorr_phat_band_f32(np.broadcast_to(src[0], (3, 2 * n)), smp, *band)
        assert all_bits(plan.xcorr_phat_band_f32(src[0], smp, *band)) == all_bits(want)          # source stride 0
        assert int(want[0][0]) == pair(n, 0)[2]
        want = plan.xcorr_phat_band_f32(src, np.broadcast_to(smp[1], (3, n)), *band)
        assert all_bits(plan.xcorr_phat_band_f32(src, smp[1], *band)) == all_bits(want)          # sample stride 0
        assert int(want[0][1]) == pair(n, 1)[2]
        want = plan.xcorr_phat_band_f32(np.broadcast_to(src[2], (3, 2 * n)), np.broadcast_to(smp[2], (3, n)), *band)
        assert all_bits(plan.xcorr_phat_band_f32(src[2], smp[2], *band, windows=np.tile(np.array([-n, n - 1]), (3, 1)))) == all_bits(want)  # both
        hop = 1000
        rec = np.concatenate([src[2], src[0][:2 * hop]])
        wins = np.stack([rec[k * hop:k * hop + 2 * n] for k in range(3)])
        want = plan.xcorr_phat_band_f32(wins, np.broadcast_to(smp[2], (3, n)), *band)
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(smp[2].copy()).cuda()
        out = outputs(torch, 3)
        torch.cuda.synchronize()
        plan.xcorr_phat_band_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, 0, 0, 3, *band, *(a.data_ptr() for a in out))
        plan.sync()
        assert [a.cpu().numpy().tobytes() for a in out] == all_bits(want)
        assert want[0].tolist() == [pair(n, 2)[2] - k * hop for k in range(3)], want[0]


def test_windows(mod):
    """per-pair rows that leave the planted lag out; a full row; a row that is not a window; the plan's window"""
    n = 144000
    band = (300, n // 4)
    src, smp = stacked(n, range(5))
    planted = [pair(n, k)[2] for k in range(5)]
    with mod.Plan(n, 2, 0) as plan:
        free = plan.xcorr_phat_band_f32(src, smp, *band)
        assert free[0].tolist() == planted
        rows = []
        for k, l in enumerate(planted):                               # a row on the other side of lag 0 from the planted lag,
            rows.append((-n // 3 - k, -5) if l >= 0 else (7, n // 3 + k))  # so every row leaves it out
        rows[2] = (-n, n - 1)                                         # full: the no-window bits
        rows[3] = (5, 4)                                              # not a window
        rows = np.array(rows, dtype=np.int64)
        got = plan.xcorr_phat_band_f32(src, smp, *band, windows=rows)
        models = {}
        for k in (0, 1, 4):
            lo, hi = (int(v) for v in rows[k])
            m = models[k] = phat_band_model.model(*pair(n, k)[:2], *band, lo, hi, r=curve(n, k, *band))
            assert not lo <= planted[k] <= hi and m[1] != planted[k]
            assert (int(got[3][k]), int(got[0][k])) == (m[0], m[1]), (k, got, m)
            assert abs(float(got[1][k]) - m[2]) < COEF_TOL and abs(float(got[2][k]) - m[3]) <= CURVE_TOL, (k, got, m)
        assert bits(got, 2) == bits(free, 2)
        assert (int(got[0][3]), int(got[3][3])) == (0, -2) and np.isnan(got[1][3]) and np.isnan(got[2][3]), got
        valid = np.array([tuple(r) if k != 3 else (-n, n - 1) for k, r in enumerate(rows)], dtype=np.int64)
        ref = plan.xcorr_phat_band_f32(src, smp, *band, windows=valid)
        for k in (0, 1, 2, 4):
            assert bits(got, k) == bits(ref, k), k
        # the plan's window, d_windows == NULL: pair 0's row for every pair
        lo, hi = (int(v) for v in rows[0])
        plan.set_lag_window(lo, hi)
        win = plan.xcorr_phat_band_f32(src, smp, *band)
        assert plan.lag_window == (lo, hi)
        assert bits(win, 0) == bits(got, 0)
        for k in range(5):
            m = phat_band_model.model(*pair(n, k)[:2], *band, lo, hi, r=curve(n, k, *band))
            assert (int(win[3][k]), int(win[0][k])) == (m[0], m[1]) and abs(float(win[2][k]) - m[3]) <= CURVE_TOL, (k, win, m)
        # rows replace the plan's window and leave it alone
        full = plan.xcorr_phat_band_f32(src, smp, *band, windows=np.array([-n, n - 1], dtype=np.int64))
        assert all_bits(full) == all_bits(free) and plan.lag_window == (lo, hi)


def test_silent_pair_counters_and_a_plain_call_after(mod, torch):
    n = 144000
    band = (300, n // 4)
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
            base = plan.xcorr_phat_band_f32(src, smp, *band)
            got = plan.xcorr_phat_band_f32(src, quiet, *band)
            assert (int(got[0][1]), float(got[2][1]), int(got[3][1])) == (0, 0.0, -1) and np.isnan(got[1][1]), got
            for k in (0, 2, 3, 4):
                assert bits(got, k) == bits(base, k), k
            plan.set_lag_window(100, 5000)                            # the seed of a window that does not hold lag 0
            got = plan.xcorr_phat_band_f32(src, quiet, *band)
            assert (int(got[0][1]), float(got[2][1]), int(got[3][1])) == (100, 0.0, -1), got
            plan.set_lag_window(-n, n - 1)
            plan.xcorr_phat_band_f32(src[0], smp, *band)
            plan.xcorr_phat_band_f32(src, smp, 0, n)
            plan.xcorr_phat_band_f32(src, smp, *band, windows=np.array([(-9, 9), (3, 2), (-n, n - 1), (0, 0), (-n, -n)], dtype=np.int64))
        plan.set_exact(True)
        assert counters(plan) == before
        assert plain(plan) == want_plain


def test_refusals(mod, torch):
    n = 144000
    src, smp = stacked(n, range(2))
    d_src = torch.from_numpy(np.concatenate([src.ravel(), src[0][:8]])).cuda()
    d_smp = torch.from_numpy(smp).cuda()
    with mod.Plan(n, 2, 0) as plan:
        good = (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n)
        for lo, hi in [(5, 4), (-1, 10), (0, n + 1), (n, n + 1), (n + 1, n + 1), (-3, -2), (2 ** 40, 2 ** 41), (-2 ** 62, 2 ** 62)]:
            out = outputs(torch, 2)
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match="not a band"):
                plan.xcorr_phat_band_dev(*good, 0, 0, 2, lo, hi, *(a.data_ptr() for a in out))
            assert untouched(torch, out), (lo, hi)
            d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
            with pytest.raises(mod.AsxError, match="not a band"):
                plan.phat_band_debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), lo, hi, d_r.data_ptr(), *(a.data_ptr() for a in out))
            assert untouched(torch, out) and not bool(d_r.any()), (lo, hi)
        # every refusal of the PHAT call
        cases = [("null", good, 1), ("aligned", (d_src.data_ptr() + 4, 2 * n, d_smp.data_ptr(), n), None),
                 ("multiples of 4", (d_src.data_ptr(), 6, d_smp.data_ptr(), n), None)]
        for text, args, drop in cases:
            out = outputs(torch, 2)
            ptrs = [a.data_ptr() for a in out]
            if drop is not None:
                ptrs[drop] = 0                                        # a NULL d_coef
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_phat_band_dev(*args, 0, 0, 2, 100, 1000, *ptrs)
            assert untouched(torch, out), text
        assert mod.lib().asx_xcorr_phat_band_f32_dev(plan._h, d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, None, 0, 0, 100, 1000, None,
                                                     outputs(torch, 2)[1].data_ptr(), None, outputs(torch, 2)[3].data_ptr(), None) == 0  # batch == 0
        out = outputs(torch, 2)
        d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        with pytest.raises(mod.AsxError, match="null"):
            plan.phat_band_debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), 100, 1000, d_r.data_ptr(), out[0].data_ptr(), 0,
                                       out[2].data_ptr(), out[3].data_ptr())
        assert untouched(torch, out)
    m = 1000  # a length outside the tuned table: a packed plan
    d_s, d_t = torch.zeros(4 * m, dtype=torch.float32, device="cuda"), torch.zeros(2 * m, dtype=torch.float32, device="cuda")
    with mod.Plan(m, 2, 0) as plan:
        assert plan.layout == "packed"
        for lo, hi in [(10, 100), (0, m)]:
            out = outputs(torch, 2)
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match="real-column"):
                plan.xcorr_phat_band_dev(d_s.data_ptr(), 2 * m, d_t.data_ptr(), m, 0, 0, 2, lo, hi, *(a.data_ptr() for a in out))
            assert untouched(torch, out)
            d_r = torch.zeros(2 * m, dtype=torch.float32, device="cuda")
            with pytest.raises(mod.AsxError, match="real-column"):
                plan.phat_band_debug_r_dev(d_s.data_ptr(), d_t.data_ptr(), lo, hi, d_r.data_ptr(), *(a.data_ptr() for a in out))
            assert untouched(torch, out)


PACKED_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as graft
mod = graft.load()
n = 144000
with mod.Plan(n, 1, 0) as plan:
    assert plan.layout == "packed", plan.layout
    for lo, hi in ((1, n // 6), (0, n)):
        try:
            plan.xcorr_phat_band_f32(np.ones(2 * n, dtype=np.float32), np.ones(n, dtype=np.float32), lo, hi)
        except mod.AsxError as e:
            assert "real-column" in str(e), e
            print("refused", lo, hi)
"""


def test_a_production_length_forced_to_a_packed_plan_is_refused(mod):
    """ASX_LAYOUT=packed is read when a plan is made; a fresh process, so that nothing of this one's state is involved"""
    env = dict(os.environ, ASX_LAYOUT="packed")
    done = subprocess.run([sys.executable, "-c", PACKED_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split("\n")[:2] == ["refused 1 24000", "refused 0 144000"], (done.stdout, done.stderr)
