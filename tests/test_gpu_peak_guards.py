"""The three guards that make the lag "the float64 argmax by construction" (csrc/asx_internal.h), each against float64 on the device's
own numbers (Plan.debug_peak over asx_plan_debug_peak; tests/guards_ref.py holds the references and the checks):

  bound value   |bound2 / (2 F B64) - 1| <= 2^-10: bound2 = 2 B F from float32 norm partials of the forward pass (sums of positive
                terms through a couple of hundred roundings, 1.2e-5; one lost column tile moves a norm by 3e-3)
  bound holds   max_k |r32[k] / F - r64[k]| <= bound2 / 4F, i.e. B / 2 with the device's own number, on asx_xcorr_debug_r_dev's r
  list          every lag with key64 >= M - B is listed and every listed lag has key64 >= M - 3 B (guards_ref.check_list: with
                |r32 - r64| <= B / 2 and the device listing key32 >= max32 - 2 B, key64 >= M - B gives key32 >= M - 1.5 B >=
                max32 - 2 B, and listed gives key64 >= key32 - B / 2 >= max32 - 2.5 B >= M - 3 B)
  exact values  up to 64 listed entries per pair against math.fsum of the exact float64 products (float32 inputs) or Fractions
                (double inputs): |refine_val - reference| <= 2^-52 |reference| + N 2^-100 sum |products|

Packed kernels at N = 4096 and 48 000 (peak_capacity < 2N there), real-column kernels at 144 000 with the pruned inverse pass on and
off.  Inputs are the suite's: a white pair (one candidate), two tonal pairs (hundreds of near-ties at 144 000), the Gaussian-smoothed pair
(a few).

Measured on an MI355X (worst over all cases; printed under -s), next to the limits:
  |bound2 / (2 F B64) - 1|        1.0e-7            (limit 2^-10 = 9.8e-4)
  max |r32 / F - r64| / B         0.109 tonal, 0.026 white, 0.061 smooth     (limit 0.5)
  must-list / listed lags         144 000 tone + weak noise 173 / 362, 24 000 smooth 3 / 4, 4096 tone 2 / 6, white 1 / 1
  exact values, float32 inputs    0.00 ulp: every checked value is the correctly rounded sum     (limit 1 ulp + N 2^-100 sum |p|)
  exact values, double inputs     0.33 ulp (17 listed lags at N = 6000)
"""
import functools

import numpy as np
import pytest

import guards_ref as G
import oracle
from test_gpu_exact_peak import tonal_pairs
from util import asx

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


def broad_pair():
    """test_gpu_parity.test_broad_peak_of_a_smooth_signal_is_resolved_exactly's pair (d = 7777), as float32"""
    rng = np.random.default_rng(8)
    n, sigma = 24000, 300.0
    t = np.arange(-1500, 1501)
    base = np.convolve(rng.normal(size=3 * n + 3000), np.exp(-0.5 * (t / sigma) ** 2), mode="valid")[: 3 * n]
    base /= np.abs(base).max()
    d = 7777
    return base[n: 3 * n].astype(np.float32), (0.8 * base[n + d: 2 * n + d] + 1e-4 * rng.normal(size=n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, name):
    """(source, sample, float64 keys in the plain-sum scale): computed once, shared by every test that runs the pair"""
    if name == "white":
        src, smp = oracle.synth_pair(77, 2, n, 1)[:2]
    elif name == "broad":
        src, smp = broad_pair()
    else:
        src, smp = tonal_pairs(n)[name]
    src, smp = np.ascontiguousarray(src, dtype=np.float32), np.ascontiguousarray(smp, dtype=np.float32)
    assert smp.size == n
    r = G.r64_all(src, smp)
    for a in (src, smp, r):
        a.setflags(write=False)
    return src, smp, r


@functools.lru_cache(maxsize=None)
def exact(n, name, idx):
    src, smp, _ = case(n, name)
    return G.exact_r(src, smp, idx)


def sample_entries(idx, winner, n, most=64):
    """positions in the list: always the first, the last, the smallest and the largest index, one index >= N if any is listed, and
    the winner; the rest evenly spaced"""
    pos = {0, idx.size - 1, int(np.argmin(idx)), int(np.argmax(idx)), int(np.nonzero(idx == winner)[0][0])}
    late = np.nonzero(idx >= n)[0]
    if late.size:
        pos.add(int(late[late.size // 2]))
    for p in np.linspace(0, idx.size - 1, most).astype(int):
        if len(pos) >= most:
            break
        pos.add(int(p))
    return sorted(pos)


def rule_winner(idx, val):
    """src/cross_correlation.c:52-67 on the exact values: index 0 signed, the others by fabs, the smallest index among equals"""
    key = np.where(idx == 0, val, np.abs(val))
    return int(idx[key == key.max()].min())


def check_pair(d, n, name, F, lag):
    """bound value, list, exact values of one pair's state -> (bound ratio - 1, must-list lags, listed lags, worst exact error in ulp)"""
    src, smp, r = case(n, name)
    key = G.keys64(r.copy())
    ratio = d["bound2"] / (2.0 * F * G.B64(src, smp, F)) - 1.0
    assert abs(ratio) <= G.RATIO_TOL, (n, name, d["bound2"], ratio)
    bp = d["bound2"] / (2.0 * F)
    assert d["index"] is not None
    if d["refine_n"] == 0:
        must, listed = G.check_list([d["index"]], key, bp, "%s N=%d" % (name, n))
        assert must == 1 and G.peak_of_lag(lag, n) == int(np.argmax(key)) == d["index"], (n, name, lag, d["index"])
        return ratio, must, listed, 0.0
    idx, val = d["refine_idx"], d["refine_val"]
    assert idx.size == d["refine_n"] == np.unique(idx).size
    must, listed = G.check_list(idx, key, bp, "%s N=%d" % (name, n))
    winner = rule_winner(idx, val)
    assert G.peak_of_lag(lag, n) == winner, (n, name, lag, winner)
    worst = 0.0
    for p in sample_entries(idx, winner, n):
        ref, sa = exact(n, name, int(idx[p]))
        worst = max(worst, G.check_exact(val[p], ref, sa, n))
    return ratio, must, listed, worst


CASES = [(4096, None, ("white", "tone + weak noise", "two tones")),
         (48000, None, ("white", "tone + weak noise", "two tones")),
         (24000, None, ("broad",)),
         (144000, True, ("white", "tone + weak noise", "two tones")),
         (144000, False, ("white", "tone + weak noise", "two tones"))]


@pytest.mark.parametrize("n,prune,names", CASES, ids=["%d%s" % (c[0], {None: "", True: "-prune", False: "-noprune"}[c[1]]) for c in CASES])
def test_bound_list_and_exact_values_in_a_batch(mod, n, prune, names):
    src = np.stack([case(n, k)[0] for k in names])
    smp = np.stack([case(n, k)[1] for k in names])
    with mod.Plan(n, len(names), 0) as plan:
        assert plan.layout == ("real-column" if n >= 144000 else "packed")
        if n == 48000:
            assert plan.peak_capacity < 2 * n
        if prune is not None:
            plan.set_prune(prune)
        lag, coef, ret = plan.xcorr_batch_f32(src, smp)
        assert plan.peak_overflows() == 0 and plan.group >= len(names)
        F = plan.fft_len
        states = [plan.debug_peak(i) for i in range(len(names))]
        if prune:
            assert plan.prune_stats()[0] < plan.prune_stats()[1]
    lists = 0
    for i, name in enumerate(names):
        assert int(ret[i]) == 0, (n, name)
        ratio, must, listed, worst = check_pair(states[i], n, name, F, int(lag[i]))
        print("N=%d %-18s bound2/(2 F B64) - 1 = %+.2e, must-list %d, listed %d, exact values worst %.2f ulp"
              % (n, name, ratio, must, listed, worst))
        lists += must >= 2
    # (the float64 reference's own count: at 48 000 these inputs have a single must-list lag each)
    assert lists >= 1 or n == 48000, "no pair of this batch had to have a near-tie list: nothing but the bound was checked"


@pytest.mark.parametrize("n", [4096, 48000, 24000, 144000])
def test_float32_error_stays_inside_half_the_devices_bound(mod, n):
    """bound holds: the premise of the list's sandwich, with the device's own bound2 and the r of every lag"""
    import torch
    names = ("broad",) if n == 24000 else ("white", "tone + weak noise", "two tones")
    with mod.Plan(n, 1, 0) as plan:
        F = plan.fft_len
        for name in names:
            src, smp, r = case(n, name)
            d_src, d_smp = torch.from_numpy(np.array(src)).cuda(), torch.from_numpy(np.array(smp)).cuda()
            d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
            d_lag = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
            d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
            plan.sync()
            d = plan.debug_peak(0)
            err = float(np.abs(d_r.cpu().numpy().astype(np.float64) / F - r).max())
            bp = d["bound2"] / (2.0 * F)
            print("N=%d %-18s max |r32 / F - r64| = %.3f B" % (n, name, err / bp))
            assert err <= 0.5 * bp, (n, name, err, bp)
            # the state this run left is a group's like any other: the same checks
            check_pair(d, n, name, F, int(d_lag[0]))
        assert plan.peak_overflows() == 0


def test_exact_values_of_double_inputs(mod):
    """asx_xcorr_f64 on doubles float32 cannot hold (the 8-byte route: k_refine_dots reads the doubles themselves): every listed
    value against the exact rational sum"""
    n = 6000
    s32, t32 = tonal_pairs(n)["sin(i) vs -sin(i+1)"]
    src, smp = s32.astype(np.float64) * (1.0 + 1e-9), t32.astype(np.float64) * (1.0 - 3e-10)
    key = G.keys64(G.r64_all(src, smp))
    assert int((key >= key.max() - G.B64(src, smp, 2 * n)).sum()) >= 2      # 17 lags inside B of the maximum: there has to be a list
    with mod.Plan(n, 1, 0) as plan:
        before = plan.narrowed_calls()
        ret, lag, coef = plan.xcorr_f64(src, smp)
        assert plan.narrowed_calls() == before and plan.peak_overflows() == 0 and ret == 0
        d = plan.debug_peak(0)
    idx, val = d["refine_idx"], d["refine_val"]
    assert d["refine_n"] >= 2 and idx.size == d["refine_n"]      # a tonal pair: the list is what is being checked
    winner = rule_winner(idx, val)
    assert G.peak_of_lag(lag, n) == winner
    worst = 0.0
    for p in sample_entries(idx, winner, n):
        ref, sa = G.exact_r(src, smp, int(idx[p]))
        worst = max(worst, G.check_exact(val[p], ref, sa, n))
    print("N=%d double inputs: %d listed, %d checked, worst %.2f ulp" % (n, idx.size, len(sample_entries(idx, winner, n)), worst))
