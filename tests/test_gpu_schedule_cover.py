"""The run-time-schedule kernels of csrc/xcorr_kernels.hip (k_fwd_cols<MAXR>, k_rows<MAXR>, k_inv_cols<MAXR, void, ...>) on every
feature the planner can produce (tests/schedule_cover.py: every radix of lds_fft.h in every stage role of every MAXR instance, every
stage count, block size, tile width and row form), on plans embedded in a longer transform, and at the longest lengths.

Per case of CASES: the spectrum bin by bin (tests/spectrum_check.py), which names the bin and its row when one radix in one stage
position is wrong, and a batch of three pairs against the oracle.  Run with `-m gpu -s` to see the measured z of every case."""
import numpy as np
import pytest

import oracle
import schedule_cover as sv
from device_spectrum import raw_r, run_case
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5       # the project's bound on the coefficient (tests/test_gpu_parity.py)
R_TOL = 2e-5          # test_raw_correlation_matches_oracle's bound on max |r - r64| / max |r64|


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in sv.PLAN_ENV:      # read when a plan is built
        monkeypatch.delenv(name, raising=False)


def case_id(c):
    return "x".join(str(v) for v in c[:-1])


def open_plan(mod, n, split, max_batch):
    """the plan of the forced split, on the kernels and block sizes the host-only planner announced"""
    d, k = sv.plan_of(mod, n, split)
    plan = mod.Plan(n, max_batch, 0, split=split)
    try:
        assert plan.layout == "packed" and (k["cols"], k["rows"]) == (None, None), (plan.layout, k)
        assert (plan.fft_len, plan.split, plan.threads) == (d["F"], (d["M1"], d["M2"], d["T"]), tuple(k["threads"]))
    except BaseException:
        plan.close()
        raise
    return plan, d


def batch_against_the_oracle(plan, n, seed, count=3):
    """`count` pairs of oracle.synth_pair in one host batch (odd n: pairs 1 and 2 start off a 16-byte boundary, k_fwd_cols' slow
    loads): lag and ret equal, coefficient within COEF_TOL, and no pair let off as a near-tie"""
    pairs = [oracle.synth_pair(seed, i, n, 1) for i in range(count)]
    lag, coef, ret = plan.xcorr_batch_f32(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    for i, (src, smp, _) in enumerate(pairs):
        o_ret, o_lag, o_coef, o_r, margin = oracle.cross_correlation(src, smp, want_results=True)
        assert margin >= sv.MARGIN_MIN, (n, seed, i, margin)
        assert (int(ret[i]), int(lag[i])) == (o_ret, o_lag), (n, seed, i, int(ret[i]), int(lag[i]), o_ret, o_lag)
        assert abs(float(coef[i]) - o_coef) < COEF_TOL, (n, seed, i, float(coef[i]), o_coef)


def time_domain(plan, torch, src, smp, o_r):
    """an embedded plan's r (F / 2N times the reference's) against the oracle's -> the pair's (lag, coef, ret)"""
    r, lag, coef, ret = raw_r(plan, torch, src, smp)
    err = np.abs(r / (plan.fft_len / (2.0 * smp.size)) - o_r).max() / np.abs(o_r).max()
    print("time domain N=%d F=%d split=%s: max |r - r64| / max |r64| = %.3g" % (smp.size, plan.fft_len, plan.split, err))
    assert err < R_TOL, err
    return lag, coef, ret


# ---- every feature of the run-time schedules -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sv.CASES, ids=case_id)
def test_case_spectrum_bin_by_bin(mod, torch, case):
    m1, m2, t, seed = case
    n, split = m1 * m2, sv.split_string(m1, m2, t)
    plan, d = open_plan(mod, n, split, 1)
    with plan:
        run_case(mod, torch, n, "W", split=split, want_layout="packed", plan=plan)
        if max(len(d["radix1"]), len(d["radix2"])) >= 3:
            run_case(mod, torch, n, "I", split=split, want_layout="packed", plan=plan)


@pytest.mark.parametrize("case", sv.CASES, ids=case_id)
def test_case_batch_matches_the_oracle(mod, case):
    m1, m2, t, seed = case
    plan, d = open_plan(mod, m1 * m2, sv.split_string(m1, m2, t), 3)
    with plan:
        batch_against_the_oracle(plan, m1 * m2, seed)


# ---- plans embedded in a longer transform: r is not X conj(Y), so the time domain and the batch -------------------------------------

@pytest.mark.parametrize("case", sv.EMBEDDED_CASES, ids=case_id)
def test_embedded_case_matches_the_oracle(mod, torch, case):
    n, m1, m2, t, seed = case
    plan, d = open_plan(mod, n, sv.split_string(m1, m2, t), 3)
    with plan:
        assert plan.fft_len != 2 * n
        src, smp, _ = oracle.synth_pair(seed, 0, n, 1)
        o_ret, o_lag, o_coef, o_r, margin = oracle.cross_correlation(src, smp, want_results=True)
        lag, coef, ret = time_domain(plan, torch, src, smp, o_r)
        assert (ret, lag) == (o_ret, o_lag) and abs(coef - o_coef) < COEF_TOL, (ret, lag, coef, o_ret, o_lag, o_coef)
        batch_against_the_oracle(plan, n, seed)


# ---- the longest lengths, on the planner's own plan --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(sv.LONG))
def test_long_length(mod, torch, n):
    F, split, threads = sv.LONG[n]
    seed, first = 5, 1                # pair 0 of the batch is spectrum_check.inputs("W", n)
    with mod.Plan(n, 2, 0) as plan:
        assert (plan.fft_len, plan.split, plan.threads, plan.layout) == (F, split, threads, "packed")
        src, smp, true_lag = oracle.synth_pair(seed, first, n, 1)
        o_ret, o_lag, o_coef, o_r, margin = oracle.cross_correlation(src, smp, want_results=True)
        assert margin >= sv.MARGIN_MIN and (o_ret, o_lag) == (0, true_lag)
        if F == 2 * n:
            res = run_case(mod, torch, n, "W", want_layout="packed", plan=plan)
            assert res.F == F
        else:
            time_domain(plan, torch, src, smp, o_r)
        # a device-resident batch of two
        d_src = torch.empty(2 * 2 * n, dtype=torch.float32, device="cuda")
        d_smp = torch.empty(2 * n, dtype=torch.float32, device="cuda")
        d_true = torch.empty(2, dtype=torch.int64, device="cuda")
        mod.synth_pairs_dev(seed, first, 2, n, 1, d_src.data_ptr(), d_smp.data_ptr(), d_true.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        d_lag = torch.zeros(2, dtype=torch.int64, device="cuda")
        d_coef = torch.zeros(2, dtype=torch.float64, device="cuda")
        d_ret = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), 2, d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
    assert np.array_equal(d_src[:2 * n].cpu().numpy().view(np.uint32), src.view(np.uint32))   # pair 0 is the oracle's pair
    assert int(d_true[0]) == true_lag
    assert d_lag.tolist() == d_true.tolist() and d_ret.tolist() == [0, 0], (d_lag.tolist(), d_true.tolist(), d_ret.tolist())
    assert abs(float(d_coef[0]) - o_coef) < COEF_TOL, (float(d_coef[0]), o_coef)
