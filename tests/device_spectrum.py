"""One pair through asx_xcorr_debug_r_dev and its r held bin by bin against the float64 reference (tests/spectrum_check.py):
what test_gpu_transform_spectrum.py and test_gpu_schedule_cover.py share (test helper, not a conftest).  Needs a GPU and torch."""
import numpy as np

import spectrum_check as sc


def raw_r(plan, torch, x, y):
    """r[0 .. 2N) of one pair as debug_r_dev leaves it (unnormalised: F times the plain sum of products) with the pair's result
    -> (r float64[2N], lag, coef, ret)"""
    n = y.size
    d_src = torch.from_numpy(x).cuda()
    d_smp = torch.from_numpy(y).cuda()
    d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_lag = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
    d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
    plan.sync()
    return d_r.cpu().numpy().astype(np.float64), int(d_lag[0]), float(d_coef[0]), int(d_ret[0])


def plain_r(plan, torch, x, y):
    """the plain sum of products r[p] = sum_j x[(j + p) mod F] y[j] as the device computes it (a plan that is not embedded)
    -> (r float64[F], plan.layout, plan.split)"""
    assert plan.fft_len == 2 * y.size
    return raw_r(plan, torch, x, y)[0] / (2 * y.size), plan.layout, plan.split


def device_r(mod, torch, x, y, split=None):
    with mod.Plan(y.size, 1, 0, split=split) as plan:
        return plain_r(plan, torch, x, y)


def impulse_edges(d):
    """a = 2N - 1 and b = M2 - 1: the last sample of the last matrix row against the last column of row 0"""
    return 2 * (d["M1"] * d["M2"]) - 1, d["M2"] - 1


def run_case(mod, torch, n, kind, split=None, want_layout=None, plan=None):
    """input family `kind` (spectrum_check.inputs) of length n through the plan of `split` (or the open `plan` of that split):
    prints the summary, asserts zmax < Z_MAX -> the spectrum_check.Result"""
    d = mod.planmath_describe(n, split)
    a, b = impulse_edges(d)
    x, y = sc.inputs(kind, n, a=a, b=b)
    r, layout, spl = plain_r(plan, torch, x, y) if plan is not None else device_r(mod, torch, x, y, split)
    if want_layout:
        assert layout == want_layout
    res = sc.check(sc.Reference(x, y), r, spl[0], spl[1], layout, kind)
    print(res.summary())
    assert res.zmax < sc.Z_MAX, res.message()
    return res
