#!/usr/bin/env python3
"""What the pool and top-k forms of the normalised cross-correlation cost: all pairs of one pool of C clips, next to the strided
NCC call on the same pairs materialised and the raw pool call, on one plan.

    python3 tools/ncc_pool_cost.py [--n 144000] [--clips 35] [--runs 21] [--warmup 3] [--out FILE]

Clip c is fixture-C-like (tests/ncc_topk_model.py): its sample is unit noise + 0.25, its source unit noise plus 0.3 / 1.0 / 0.6 times
the sample at lags N/10, N/2 and 8N/10 and a level step of 2.0 from frame 1.3 N on.  The C x C pairs are every source against every
sample: the C matched pairs hold three peaks, the others none (a runner-up at the noise floor).  The method is tools/ncc_cost.py's:
the calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  pool      asx_xcorr_pool_f32_dev, asynchronous mode (asx_plan_set_exact(plan, 0)), as the plan is created otherwise
  ncc       asx_xcorr_ncc_f32_dev on the materialised pairs [C * C][2N], [C * C][N]
  pool_ncc  asx_xcorr_pool_ncc_f32_dev
  k = 2, 4, 8   asx_xcorr_pool_ncc_topk_f32_dev, min_separation N / 100
Prints median, minimum and maximum in milliseconds and the ratios, and appends the same text to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--clips", type=int, default=35)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n, c = a.n, a.clips
    b = c * c
    lags = (n // 10, n // 2, (8 * n) // 10)
    with asx.Plan(n, 4096, 0) as plan:
        gen = torch.Generator(device="cuda").manual_seed(3000)
        smp = torch.randn((c, n), dtype=torch.float32, device="cuda", generator=gen) + 0.25
        src = torch.randn((c, 2 * n), dtype=torch.float32, device="cuda", generator=gen)
        for gain, lag in zip((0.3, 1.0, 0.6), lags):
            src[:, lag:lag + n] += gain * smp
        src[:, (13 * n) // 10:] += 2.0
        ia = torch.arange(c, device="cuda").repeat_interleave(c)
        ib = torch.arange(c, device="cuda").repeat(c)
        src_m, smp_m = src[ia].contiguous(), smp[ib].contiguous()
        kmax = 8
        lag = torch.empty(b * kmax, dtype=torch.int64, device="cuda")
        coef = torch.empty(b * kmax, dtype=torch.float64, device="cuda")
        peak = torch.empty(b * kmax, dtype=torch.float64, device="cuda")
        ret = torch.empty(b * kmax, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T, SM, TM = src.data_ptr(), smp.data_ptr(), src_m.data_ptr(), smp_m.data_ptr()
        plan.set_exact(False)
        out3 = (lag.data_ptr(), coef.data_ptr(), ret.data_ptr())
        out4 = (lag.data_ptr(), coef.data_ptr(), peak.data_ptr(), ret.data_ptr())
        sep = n // 100

        def topk(k):
            return lambda: plan.xcorr_pool_ncc_topk_dev(S, 2 * n, c, T, n, c, 0, 0, 0, b, 1e-3, k, sep, *out4, sp)

        calls = {"pool": lambda: plan.xcorr_pool_dev(S, 2 * n, c, T, n, c, 0, 0, 0, b, *out3, sp),
                 "ncc": lambda: plan.xcorr_ncc_dev(SM, 2 * n, TM, n, 0, 0, b, 1e-3, *out4, sp),
                 "pool_ncc": lambda: plan.xcorr_pool_ncc_dev(S, 2 * n, c, T, n, c, 0, 0, 0, b, 1e-3, *out4, sp),
                 "k = 2": topk(2), "k = 4": topk(4), "k = 8": topk(8)}
        times = {k: [] for k in calls}
        with torch.cuda.stream(st):
            for run in range(a.warmup + a.runs):
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    if run >= a.warmup:
                        times[k].append(e0.elapsed_time(e1))
            calls["ncc"]()
            plan.sync(sp)
            want = [t[:b].cpu().numpy().tobytes() for t in (lag, coef, peak, ret)]
            calls["pool_ncc"]()
            plan.sync(sp)
            assert [t[:b].cpu().numpy().tobytes() for t in (lag, coef, peak, ret)] == want, "the pool call is not the strided call's bits"
            calls["k = 4"]()
            plan.sync(sp)
            top = lag[:4 * b].cpu().reshape(c, c, 4)
            for i in range(c):
                assert top[i, i, :3].tolist() == [lags[1], lags[2], lags[0]], (i, top[i, i])
        group, split, layout = plan.group, plan.split, plan.layout
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = ["N = %d, C = %d clips, %d pairs (plan group %d; NCC groups of %d), split %s (%s), %d alternating calls, %s"
             % (n, c, b, group, max(1, min(group, (1 << 30) // (24 * n))), split, layout, a.runs, torch.cuda.get_device_name(0))]
    for k, v in times.items():
        v = sorted(v)
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms" % (k, v[len(v) // 2], v[0], v[-1]))
    lines.append("  pool_ncc / pool = %.2f, ncc / pool = %.2f, pool_ncc / ncc = %.2f (medians)"
                 % (med["pool_ncc"] / med["pool"], med["ncc"] / med["pool"], med["pool_ncc"] / med["ncc"]))
    lines.append("  per extra entry, against k = 1 (pool_ncc): k = 2 %+.4f ms, k = 4 %+.4f ms, k = 8 %+.4f ms = %.2f %%, %.2f %%, %.2f %% of it; "
                 "per pair and entry %.2f, %.2f, %.2f us"
                 % tuple([(med["k = %d" % k] - med["pool_ncc"]) / (k - 1) for k in (2, 4, 8)]
                         + [100 * (med["k = %d" % k] - med["pool_ncc"]) / (k - 1) / med["pool_ncc"] for k in (2, 4, 8)]
                         + [1e3 * (med["k = %d" % k] - med["pool_ncc"]) / (k - 1) / b for k in (2, 4, 8)]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
