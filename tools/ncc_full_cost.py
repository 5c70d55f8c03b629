#!/usr/bin/env python3
"""What the full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev) costs on full launch groups, next to the NCC call
(asx_xcorr_ncc_f32_dev) on the same plan and pairs.

    python3 tools/ncc_full_cost.py [--n 144000] [--runs 21] [--warmup 3] [--out FILE]

One plan group's worth of device-resident pairs (batch = the plan's group).  In each pair the sample starts 1000 frames before the
source: its frames from 1000 on are the source's first N - 1000 plus noise, so the NCC call finds nothing and the full-range call
lag -1000.  The calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  ncc       asx_xcorr_ncc_f32_dev without rows, min_energy 1e-3: NCC groups of at most 2^30 / 24N pairs
  full      asx_xcorr_ncc_full_f32_dev without rows, min_energy 1e-3, min_overlap (N + 1) / 2: groups of at most 2^30 / 72N pairs
  ncc_bc    the NCC call with the first source for every pair (a stride of 0)
  full_bc   the full-range call with the first source for every pair: its moments, staged copy and tables once per call
Prints median, minimum and maximum in milliseconds, and appends the same text to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n = a.n
    shift = 1000
    with asx.Plan(n, 4096, 0) as plan:
        b = plan.group
        gen = torch.Generator(device="cuda").manual_seed(2024)
        src = torch.randn((b, 2 * n), dtype=torch.float32, device="cuda", generator=gen)
        smp = torch.randn((b, n), dtype=torch.float32, device="cuda", generator=gen)
        smp[:, shift:] = src[:, :n - shift] + 0.5 * smp[:, shift:]
        lag = torch.empty(b, dtype=torch.int64, device="cuda")
        coef = torch.empty(b, dtype=torch.float64, device="cuda")
        peak = torch.empty(b, dtype=torch.float64, device="cuda")
        ret = torch.empty(b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T = src.data_ptr(), smp.data_ptr()
        out4 = (lag.data_ptr(), coef.data_ptr(), peak.data_ptr(), ret.data_ptr())
        mo = (n + 1) // 2
        calls = {"ncc": lambda: plan.xcorr_ncc_dev(S, 2 * n, T, n, 0, 0, b, 1e-3, *out4, sp),
                 "full": lambda: plan.xcorr_ncc_full_dev(S, 2 * n, T, n, 0, 0, b, 1e-3, mo, *out4, sp),
                 "ncc_bc": lambda: plan.xcorr_ncc_dev(S, 0, T, n, 0, 0, b, 1e-3, *out4, sp),
                 "full_bc": lambda: plan.xcorr_ncc_full_dev(S, 0, T, n, 0, 0, b, 1e-3, mo, *out4, sp)}
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
            calls["full"]()
            plan.sync(sp)
            assert ret.cpu().tolist() == [0] * b and lag.cpu().tolist() == [-shift] * b
            assert (abs(peak.cpu().numpy() - 0.8944) < 0.01).all()        # 1 / sqrt(1.25)
            calls["ncc"]()
            plan.sync(sp)
            assert (peak.cpu().numpy() < 0.2).all()                       # no lag >= 0 has anything to offer
        split = plan.split
        layout = plan.layout
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = ["N = %d, %d pairs (the plan's group; NCC groups of %d, full-range groups of %d), split %s (%s), %d alternating calls, %s"
             % (n, b, max(1, min(b, (1 << 30) // (24 * n))), max(1, min(b, (1 << 30) // (72 * n))), split, layout, a.runs,
                torch.cuda.get_device_name(0))]
    for k, v in times.items():
        v = sorted(v)
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms" % (k, med[k], v[0], v[-1]))
    lines.append("  full / ncc = %.2f, full_bc / ncc_bc = %.2f (medians)" % (med["full"] / med["ncc"], med["full_bc"] / med["ncc_bc"]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
