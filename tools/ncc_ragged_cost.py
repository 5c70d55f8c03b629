#!/usr/bin/env python3
"""What the ragged normalised cross-correlation (asx_xcorr_ncc_ragged_f32_dev) costs on full launch groups, next to the full-range
call (asx_xcorr_ncc_full_f32_dev) on the same plan and pairs.

    python3 tools/ncc_ragged_cost.py [--n 144000] [--runs 21] [--warmup 3] [--out FILE]

One plan group's worth of device-resident pairs (batch = the plan's group), tools/ncc_full_cost.py's: in each pair the sample starts
1000 frames before the source, so both calls return lag -1000 at the plan's shape.  The calls ALTERNATE within each of --runs rounds,
each between two events on the stream:
  full      asx_xcorr_ncc_full_f32_dev without rows, min_energy 1e-3, min_overlap (N + 1) / 2: groups of at most 2^30 / 72N pairs
  ragged    asx_xcorr_ncc_ragged_f32_dev with d_lengths == NULL, i.e. (2N, N): groups of at most 2^30 / 84N pairs
  rows      the ragged call with a row (2N, N) per pair in device memory
  short     the ragged call with (1.5 N, 0.7 N) for every pair (one row, a length_stride of 0)
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
        rows = torch.tensor([[2 * n, n]] * b, dtype=torch.int64, device="cuda")
        short = torch.tensor([(3 * n) // 2, (7 * n) // 10], dtype=torch.int64, device="cuda")
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
        calls = {"full": lambda: plan.xcorr_ncc_full_dev(S, 2 * n, T, n, 0, 0, b, 1e-3, mo, *out4, sp),
                 "ragged": lambda: plan.xcorr_ncc_ragged_dev(S, 2 * n, T, n, 0, 0, 0, 0, b, 1e-3, mo, *out4, sp),
                 "rows": lambda: plan.xcorr_ncc_ragged_dev(S, 2 * n, T, n, rows.data_ptr(), 1, 0, 0, b, 1e-3, mo, *out4, sp),
                 "short": lambda: plan.xcorr_ncc_ragged_dev(S, 2 * n, T, n, short.data_ptr(), 0, 0, 0, b, 1e-3, mo, *out4, sp)}
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
            for k in ("full", "ragged", "rows", "short"):
                calls[k]()
                plan.sync(sp)
                assert ret.cpu().tolist() == [0] * b and lag.cpu().tolist() == [-shift] * b, k
                assert (abs(peak.cpu().numpy() - 0.8944) < 0.01).all(), k    # 1 / sqrt(1.25)
        split = plan.split
        layout = plan.layout
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = ["N = %d, %d pairs (the plan's group; full-range groups of %d, ragged groups of %d), split %s (%s), %d alternating calls, %s"
             % (n, b, max(1, min(b, (1 << 30) // (72 * n))), max(1, min(b, (1 << 30) // (84 * n))), split, layout, a.runs,
                torch.cuda.get_device_name(0))]
    for k, v in times.items():
        v = sorted(v)
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms" % (k, med[k], v[0], v[-1]))
    lines.append("  ragged / full = %.2f, rows / full = %.2f, short / full = %.2f (medians)"
                 % (med["ragged"] / med["full"], med["rows"] / med["full"], med["short"] / med["full"]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
