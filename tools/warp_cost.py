#!/usr/bin/env python3
"""What the warped correlation (asx_xcorr_warp_f32_dev: k_warp_dots, then k_warp_final) costs on a full launch group, next to what r
and one coefficient at a constant lag cost without it: the curve call's r pass plus one direct Pearson pass.

    python3 tools/warp_cost.py [--n 144000] [--runs 21] [--warmup 3] [--calls r1,r8,w1,w8,w1d,w8d] [--out FILE]

One launch group's worth of device-resident pairs (batch = the plan's group; each sample is its source from frame 1000 on), one entry
per pair centred on lag 1000.  The calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  r1, r8     asx_xcorr_curve_f32_dev with d_coef = NULL and half_width 1, 8: the curve's r pass alone
  w1, w8     the warp call on the line (0, 0): no frame steps, one window per thread
  w1d, w8d   the warp call on the line (12 / N, 0.25): every sixteenth thread or so holds a step and reads a second window
Then, the group alone: `pearson`, one direct Pearson pass over it (what one windowed call with [l, l] rows adds to its transforms), by
the plan's own events (asx_plan_set_profiling) around asx_xcorr_strided_f32_dev under asx_plan_set_pearson(plan, 0).
Prints median, minimum and maximum in milliseconds, each warp call's median over r + pearson, and appends the same text to --out."""
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
    ap.add_argument("--calls", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n = a.n
    with asx.Plan(n, 4096, 0) as plan:
        b = plan.group
        gen = torch.Generator(device="cuda").manual_seed(2024)
        src = torch.randn((b, 2 * n), dtype=torch.float32, device="cuda", generator=gen)
        smp = src[:, 1000:1000 + n].contiguous()
        centre = torch.full((b,), 1000, dtype=torch.int64, device="cuda")
        flat = torch.tensor([0.0, 0.0], dtype=torch.float64, device="cuda")
        drift = torch.tensor([12.0 / n, 0.25], dtype=torch.float64, device="cuda")
        r = torch.empty(b * 17, dtype=torch.float64, device="cuda")
        frac = torch.empty(b, dtype=torch.float64, device="cuda")
        coef = torch.empty(b, dtype=torch.float64, device="cuda")
        length = torch.empty(b, dtype=torch.int64, device="cuda")
        lag = torch.empty(b, dtype=torch.int64, device="cuda")
        ret = torch.empty(b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T = src.data_ptr(), smp.data_ptr()
        plan.set_pearson(False)

        def curve(h):
            plan.xcorr_curve_dev(S, 2 * n, T, n, b, 1, centre.data_ptr(), h, r.data_ptr(), 0, frac.data_ptr(), ret.data_ptr(), sp)

        def warp(h, line):
            plan.xcorr_warp_dev(S, 2 * n, T, n, b, 1, centre.data_ptr(), line.data_ptr(), 0, h, r.data_ptr(), frac.data_ptr(),
                                coef.data_ptr(), length.data_ptr(), ret.data_ptr(), sp)

        calls = {"r1": lambda: curve(1), "r8": lambda: curve(8), "w1": lambda: warp(1, flat), "w8": lambda: warp(8, flat),
                 "w1d": lambda: warp(1, drift), "w8d": lambda: warp(8, drift)}
        if a.calls:
            calls = {k: fn for k, fn in calls.items() if k in a.calls.split(",")}
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
            warp(8, flat)
            plan.sync(sp)
            assert ret.cpu().tolist() == [0] * b and length.cpu().tolist() == [n] * b
            got = r.cpu().numpy().reshape(b, 17)
            assert (got[:, 8] > 0.5 * n).all() and (abs(got[:, 7]) < 0.1 * n).all()          # the planted lag's peak
            assert (abs(coef.cpu().numpy() - 1.0) < 1e-12).all()
            # one direct Pearson pass of the group, by the plan's own events
            plan.set_profiling(1)
            pearson = []
            for run in range(a.warmup + a.runs):
                plan.xcorr_strided_dev(S, 2 * n, T, n, b, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)
                plan.sync(sp)
                if run >= a.warmup:
                    pearson.append(plan.last_timings_ms()["pearson"])
            plan.set_profiling(0)
            times["pearson"] = pearson
        split = plan.split
        layout = plan.layout
    lines = ["N = %d, one group of %d pairs, one entry each, split %s (%s), %d alternating calls, %s"
             % (n, b, split, layout, a.runs, torch.cuda.get_device_name(0))]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        v = sorted(v)
        base = "r" + k[1] if k.startswith("w") else None
        ratio = ""
        if base in med:
            ratio = "  %6.4f ms per entry, %5.2f x (%s + pearson)" % (med[k] / b, med[k] / (med[base] + med["pearson"]), base)
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms%s" % (k, v[len(v) // 2], v[0], v[-1], ratio))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
