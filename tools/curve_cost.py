#!/usr/bin/env python3
"""What the curve around given lags (asx_xcorr_curve_f32_dev: k_curve_dots, then one direct Pearson pass per neighbour) costs on a
full launch group, next to the two things it stands in for.

    python3 tools/curve_cost.py [--n 144000] [--runs 21] [--warmup 3] [--calls r1,r8,full1,full8,win1,win8] [--out FILE]

One launch group's worth of device-resident pairs (batch = the plan's group; each sample is its source from frame 1000 on), one entry
per pair centred on lag 1000.  The calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  r1, r8        the call with d_coef = NULL, half_width 1 and 8: the r pass alone (k_curve_dots and, past one block per entry, k_curve_sum)
  full1, full8  the call with d_coef: the r pass plus 2h + 1 direct Pearson passes; full - r is the coefficient curve
  win1, win8    what a caller had before: 2h + 1 asx_xcorr_windowed_f32_dev calls with the rows [l, l], direct Pearson form
Then, in the same process, ONE direct Pearson pass of the same group -- the same 8N bytes per pair -- from the plan's own kernel
events (asx_plan_set_profiling) around an asx_xcorr_strided_f32_dev call under asx_plan_set_pearson(plan, 0), --runs times.
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
        r = torch.empty(b * 17, dtype=torch.float64, device="cuda")
        cf = torch.empty(b * 17, dtype=torch.float64, device="cuda")
        frac = torch.empty(b, dtype=torch.float64, device="cuda")
        lag = torch.empty(b, dtype=torch.int64, device="cuda")
        coef = torch.empty(b, dtype=torch.float64, device="cuda")
        ret = torch.empty(b, dtype=torch.int32, device="cuda")
        rows = {d: torch.full((b, 2), 1000 + d, dtype=torch.int64, device="cuda") for d in range(-8, 9)}
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T = src.data_ptr(), smp.data_ptr()
        plan.set_pearson(False)

        def curve(h, with_coef):
            plan.xcorr_curve_dev(S, 2 * n, T, n, b, 1, centre.data_ptr(), h, r.data_ptr(), cf.data_ptr() if with_coef else 0,
                                 frac.data_ptr(), ret.data_ptr(), sp)

        def windowed(h):
            for d in range(-h, h + 1):
                plan.xcorr_windowed_dev(S, 2 * n, T, n, rows[d].data_ptr(), 1, b, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)

        calls = {"r1": lambda: curve(1, False), "r8": lambda: curve(8, False), "full1": lambda: curve(1, True),
                 "full8": lambda: curve(8, True), "win1": lambda: windowed(1), "win8": lambda: windowed(8)}
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
            curve(8, True)
            plan.sync(sp)
            assert ret.cpu().tolist() == [0] * b
            got = r.cpu().numpy().reshape(b, 17)
            assert (got[:, 8] > 0.5 * n).all() and (abs(got[:, 7]) < 0.1 * n).all()          # the planted lag's peak
            assert (abs(cf.cpu().numpy().reshape(b, 17)[:, 8] - 1.0) < 1e-12).all()
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
    for k, v in times.items():
        v = sorted(v)
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms" % (k, v[len(v) // 2], v[0], v[-1]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
