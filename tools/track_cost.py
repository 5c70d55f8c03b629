#!/usr/bin/env python3
"""What the lag track (asx_xcorr_track_f32_dev: k_track_dots per lag tile, k_track_sum past one block per segment and tile, then
k_track_fit) costs on a full launch group, next to the curve call's r pass, whose sweep it shares.

    python3 tools/track_cost.py [--n 144000] [--runs 21] [--warmup 3] [--calls r8,t8x1,t32x16,t64x64] [--out FILE]

One launch group's worth of device-resident pairs (batch = the plan's group; each sample is its source from frame 1000 on), one entry
per pair centred on lag 1000.  The calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  r8         asx_xcorr_curve_f32_dev with d_coef = NULL and half_width 8: the curve's r pass alone, one sweep over 8N bytes per entry
  t8x1       the track call with (half_width, segments) = (8, 1): the same sweep, one lag tile, one segment
  t32x16     (32, 16): four lag tiles, sixteen segments
  t64x64     (64, 64): eight lag tiles, sixty-four segments
Prints median, minimum and maximum in milliseconds and each track call's median over r8's, and appends the same text to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

SHAPES = {"t8x1": (8, 1), "t32x16": (32, 16), "t64x64": (64, 64)}


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
        r = torch.empty(b * 64 * 129, dtype=torch.float64, device="cuda")
        seg = torch.empty(b * 64 * 2, dtype=torch.float64, device="cuda")
        fit = torch.empty(b * 3, dtype=torch.float64, device="cuda")
        frac = torch.empty(b, dtype=torch.float64, device="cuda")
        used = torch.empty(b, dtype=torch.int32, device="cuda")
        ret = torch.empty(b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T = src.data_ptr(), smp.data_ptr()

        def curve():
            plan.xcorr_curve_dev(S, 2 * n, T, n, b, 1, centre.data_ptr(), 8, r.data_ptr(), 0, frac.data_ptr(), ret.data_ptr(), sp)

        def track(h, segs):
            plan.xcorr_track_dev(S, 2 * n, T, n, b, 1, centre.data_ptr(), h, segs, r.data_ptr(), seg.data_ptr(), fit.data_ptr(),
                                 used.data_ptr(), ret.data_ptr(), sp)

        calls = {"r8": curve}
        calls.update({k: (lambda hs=hs: track(*hs)) for k, hs in SHAPES.items()})
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
            track(32, 16)
            plan.sync(sp)
            assert ret.cpu().tolist() == [0] * b and used.cpu().tolist() == [16] * b
            got = r.cpu().numpy()[:b * 16 * 65].reshape(b, 16, 65)
            assert (got[:, :, 32] > 0.5 * n / 16).all() and (abs(got[:, :, 31]) < 0.1 * n / 16).all()      # the planted lag's ridge
            assert (abs(fit.cpu().numpy().reshape(b, 3)[:, 0]) * n < 0.05).all()                       # and no drift
        split = plan.split
        layout = plan.layout
    lines = ["N = %d, one group of %d pairs, one entry each, split %s (%s), %d alternating calls, %s"
             % (n, b, split, layout, a.runs, torch.cuda.get_device_name(0))]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, v in times.items():
        v = sorted(v)
        ratio = "  %5.2f x r8" % (med[k] / med["r8"]) if k != "r8" and "r8" in med else ""
        lines.append("  %-8s median %9.4f  min %9.4f  max %9.4f ms%s" % (k, v[len(v) // 2], v[0], v[-1], ratio))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
