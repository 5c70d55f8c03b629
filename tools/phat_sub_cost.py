#!/usr/bin/env python3
"""What the sub-sample PHAT call (asx_xcorr_phat_sub_f32_dev: k_phat_near behind each group's tail) costs next to the banded PHAT
call on the same pairs.

    python3 tools/phat_sub_cost.py [--n 144000] [--runs 21] [--warmup 3] [--band LO HI] [--calls band,sub1,sub8] [--pkg DIR] [--out FILE]

One launch group's worth of device-resident pairs (batch = the plan's group; each sample is its source from frame 1000 on, so every
pair has a sharp peak).  The calls ALTERNATE within each of --runs rounds, each between two events on the stream:
  band   asx_xcorr_phat_band_f32_dev
  sub1   asx_xcorr_phat_sub_f32_dev, half_width 1    (only when the library has the call)
  sub8   asx_xcorr_phat_sub_f32_dev, half_width 8
--pkg names another build of the package directory (a parent commit's, for instance): a library without the sub call times `band`
alone, so that alternating processes compare the two builds' banded call.  --band are bins of the 2N-point transform (default the
full band); --calls keeps only the named calls (a kernel trace of one half width).  Prints median, minimum and maximum in
milliseconds, and appends the same text to --out."""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def load_from(pkg_dir):
    spec = importlib.util.spec_from_file_location("audiosync_amd", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["audiosync_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--band", type=int, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--calls", default=None)
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = load_from(os.path.abspath(a.pkg)) if a.pkg else graft.load()
    n = a.n
    lo, hi = a.band if a.band else (0, n)
    with asx.Plan(n, 4096, 0) as plan:
        b = plan.group
        gen = torch.Generator(device="cuda").manual_seed(2024)
        src = torch.randn((b, 2 * n), dtype=torch.float32, device="cuda", generator=gen)
        smp = src[:, 1000:1000 + n].contiguous()
        lag = torch.empty(b, dtype=torch.int64, device="cuda")
        coef = torch.empty(b, dtype=torch.float64, device="cuda")
        peak = torch.empty(b, dtype=torch.float64, device="cuda")
        frac = torch.empty(b, dtype=torch.float64, device="cuda")
        near = torch.empty(b * 17, dtype=torch.float64, device="cuda")
        ret = torch.empty(b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        S, T = src.data_ptr(), smp.data_ptr()
        calls = {"band": lambda: plan.xcorr_phat_band_dev(S, 2 * n, T, n, 0, 0, b, lo, hi, lag.data_ptr(), coef.data_ptr(), peak.data_ptr(),
                                                          ret.data_ptr(), sp)}
        if hasattr(plan, "xcorr_phat_sub_dev"):
            for h in (1, 8):
                calls["sub%d" % h] = lambda h=h: plan.xcorr_phat_sub_dev(S, 2 * n, T, n, 0, 0, b, lo, hi, h, lag.data_ptr(), coef.data_ptr(),
                                                                         peak.data_ptr(), frac.data_ptr(), near.data_ptr(), ret.data_ptr(), sp)
        if a.calls:
            calls = {k: fn for k, fn in calls.items() if k in a.calls.split(",")}
        times = {k: [] for k in calls}
        with torch.cuda.stream(st):
            for r in range(a.warmup + a.runs):
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    if r >= a.warmup:
                        times[k].append(e0.elapsed_time(e1))
        assert lag.cpu().tolist() == [1000] * b and ret.cpu().tolist() == [0] * b
        split = plan.split
    lines = ["%s  N = %d, one group of %d pairs, band [%d, %d], split %s, %d alternating calls, %s"
             % (a.pkg or "this tree", n, b, lo, hi, split, a.runs, torch.cuda.get_device_name(0))]
    for k, v in times.items():
        v = sorted(v)
        lines.append("  %-5s median %8.4f  min %8.4f  max %8.4f ms" % (k, v[len(v) // 2], v[0], v[-1]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
