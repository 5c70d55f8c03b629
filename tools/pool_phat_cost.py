#!/usr/bin/env python3
"""What GCC-PHAT over a pool (asx_xcorr_pool_phat_f32_dev) costs next to the plain pool call and to the strided PHAT call on the same
pairs.

    python3 tools/pool_phat_cost.py [--n 1440000] [--clips 11] [--runs 21] [--warmup 3] [--band LO HI] [--out FILE]

One pool of --clips clips of 2N frames, cut from one recording so that consecutive clips overlap by half, device resident, passed
as both pools (a clip's first N frames are the sample): all clips x clips pairs, which should fill one launch group.  Three calls:
  pool_phat   asx_xcorr_pool_phat_f32_dev over every combination: 2 x clips forward column passes into the bank, k_rows_rlp / k_rows_rlb
  pool        asx_xcorr_pool_f32_dev on the same pools under asx_plan_set_pearson(plan, 0): the same passes but for the row flavour
              (k_rows_rl) and the tail
  strided     asx_xcorr_phat_band_f32_dev on materialised copies of the same pairs (made once, outside the timing): clips x clips
              forward column passes of each operand, k_rows_rp / k_rows_rb
--band are bins of the 2N-point transform (default 1 .. N/6; 0 N is the full band, plain PHAT).  The three calls ALTERNATE within
each of --runs rounds.  The phases come from the plan's own events (asx_plan_set_profiling, asx_plan_timings_ms), which begin behind
a pool call's bank fill: `call` is the whole call between two events on the stream, and `forward` = fwd_cols + (call - total) is
everything in front of the row pass, the bank fill included.  Prints the medians in milliseconds and the commit, and writes the same
text to --out."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

PHASES = ("fwd_cols", "rows", "inv_cols", "finalize", "pearson", "total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1440000)
    ap.add_argument("--clips", type=int, default=11)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--band", type=int, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n, c = a.n, a.clips
    b = c * c
    lo, hi = a.band if a.band else (1, n // 6)
    gen = torch.Generator(device="cuda").manual_seed(2024)
    rec = torch.randn(n * (c + 1), dtype=torch.float32, device="cuda", generator=gen)
    clips = torch.stack([rec[k * n:k * n + 2 * n] for k in range(c)]).contiguous()      # clip k starts at k N
    rep_src = clips.repeat_interleave(c, dim=0).contiguous()                            # pair (a, b) at a c + b, source-major
    rep_smp = clips[:, :n].repeat(c, 1).contiguous()
    lag = torch.empty(b, dtype=torch.int64, device="cuda")
    coef = torch.empty(b, dtype=torch.float64, device="cuda")
    peak = torch.empty(b, dtype=torch.float64, device="cuda")
    ret = torch.empty(b, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    times = {"pool_phat": [], "pool": [], "strided": []}
    with asx.Plan(n, b, 0) as plan:
        assert plan.group >= b, (plan.group, b)
        plan.set_pearson(False)
        plan.set_profiling(2)
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        P = clips.data_ptr()
        calls = {
            "pool_phat": lambda: plan.xcorr_pool_phat_dev(P, 2 * n, c, P, 2 * n, c, 0, 0, 0, b, lo, hi, lag.data_ptr(), coef.data_ptr(),
                                                          peak.data_ptr(), ret.data_ptr(), sp),
            "pool": lambda: plan.xcorr_pool_dev(P, 2 * n, c, P, 2 * n, c, 0, 0, 0, b, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp),
            "strided": lambda: plan.xcorr_phat_band_dev(rep_src.data_ptr(), 2 * n, rep_smp.data_ptr(), n, 0, 0, b, lo, hi, lag.data_ptr(),
                                                        coef.data_ptr(), peak.data_ptr(), ret.data_ptr(), sp),
        }
        with torch.cuda.stream(st):
            for r in range(a.warmup + a.runs):
                for k, fn in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    plan.sync(sp)
                    if r >= a.warmup:
                        t = plan.last_timings_ms()
                        t["call"] = e0.elapsed_time(e1)
                        t["forward"] = t["fwd_cols"] + t["call"] - t["total"]
                        times[k].append(t)
        layout, split, bank = plan.layout, plan.split, plan.debug_bank()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    rows = PHASES + ("call", "forward")
    med = {k: {p: sorted(t[p] for t in v)[len(v) // 2] for p in rows} for k, v in times.items()}
    lines = ["PHAT over a pool against the plain pool call (direct Pearson form) and the strided PHAT call on copies of the pairs: medians "
             "over %d alternating calls, ms" % a.runs,
             "commit %s  N = %d, %d clips as both pools, one group of %d pairs, band [%d, %d], %s plan, split %s, bank %s, %s"
             % (commit or "?", n, c, b, lo, hi, layout, split, bank[:2], torch.cuda.get_device_name(0)),
             "%-10s" % "phase" + "".join("%12s" % k for k in med) + "%14s%16s" % ("phat - pool", "strided - phat")]
    for p in rows:
        lines.append("%-10s" % p + "".join("%12.4f" % med[k][p] for k in med)
                     + "%14.4f%16.4f" % (med["pool_phat"][p] - med["pool"][p], med["strided"][p] - med["pool_phat"][p]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
