#!/usr/bin/env python3
"""What the PHAT calls (asx_xcorr_phat_f32_dev, asx_xcorr_phat_band_f32_dev) cost next to the plain strided call on the same pairs.

    python3 tools/phat_cost.py [--n 1440000] [--pairs 124] [--runs 21] [--warmup 3] [--band LO HI] [--out FILE]

One group of --pairs generator pairs of length --n, device resident.  The plain call runs with asx_plan_set_pearson(plan, 0) and
asx_plan_set_prune(plan, 0): the same passes as the PHAT call but for the row flavour (k_rows_r / k_rows_rp) and the tail
(k_finalize and the exact re-evaluation / k_phat_finalize).  The banded call (--band, bins of the 2N-point transform; default 1 .. N/6)
is the PHAT call with the row flavour k_rows_rb.  The three calls ALTERNATE within each of --runs rounds; the phases come
from the plan's own events (asx_plan_set_profiling, asx_plan_timings_ms).  Prints the medians per phase in milliseconds and the
commit, and writes the same text to --out."""
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
    ap.add_argument("--pairs", type=int, default=124)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--band", type=int, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n, b = a.n, a.pairs
    lo, hi = a.band if a.band else (1, n // 6)
    assert (lo, hi) != (0, n), "the full band is the PHAT call itself"
    src = torch.empty((b, 2 * n), dtype=torch.float32, device="cuda")
    smp = torch.empty((b, n), dtype=torch.float32, device="cuda")
    asx.synth_pairs_dev(2024, 0, b, n, 1, src.data_ptr(), smp.data_ptr())
    lag = torch.empty(b, dtype=torch.int64, device="cuda")
    coef = torch.empty(b, dtype=torch.float64, device="cuda")
    peak = torch.empty(b, dtype=torch.float64, device="cuda")
    ret = torch.empty(b, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    times = {"plain": [], "phat": [], "band": []}
    with asx.Plan(n, b, 0) as plan:
        assert plan.group >= b, (plan.group, b)
        plan.set_pearson(False)
        plan.set_prune(False)
        plan.set_profiling(2)
        calls = {
            "plain": lambda: plan.xcorr_strided_dev(src.data_ptr(), 2 * n, smp.data_ptr(), n, b, lag.data_ptr(), coef.data_ptr(),
                                                    ret.data_ptr()),
            "phat": lambda: plan.xcorr_phat_dev(src.data_ptr(), 2 * n, smp.data_ptr(), n, 0, 0, b, lag.data_ptr(), coef.data_ptr(),
                                                peak.data_ptr(), ret.data_ptr()),
            "band": lambda: plan.xcorr_phat_band_dev(src.data_ptr(), 2 * n, smp.data_ptr(), n, 0, 0, b, lo, hi, lag.data_ptr(),
                                                     coef.data_ptr(), peak.data_ptr(), ret.data_ptr()),
        }
        for r in range(a.warmup + a.runs):
            for k, fn in calls.items():
                fn()
                plan.sync()
                if r >= a.warmup:
                    times[k].append(plan.last_timings_ms())
        layout, split = plan.layout, plan.split
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    med = {k: {p: sorted(t[p] for t in v)[len(v) // 2] for p in PHASES} for k, v in times.items()}
    lines = ["PHAT calls against the plain strided call (direct Pearson form, no pruned pass): medians over %d alternating calls, ms"
             % a.runs,
             "commit %s  N = %d, one group of %d pairs, band [%d, %d], %s plan, split %s, %s"
             % (commit or "?", n, b, lo, hi, layout, split, torch.cuda.get_device_name(0)),
             "%-10s" % "phase" + "".join("%12s" % k for k in med) + "%12s%12s" % ("phat/plain", "band/phat")]

    def ratio(x, y):
        return "%12.3f" % (x / y) if y > 0 else "%12s" % "-"
    for p in PHASES:
        lines.append("%-10s" % p + "".join("%12.4f" % med[k][p] for k in med) + ratio(med["phat"][p], med["plain"][p])
                     + ratio(med["band"][p], med["phat"][p]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
