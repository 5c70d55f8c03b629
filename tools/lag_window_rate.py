#!/usr/bin/env python3
"""What a lag window (asx_plan_set_lag_window) costs: pairs per second of asx_xcorr_batch_f32_dev with the full window against
windows that exclude lags.

    python3 tools/lag_window_rate.py [--runs 7] [--warmup 2] [--out FILE]

At N = 1 440 000 x 124 and N = 480 000 x 1024 synthetic pairs (asx_synth_pairs_dev: true lags up to a quarter of N) it times, with
HIP events on one plan per length, the median of --runs calls for each window:
  full      [-N, N-1]: the kernels of a plan that never had a window
  pm2s      +-2 s (+-96 000 frames): the windowed inverse column kernel
  exclude   [N/2, N-1]: a window that excludes most true lags, so the in-window maximum is small against the same error bound
and reports the inverse column and finalize (+ exact re-evaluation) times of the last call (asx_plan_timings_ms) and the plan's
overflow and repair counters.  The window does not prune work; any difference is the masking and the candidate lists.
Prints one JSON line per length and window (and writes them to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="1440000x124,480000x1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    lines = []
    for case in a.cases.split(","):
        n, batch = (int(v) for v in case.split("x"))
        d_src = torch.empty(batch * 2 * n, dtype=torch.float32, device="cuda")
        d_smp = torch.empty(batch * n, dtype=torch.float32, device="cuda")
        d_true = torch.empty(batch, dtype=torch.int64, device="cuda")
        asx.synth_pairs_dev(2024, 0, batch, n, 1, d_src.data_ptr(), d_smp.data_ptr(), d_true.data_ptr())
        torch.cuda.synchronize()
        true_lag = d_true.cpu()
        lag = torch.empty(batch, dtype=torch.int64, device="cuda")
        coef = torch.empty(batch, dtype=torch.float64, device="cuda")
        ret = torch.empty(batch, dtype=torch.int32, device="cuda")
        with asx.Plan(n, batch, 0) as plan:
            st = torch.cuda.Stream()
            sp = st.cuda_stream
            plan.set_profiling(1)
            for name, (lo, hi) in (("full", (-n, n - 1)), ("pm2s", (-96000, 96000)), ("exclude", (n // 2, n - 1))):
                plan.set_lag_window(lo, hi)
                ov0, rep0 = plan.peak_overflows(), plan.peak_repairs()
                with torch.cuda.stream(st):
                    for _ in range(a.warmup):
                        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)
                    times = []
                    for _ in range(a.runs):
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)
                        e1.record(st)
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1))
                times.sort()
                ms = times[len(times) // 2]
                t = plan.last_timings_ms()
                inside = ((true_lag >= lo) & (true_lag <= hi)).sum().item()
                res = {"N": n, "batch": batch, "window": name, "lo": lo, "hi": hi, "runs": a.runs, "layout": plan.layout,
                       "pairs_per_s": round(batch / (ms / 1e3), 1), "ms": round(ms, 4),
                       "inv_cols_ms": round(t["inv_cols"], 4), "finalize_refine_ms": round(t["finalize"], 4),
                       "true_lags_in_window": inside, "lag_is_true": int((lag.cpu() == true_lag).sum().item()),
                       "overflows": plan.peak_overflows() - ov0, "repairs": plan.peak_repairs() - rep0}
                print(json.dumps(res), flush=True)
                lines.append(res)
        del d_src, d_smp
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
