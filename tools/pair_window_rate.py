#!/usr/bin/env python3
"""What per-pair lag windows (asx_xcorr_windowed_f32_dev) cost against the plain strided call: pairs per second of
asx_xcorr_strided_f32_dev and of asx_xcorr_windowed_f32_dev with every row full ([-N, N-1]), so that both find the same peaks,
and of asx_xcorr_strided_f32_dev with the plan window [-N+1, N-1] (the plan-window kernels k_inv_cols_r<..., AsxWin>: what the masking of the
windowed inverse body costs by itself).

    python3 tools/pair_window_rate.py [--runs 9] [--warmup 2] [--cases 1440000x124,480000x1024] [--out FILE]

On asx_synth_pairs_dev pairs (contiguous: source stride 2N, sample stride N) it times, with HIP events on one plan per length,
the calls ALTERNATING (strided, windowed, plan window, strided, ...) so that clock drift falls on all, and reports the median of
--runs calls of each, the ratio, the inverse column time of each (asx_plan_timings_ms, profiling on) and whether the strided and
windowed calls returned the same bits.  The difference is the per-pair kernels' row loads and the
pass behind the Pearson kernels that rewrites invalid rows.  Prints one JSON line per length (and writes them to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
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
        rows = torch.tensor([[-n, n - 1]] * batch, dtype=torch.int64, device="cuda")
        out = {k: (torch.empty(batch, dtype=torch.int64, device="cuda"), torch.empty(batch, dtype=torch.float64, device="cuda"),
                   torch.empty(batch, dtype=torch.int32, device="cuda")) for k in ("strided", "windowed", "plan_window")}
        torch.cuda.synchronize()
        with asx.Plan(n, batch, 0) as plan:
            st = torch.cuda.Stream()
            sp = st.cuda_stream

            def call(kind):
                lag, coef, ret = (t.data_ptr() for t in out[kind])
                plan.set_lag_window(-n + 1 if kind == "plan_window" else -n, n - 1)
                if kind != "windowed":
                    plan.xcorr_strided_dev(d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, batch, lag, coef, ret, sp)
                else:
                    plan.xcorr_windowed_dev(d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n, rows.data_ptr(), 1, batch, lag, coef, ret, sp)

            kinds = ("strided", "windowed", "plan_window")
            times = {k: [] for k in kinds}
            inv = {k: [] for k in kinds}
            plan.set_profiling(1)
            with torch.cuda.stream(st):
                for _ in range(a.warmup):
                    for kind in kinds:
                        call(kind)
                for _ in range(a.runs):
                    for kind in kinds:
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        call(kind)
                        e1.record(st)
                        e1.synchronize()
                        times[kind].append(e0.elapsed_time(e1))
                        inv[kind].append(plan.last_timings_ms()["inv_cols"])
            ms = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            inv_ms = {k: sorted(v)[len(v) // 2] for k, v in inv.items()}
            same = all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(out["strided"], out["windowed"]))
            res = {"N": n, "batch": batch, "layout": plan.layout, "runs": a.runs,
                   "strided_ms": round(ms["strided"], 4), "windowed_ms": round(ms["windowed"], 4),
                   "strided_pairs_per_s": round(batch / (ms["strided"] / 1e3), 1),
                   "windowed_pairs_per_s": round(batch / (ms["windowed"] / 1e3), 1),
                   "plan_window_ms": round(ms["plan_window"], 4),
                   "windowed_over_strided": round(ms["windowed"] / ms["strided"], 4),
                   "plan_window_over_strided": round(ms["plan_window"] / ms["strided"], 4),
                   "inv_cols_ms": {k: round(v, 4) for k, v in inv_ms.items()},
                   "strided_spread_ms": round(max(times["strided"]) - min(times["strided"]), 4),
                   "windowed_spread_ms": round(max(times["windowed"]) - min(times["windowed"]), 4),
                   "same_bits": bool(same)}
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
