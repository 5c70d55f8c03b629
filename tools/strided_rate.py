#!/usr/bin/env python3
"""Pairs per second of the strided entry point (asx_xcorr_strided_f32_dev) against the contiguous one on materialised copies.

    python3 tools/strided_rate.py [--runs 7] [--warmup 2] [--out FILE]

At N = 1 440 000 x 124 and N = 480 000 x 1024 pairs it times, with HIP events on one plan per length, the median of --runs calls:
  contiguous   asx_xcorr_batch_f32_dev on `batch` materialised pairs (the shared track copied batch times)
  bcast_source one source, `batch` samples (source stride 0)
  bcast_sample one sample, `batch` sources (sample stride 0)
  windows      overlapping windows of one recording of (batch + 1) N frames, hop N, one sample
Prints one JSON line per length (and writes them to --out)."""
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
        d_lag = torch.empty(batch, dtype=torch.int64, device="cuda")
        asx.synth_pairs_dev(2024, 0, batch, n, 1, d_src.data_ptr(), d_smp.data_ptr(), d_lag.data_ptr())
        torch.cuda.synchronize()
        one_src = d_src[:2 * n].clone()
        one_smp = d_smp[:n].clone()
        # materialised copies of the broadcast forms (what a caller has to build without the strided call)
        rep_src = one_src.repeat(batch)
        rep_smp = one_smp.repeat(batch)
        rec = d_src[:(batch + 1) * n].clone()
        win_src = torch.cat([rec[k * n:k * n + 2 * n] for k in range(batch)])
        lag = torch.empty(batch, dtype=torch.int64, device="cuda")
        coef = torch.empty(batch, dtype=torch.float64, device="cuda")
        ret = torch.empty(batch, dtype=torch.int32, device="cuda")
        res = {"N": n, "batch": batch, "runs": a.runs}
        with asx.Plan(n, batch, 0) as plan:
            st = torch.cuda.Stream()
            sp = st.cuda_stream

            def rate(fn):
                with torch.cuda.stream(st):
                    for _ in range(a.warmup):
                        fn()
                    times = []
                    for _ in range(a.runs):
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        fn()
                        e1.record(st)
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1))
                times.sort()
                ms = times[len(times) // 2]
                return round(batch / (ms / 1e3), 1), round(ms, 4)

            def contig(s, m):
                return lambda: plan.xcorr_batch_dev(s.data_ptr(), m.data_ptr(), batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)

            def strided(s, ss, m, ms):
                return lambda: plan.xcorr_strided_dev(s.data_ptr(), ss, m.data_ptr(), ms, batch, lag.data_ptr(), coef.data_ptr(),
                                                      ret.data_ptr(), sp)

            for name, fn in (("contiguous", contig(d_src, d_smp)),
                             ("contiguous_bcast_source_copies", contig(rep_src, d_smp)),
                             ("bcast_source", strided(one_src, 0, d_smp, n)),
                             ("contiguous_bcast_sample_copies", contig(d_src, rep_smp)),
                             ("bcast_sample", strided(d_src, 2 * n, one_smp, 0)),
                             ("contiguous_window_copies", contig(win_src, rep_smp)),
                             ("windows", strided(rec, n, one_smp, 0))):
                res[name + "_pairs_per_s"], res[name + "_ms"] = rate(fn)
            res["layout"] = plan.layout
        print(json.dumps(res), flush=True)
        lines.append(res)
        del d_src, d_smp, rep_src, rep_smp, rec, win_src
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
