#!/usr/bin/env python3
"""What the top-k peaks (asx_xcorr_topk_f32_dev) cost against the plain strided call: pairs per second of asx_xcorr_strided_f32_dev
and of asx_xcorr_topk_f32_dev with k = 1, 2 and 4, on two kinds of pairs:

    synth   asx_synth_pairs_dev pairs: one true peak, so entries 2.. are runner-ups at the noise floor (long near-tie lists)
    decoy   a copy of the same pairs with a second copy of the source added to the sample at lag N/3 (0.7 times as strong): entry 2
            is that copy, entries 3.. the noise floor

    python3 tools/topk_rate.py [--runs 9] [--reps 4] [--cases 1440000x124,480000x1024] [--sep 4800] [--out FILE]

Device time: the plan runs in the asynchronous mode (asx_plan_set_exact(plan, 0): no host synchronisation inside a call) with
profiling off, and --reps calls of one kind are timed back to back between two HIP events, so the events see the kernels and not
the host.  The kinds ALTERNATE (strided, k = 1, k = 2, k = 4, strided, ...; --order, a permutation of 0,1,2,4) so that clock drift
falls on all; reported are the median over --runs rounds of the time per call, the cost of one further pass ((t_k - t_1) / (k - 1)),
whether k = 1 returned the strided call's bits, and how many entries came back marked inexact (ret = 1: the exact mode would have
taken the second look at them).  The kernels of each pass (k_inv_cols_r<..., AsxSelTopk<ZC>> and the tail) show by name in a kernel trace of the same
run (tools/README.md).  Prints one JSON line per length and kind of pair (and writes them to --out)."""
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
    ap.add_argument("--reps", type=int, default=4, help="calls of one kind between two events")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="1440000x124,480000x1024")
    ap.add_argument("--sep", type=int, default=4800, help="min_separation in frames (default 0.1 s at 48 kHz)")
    ap.add_argument("--kinds", default="synth,decoy")
    ap.add_argument("--order", default="0,1,2,4", help="the alternation: 0 = the strided call, else k (1, 2 and 4 must appear)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    order = tuple(int(v) for v in a.order.split(","))
    if sorted(order) != [0, 1, 2, 4]:
        ap.error("--order must be a permutation of 0,1,2,4, not %s" % a.order)
    import torch
    asx = graft.load()
    lines = []
    for case in a.cases.split(","):
        n, batch = (int(v) for v in case.split("x"))
        d_src = torch.empty(batch * 2 * n, dtype=torch.float32, device="cuda")
        d_smp = torch.empty(batch * n, dtype=torch.float32, device="cuda")
        asx.synth_pairs_dev(2024, 0, batch, n, 1, d_src.data_ptr(), d_smp.data_ptr())
        torch.cuda.synchronize()
        for kind in a.kinds.split(","):
            smp = d_smp
            if kind == "decoy":
                d = n // 3
                smp = d_smp.clone()
                smp.view(batch, n).add_(0.7 * d_src.view(batch, 2 * n)[:, d:d + n])
                torch.cuda.synchronize()
            ks = (1, 2, 4)
            outs = {k: tuple(torch.empty(batch * max(k, 1), dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.int32))
                    for k in (0,) + ks}  # (0: the strided call)
            with asx.Plan(n, batch, 0) as plan:
                st = torch.cuda.Stream()
                sp = st.cuda_stream
                plan.set_exact(False)

                def call(k):
                    lag, coef, ret = (t.data_ptr() for t in outs[k])
                    if k == 0:
                        plan.xcorr_strided_dev(d_src.data_ptr(), 2 * n, smp.data_ptr(), n, batch, lag, coef, ret, sp)
                    else:
                        plan.xcorr_topk_dev(d_src.data_ptr(), 2 * n, smp.data_ptr(), n, 0, 0, batch, k, a.sep, lag, coef, ret, sp)

                times = {k: [] for k in order}
                with torch.cuda.stream(st):
                    for _ in range(a.warmup):
                        for k in order:
                            call(k)
                    for _ in range(a.runs):
                        for k in order:
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            for _ in range(a.reps):
                                call(k)
                            e1.record(st)
                            e1.synchronize()
                            times[k].append(e0.elapsed_time(e1) / a.reps)
                torch.cuda.synchronize()
                ms = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
                same = all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(outs[0], outs[1]))
                ret4 = outs[4][2].view(batch, 4).cpu().numpy()
                lag4 = outs[4][0].view(batch, 4).cpu().numpy()
                res = {"N": n, "batch": batch, "kind": kind, "layout": plan.layout, "runs": a.runs, "reps": a.reps, "sep": a.sep,
                       "mode": "asynchronous, profiling off",
                       "strided_ms": round(ms[0], 4), "strided_pairs_per_s": round(batch / (ms[0] / 1e3), 1),
                       "topk_ms": {str(k): round(ms[k], 4) for k in ks},
                       "topk_pairs_per_s": {str(k): round(batch / (ms[k] / 1e3), 1) for k in ks},
                       "k1_over_strided": round(ms[1] / ms[0], 4),
                       "per_further_pass_ms": {str(k): round((ms[k] - ms[1]) / (k - 1), 4) for k in ks if k > 1},
                       "spread_ms": {str(k): round(max(v) - min(v), 4) for k, v in times.items()},
                       "k1_same_bits_as_strided": bool(same),
                       "k4_entries_ok": int((ret4 == 0).sum()), "k4_entries": int(ret4.size), "k4_inexact": int((ret4 == 1).sum()),
                       "k4_entry2_at_decoy": int((lag4[:, 1] == n // 3).sum()) if kind == "decoy" else None}
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
