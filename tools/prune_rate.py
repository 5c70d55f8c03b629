#!/usr/bin/env python3
"""What the pruned inverse column pass (asx_plan_set_prune) costs where it can skip nothing, and what it saves where it can.

    python3 tools/prune_rate.py [--runs 7] [--warmup 2] [--cases 1440000x124,480000x1024,144000x1024] [--out FILE]

Per length, on ONE plan, pruning on and off ALTERNATING run by run (HIP events around one device-resident batch call, median of
--runs each), for two kinds of input:
  unrelated   independent Gaussian noise in both tracks: no tile's bound lies under the window of the running maximum, every tile
              is transformed -- the row pass's extra work and the two small kernels are pure cost
  generator   the bench's pairs (a planted delay): one or two tiles per pair are transformed
and, with the plan's kernel events (asx_plan_set_profiling, on for every timed call both ways), the row family and the inverse
family of each of those calls: median and range per setting, so that the two can be told apart beyond run-to-run spread.
Prints one JSON line per length (and writes them to --out).

Measured (profiles/r7_prune/prune_rate.jsonl, EXPERIMENTS.md round 7): unrelated tracks are 3.2 % slower with pruning on at
N = 1 440 000 x 124 (5.179 -> 5.343 ms per call; inverse family 0.337 [0.321, 0.348] -> 0.398 [0.391, 0.403] ms), 3.1 % at 480 000,
5.3 % at 144 000.  That is MORE than the row pass's extra work plus the two small kernels (0.037 ms of the family's +0.061): the first
launch of the pruned pass is a generation of its own (22 us).  The second launch, 0.339 ms for 148 of 150 tiles, is inside the spread
of k_inv_cols_r's 0.337 for all 150.  Generator pairs: 2.286 -> 2.201 ms per call."""
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
    ap.add_argument("--cases", default="1440000x124,480000x1024,144000x1024")
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
        lag = torch.empty(batch, dtype=torch.int64, device="cuda")
        coef = torch.empty(batch, dtype=torch.float64, device="cuda")
        ret = torch.empty(batch, dtype=torch.int32, device="cuda")
        res = {"N": n, "batch": batch, "runs": a.runs}
        with asx.Plan(n, batch, 0) as plan:
            plan.set_exact(False)  # no host synchronisation inside the timed call
            st = torch.cuda.Stream()
            sp = st.cuda_stream

            def call():
                plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp)

            def timed():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for kind in ("unrelated", "generator"):
                if kind == "unrelated":
                    g = torch.Generator(device="cuda")
                    g.manual_seed(n)
                    d_src.normal_(generator=g)
                    d_smp.normal_(generator=g)
                else:
                    asx.synth_pairs_dev(20260101, 0, batch, n, 1, d_src.data_ptr(), d_smp.data_ptr(), d_lag.data_ptr())
                torch.cuda.synchronize()
                times = {True: [], False: []}
                fam = {(on, k): [] for on in (True, False) for k in ("rows", "inv_cols")}
                plan.set_profiling(1)
                with torch.cuda.stream(st):
                    for on in (True, False):
                        plan.set_prune(on)
                        for _ in range(a.warmup):
                            call()
                    for _ in range(a.runs):
                        for on in (True, False):
                            plan.set_prune(on)
                            times[on].append(timed())
                            t = plan.last_timings_ms()
                            for k in ("rows", "inv_cols"):
                                fam[(on, k)].append(t[k])
                    # the tiles one pruned call transforms
                    plan.set_prune(True)
                    before = plan.prune_stats()
                    call()
                    plan.sync(sp)
                    after = plan.prune_stats()
                    res[kind + "_tiles_transformed"] = after[0] - before[0]
                    res[kind + "_tiles_total"] = after[1] - before[1]
                plan.set_profiling(0)
                for on in (True, False):
                    tag = "%s_%s" % (kind, "on" if on else "off")
                    for name, v in (("", sorted(times[on])), ("_rows", sorted(fam[(on, "rows")])), ("_inv_cols", sorted(fam[(on, "inv_cols")]))):
                        res[tag + name + "_ms"] = round(v[len(v) // 2], 4)
                        res[tag + name + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
            res["layout"] = plan.layout
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
