#!/usr/bin/env python3
"""Pairs per second of top-k over pools (asx_xcorr_pool_topk_f32_dev) against what a caller had to do before it: one
asx_xcorr_topk_f32_dev call per source, that source broadcast (stride 0) over the sample pool.

    python3 tools/pool_topk_rate.py [--runs 7] [--warmup 2] [--topk 2,4] [--sep 4800] [--cases 1440000:124x4,480000:256x4]
                                    [--allpairs 480000:32] [--only FORMS] [--out FILE]

Cases N:SxR are S sources of 2N frames against R samples of N frames, every combination (S x R pairs).  Every sample is a cut of one
source at a planted lag plus a weaker copy (0.6) of the same source at a second lag (the decoy construction of tools/topk_rate.py),
so each related pair has a real second peak; the unrelated pairs' entries are all at the noise floor, where the exact
re-evaluation dominates every form alike.  --allpairs N:C is one pool of C clips of 2N frames cut from one long recording that
repeats itself (the recording plus 0.6 of itself --sep + 5000 frames later; consecutive clips overlap by half), all against all.
Forms, for each k of --topk:
  pool_topk    one asx_xcorr_pool_topk_f32_dev call (every track transformed once, whatever k is)
  bcast_topk   S calls of asx_xcorr_topk_f32_dev, source stride 0, over the R samples (each call transforms the sample pool again)
HIP events around each form (the plan's exact mode, as a caller runs it: one host synchronisation per call), the forms ALTERNATING
within each of --runs rounds; reported are the medians, the pairs per second and the ratio.  Both forms must return the same bytes;
the line says whether they did.  --only pool_topk runs just that form: its kernels then show alone in a kernel trace
(rocprofv3 --kernel-trace --stats -- python3 tools/pool_topk_rate.py --only pool_topk --runs 3), where k_pearson_prep_xl stands
beside the k_pearson_prep_x of --only bcast_topk.  Prints one JSON line per case and k."""
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
    ap.add_argument("--topk", default="2,4")
    ap.add_argument("--sep", type=int, default=4800)
    ap.add_argument("--cases", default="1440000:124x4,480000:256x4")
    ap.add_argument("--allpairs", default="480000:32", help="N:C, or '' for none")
    ap.add_argument("--only", default="pool_topk,bcast_topk")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    asx = graft.load()
    only = set(a.only.split(","))
    cases = [(c, False) for c in a.cases.split(",") if c] + ([(a.allpairs, True)] if a.allpairs else [])
    lines = []
    for case, allpairs in cases:
        rng = np.random.default_rng(2024)
        if allpairs:
            n, c = (int(v) for v in case.split(":"))
            S = R = c
            d = a.sep + 5000
            rec = torch.from_numpy(rng.standard_normal(2 * n * (c + 1) // 2 + 2 * n + d).astype(np.float32)).cuda()
            rec = rec[d:] + 0.6 * rec[:-d]                                                    # every passage comes again d frames later
            src = torch.stack([rec[k * n:k * n + 2 * n] for k in range(c)]).contiguous()      # clip k starts at k N: half overlaps
            smp = src[:, :n].contiguous()
        else:
            n, sr = case.split(":")
            n = int(n)
            S, R = (int(v) for v in sr.split("x"))
            src = torch.from_numpy(rng.standard_normal((S, 2 * n)).astype(np.float32)).cuda()
            rows = []
            for b in range(R):
                a_, lag = int(rng.integers(S)), int(rng.integers(-n // 2, n // 2))
                second = lag + (2 * a.sep + 3000) * (1 if lag < 0 else -1)
                i1 = torch.from_numpy((np.arange(n) + lag % (2 * n)) % (2 * n)).cuda()
                i2 = torch.from_numpy((np.arange(n) + second % (2 * n)) % (2 * n)).cuda()
                rows.append(src[a_, i1] + 0.6 * src[a_, i2] + 0.1 * torch.randn(n, device="cuda"))
            smp = torch.stack(rows).contiguous()
        batch = S * R
        torch.cuda.synchronize()
        with asx.Plan(n, min(batch, 1024), 0) as plan:
            st = torch.cuda.Stream()
            sp = st.cuda_stream
            for k in (int(v) for v in a.topk.split(",")):
                out = {f: (torch.zeros(batch * k, dtype=torch.int64, device="cuda"), torch.zeros(batch * k, dtype=torch.float64, device="cuda"),
                           torch.zeros(batch * k, dtype=torch.int32, device="cuda")) for f in ("pool_topk", "bcast_topk")}
                res = {"N": n, "sources": S, "samples": R, "pairs": batch, "k": k, "sep": a.sep, "runs": a.runs, "allpairs": allpairs}

                def pool_topk(k=k):
                    lag, coef, ret = out["pool_topk"]
                    plan.xcorr_pool_topk_dev(src.data_ptr(), 2 * n, S, smp.data_ptr(), n, R, 0, 0, 0, batch, k, a.sep, lag.data_ptr(),
                                             coef.data_ptr(), ret.data_ptr(), sp)

                def bcast_topk(k=k):
                    lag, coef, ret = out["bcast_topk"]
                    for s in range(S):   # results of source s at s R k .. (source-major, as the pool call's)
                        o = s * R * k
                        plan.xcorr_topk_dev(src[s].data_ptr(), 0, smp.data_ptr(), n, 0, 0, R, k, a.sep, lag[o:].data_ptr(),
                                            coef[o:].data_ptr(), ret[o:].data_ptr(), sp)

                forms = {f: fn for f, fn in (("pool_topk", pool_topk), ("bcast_topk", bcast_topk)) if f in only}
                times = {f: [] for f in forms}
                with torch.cuda.stream(st):
                    for fn in forms.values():
                        for _ in range(a.warmup):
                            fn()
                    for _ in range(a.runs):
                        for f, fn in forms.items():
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record(st)
                            fn()
                            e1.record(st)
                            e1.synchronize()
                            times[f].append(e0.elapsed_time(e1))
                torch.cuda.synchronize()
                for f in forms:
                    t = sorted(times[f])
                    ms = t[len(t) // 2]
                    res[f + "_ms"] = round(ms, 3)
                    res[f + "_pairs_per_s"] = round(batch / (ms / 1e3), 1)
                if len(forms) == 2:
                    res["pool_over_bcast"] = round(res["bcast_topk_ms"] / res["pool_topk_ms"], 3)
                    res["same_bytes"] = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                                        y.view(torch.int64) if y.dtype == torch.float64 else y)
                                            for x, y in zip(out["pool_topk"], out["bcast_topk"]))
                lag, coef, ret = out["pool_topk" if "pool_topk" in forms else "bcast_topk"]
                good = (ret.view(batch, k) == 0) & (coef.view(batch, k) > 0.2)
                res["pairs_with_two_peaks"] = int((good.sum(dim=1) >= 2).sum()) if k >= 2 else 0
                res["layout"] = plan.layout
                res["overflows"] = plan.peak_overflows()
                print(json.dumps(res), flush=True)
                lines.append(res)
        del src, smp
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
