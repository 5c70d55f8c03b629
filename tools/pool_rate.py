#!/usr/bin/env python3
"""Pairs per second of the pool call (asx_xcorr_pool_f32_dev) against the two ways a caller had before it: R strided calls that each
broadcast one sample against all S sources, and the contiguous call on materialised copies of every pair.

    python3 tools/pool_rate.py [--runs 7] [--warmup 2] [--cases 1440000:124x4,...] [--allpairs 480000:32] [--only FORMS] [--out FILE]

Cases N:SxR are S sources of 2N frames against R samples of N frames, every combination (S x R pairs); the samples are cuts of the
sources at planted lags, so every sample matches one source.  --allpairs N:C is one pool of C clips of 2N frames cut from one long
recording (consecutive clips overlap by half, so most pairs match), correlated all against all: the pool call with the list of the
C (C - 1) ordered pairs a != b ("pool_list"), the pool call over every combination ("pool", C x C), C broadcast calls of C pairs and
the contiguous call on C x C copies.  Forms:
  pool         one asx_xcorr_pool_f32_dev call
  bcast        R calls of asx_xcorr_strided_f32_dev, sample stride 0 (the best strided form: one sample against many sources)
  contiguous   asx_xcorr_batch_f32_dev on S x R materialised pairs (the copies are made once, outside the timing)
HIP events around each call (the plan's exact mode, as a caller runs it: one host synchronisation per strided call), the forms
ALTERNATING within each of --runs rounds; reported are the medians and pairs per second of the pairs each form computes.
--only pool,bcast runs just those forms: the kernels of one form then show alone in a kernel trace
(rocprofv3 --kernel-trace --stats -- python3 tools/pool_rate.py --only pool --runs 3).  Prints one JSON line per case."""
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
    ap.add_argument("--cases", default="1440000:124x4,1440000:124x16,480000:256x4")
    ap.add_argument("--allpairs", default="480000:32", help="N:C, or '' for none")
    ap.add_argument("--only", default="pool,pool_list,bcast,contiguous")
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
            rec = torch.from_numpy(rng.standard_normal(2 * n * (c + 1) // 2 + 2 * n).astype(np.float32)).cuda()
            src = torch.stack([rec[k * n:k * n + 2 * n] for k in range(c)]).contiguous()      # clip k starts at k N: half overlaps
            smp = src[:, :n].contiguous()
        else:
            n, sr = case.split(":")
            n = int(n)
            S, R = (int(v) for v in sr.split("x"))
            src = torch.from_numpy(rng.standard_normal((S, 2 * n)).astype(np.float32)).cuda()
            rows = []
            for b in range(R):
                a_, lag = int(rng.integers(S)), int(rng.integers(-n, n))
                idx = torch.from_numpy((np.arange(n) + lag % (2 * n)) % (2 * n)).cuda()
                rows.append(src[a_, idx] + 0.1 * torch.randn(n, device="cuda"))
            smp = torch.stack(rows).contiguous()
        batch = S * R
        lag = torch.empty(batch, dtype=torch.int64, device="cuda")
        coef = torch.empty(batch, dtype=torch.float64, device="cuda")
        ret = torch.empty(batch, dtype=torch.int32, device="cuda")
        plist = torch.tensor([[x, y] for x in range(S) for y in range(R) if x != y], dtype=torch.int32, device="cuda")
        rep_src = src.repeat_interleave(R, dim=0).contiguous() if "contiguous" in only else None   # pair (a, b) at a R + b
        rep_smp = smp.repeat(S, 1).contiguous() if "contiguous" in only else None
        torch.cuda.synchronize()
        res = {"N": n, "sources": S, "samples": R, "pairs": batch, "runs": a.runs, "allpairs": allpairs}
        with asx.Plan(n, min(batch, 1024), 0) as plan:
            st = torch.cuda.Stream()
            sp = st.cuda_stream
            forms = {}
            if "pool" in only:
                forms["pool"] = (batch, lambda: plan.xcorr_pool_dev(src.data_ptr(), 2 * n, S, smp.data_ptr(), n, R, 0, 0, 0, batch,
                                                                    lag.data_ptr(), coef.data_ptr(), ret.data_ptr(), sp))
            if "pool_list" in only and allpairs:
                forms["pool_list"] = (plist.shape[0], lambda: plan.xcorr_pool_dev(src.data_ptr(), 2 * n, S, smp.data_ptr(), n, R,
                                                                                  plist.data_ptr(), 0, 0, plist.shape[0], lag.data_ptr(),
                                                                                  coef.data_ptr(), ret.data_ptr(), sp))
            if "bcast" in only:
                def bcast():
                    for b in range(R):   # results of sample b at b S .. b S + S - 1 (sample-major)
                        plan.xcorr_strided_dev(src.data_ptr(), 2 * n, smp[b].data_ptr(), 0, S, lag[b * S:].data_ptr(),
                                               coef[b * S:].data_ptr(), ret[b * S:].data_ptr(), sp)
                forms["bcast"] = (batch, bcast)
            if "contiguous" in only:
                forms["contiguous"] = (batch, lambda: plan.xcorr_batch_dev(rep_src.data_ptr(), rep_smp.data_ptr(), batch, lag.data_ptr(),
                                                                           coef.data_ptr(), ret.data_ptr(), sp))
            times = {k: [] for k in forms}
            with torch.cuda.stream(st):
                for k, (_, fn) in forms.items():
                    for _ in range(a.warmup):
                        fn()
                for _ in range(a.runs):
                    for k, (_, fn) in forms.items():
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        fn()
                        e1.record(st)
                        e1.synchronize()
                        times[k].append(e0.elapsed_time(e1))
            for k, (pairs, _) in forms.items():
                t = sorted(times[k])
                ms = t[len(t) // 2]
                res[k + "_ms"] = round(ms, 3)
                res[k + "_pairs_per_s"] = round(pairs / (ms / 1e3), 1)
            res["layout"] = plan.layout
            res["bank_tracks"] = plan.debug_bank()[:2]
        print(json.dumps(res), flush=True)
        lines.append(res)
        del src, smp, rep_src, rep_smp
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
