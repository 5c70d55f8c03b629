#!/usr/bin/env python3
"""What a further entry of the PHAT top-k calls costs (asx_xcorr_phat_topk_f32_dev, asx_xcorr_pool_phat_topk_f32_dev), next to the
calls they extend and to the raw top-k call.

    python3 tools/phat_topk_cost.py [--runs 9] [--reps 4] [--cases 1440000x124,144000x1024] [--pool 16] [--sep 4800]
                                    [--band LO HI] [--lib FILE] [--out FILE]

Strided part, per case NxB: one group of B generator pairs with a second copy of the source in the sample at lag N/3, 0.7 times as
strong (the `decoy` pairs of tools/topk_rate.py), so the first two entries of either ranking are real peaks (the added copy, which
carries no noise, then the generator's planted lag) and entries 3.. are not.  Kinds: band (asx_xcorr_phat_band_f32_dev), p1 / p2 / p4 (the PHAT top-k call with k = 1, 2, 4), raw2 (asx_xcorr_topk_f32_dev,
k = 2), raw1 (k = 1).  Pool part (--pool C, 0 = none), at each case's N: C clips of one recording 1000 frames apart as both pools,
all C * C pairs: pool (asx_xcorr_pool_phat_f32_dev), q1 / q2 / q4 (the pool PHAT top-k call).

Device time as tools/topk_rate.py takes it: the asynchronous mode (asx_plan_set_exact(plan, 0)), profiling off, --reps calls of one
kind back to back between two HIP events; the kinds ALTERNATE within each of --runs rounds; reported are the medians per call, the
cost of one further pass ((t_k - t_1) / (k - 1)) and each kind's spread.  --lib FILE loads another build's libaudiosync_hip.so (the
parent commit's, for the comparison of the calls both builds have): the kinds that library lacks are left out.  Prints one JSON
line per case and part (and writes them to --out)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def timed(torch, st, calls, runs, reps, warmup):
    """{kind: [ms per call, one per round]}: the kinds alternate within a round"""
    times = {k: [] for k in calls}
    with torch.cuda.stream(st):
        for _ in range(warmup):
            for fn in calls.values():
                fn()
        for _ in range(runs):
            for k, fn in calls.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(reps):
                    fn()
                e1.record(st)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps)
    torch.cuda.synchronize()
    return times


def summary(times):
    ms = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return ms, {"ms": {k: round(v, 4) for k, v in ms.items()},
                "spread_ms": {k: round(max(v) - min(v), 4) for k, v in times.items()}}


def further(ms, one, more):
    return {k: round((ms[k] - ms[one]) / (int(k[1:]) - 1), 4) for k in more if k in ms and one in ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=4, help="calls of one kind between two events")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="1440000x124,144000x1024")
    ap.add_argument("--pool", type=int, default=16, help="clips of the pool part (0: none)")
    ap.add_argument("--sep", type=int, default=4800, help="min_separation in frames (default 0.1 s at 48 kHz)")
    ap.add_argument("--band", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="default 1 .. N/6")
    ap.add_argument("--lib", default=None, help="another build's libaudiosync_hip.so")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    from audiosync_amd import hipxcorr
    if a.lib:
        probe = ctypes.CDLL(os.path.abspath(a.lib))
        for name in [s for s in hipxcorr.SIGNATURES if not hasattr(probe, s)]:
            del hipxcorr.SIGNATURES[name]
        hipxcorr.LIB_PATH = os.path.abspath(a.lib)
    have_new = "asx_xcorr_phat_topk_f32_dev" in hipxcorr.SIGNATURES
    lines = []
    for case in a.cases.split(","):
        n, batch = (int(v) for v in case.split("x"))
        lo, hi = a.band if a.band else (1, n // 6)
        d_src = torch.empty(batch * 2 * n, dtype=torch.float32, device="cuda")
        d_smp = torch.empty(batch * n, dtype=torch.float32, device="cuda")
        asx.synth_pairs_dev(2024, 0, batch, n, 1, d_src.data_ptr(), d_smp.data_ptr())
        d = n // 3
        d_smp.view(batch, n).add_(0.7 * d_src.view(batch, 2 * n)[:, d:d + n])
        torch.cuda.synchronize()
        out = tuple(torch.empty(batch * 4, dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.float64, torch.int32))
        lag, coef, peak, ret = (t.data_ptr() for t in out)
        st = torch.cuda.Stream()
        sp = st.cuda_stream
        with asx.Plan(n, batch, 0) as plan:
            assert plan.group >= batch, (plan.group, batch)
            plan.set_exact(False)
            src, smp = d_src.data_ptr(), d_smp.data_ptr()
            calls = {"band": lambda: plan.xcorr_phat_band_dev(src, 2 * n, smp, n, 0, 0, batch, lo, hi, lag, coef, peak, ret, sp)}
            if have_new:
                for k in (1, 2, 4):
                    calls["p%d" % k] = (lambda k=k: plan.xcorr_phat_topk_dev(src, 2 * n, smp, n, 0, 0, batch, lo, hi, k, a.sep, lag, coef,
                                                                            peak, ret, sp))
            for k in (1, 2):
                calls["raw%d" % k] = lambda k=k: plan.xcorr_topk_dev(src, 2 * n, smp, n, 0, 0, batch, k, a.sep, lag, coef, ret, sp)
            ms, res = summary(timed(torch, st, calls, a.runs, a.reps, a.warmup))
            res.update({"part": "strided", "N": n, "batch": batch, "band": [lo, hi], "sep": a.sep, "runs": a.runs, "reps": a.reps,
                        "layout": plan.layout, "lib": a.lib or "this build", "mode": "asynchronous, profiling off",
                        "per_further_pass_ms": dict(further(ms, "p1", ("p2", "p4")), raw2=round(ms["raw2"] - ms["raw1"], 4))})
            if have_new:
                calls["p4"]()
                plan.sync(sp)
                l4 = out[0].view(batch, 4).cpu().numpy()
                p4 = out[2].view(batch, 4).cpu().numpy()
                res["p4_entry1_at_copy"] = int((l4[:, 0] == d).sum())     # the added copy carries no noise: it ranks first
                res["p4_peaks_of_the_median_pair"] = [round(float(v), 4) for v in sorted(p4.tolist())[batch // 2]]
            print(json.dumps(res), flush=True)
            lines.append(res)
        del d_src, d_smp
        torch.cuda.empty_cache()
        C = a.pool
        if C:
            hop = 1000
            rec = torch.randn(2 * n + (C - 1) * hop, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            pout = tuple(torch.empty(C * C * 4, dtype=dt, device="cuda") for dt in (torch.int64, torch.float64, torch.float64, torch.int32))
            lag, coef, peak, ret = (t.data_ptr() for t in pout)
            with asx.Plan(n, C * C, 0) as plan:
                plan.set_exact(False)
                group = plan.group
                r = rec.data_ptr()
                calls = {"pool": lambda: plan.xcorr_pool_phat_dev(r, hop, C, r, hop, C, 0, 0, 0, C * C, lo, hi, lag, coef, peak, ret, sp)}
                if have_new:
                    for k in (1, 2, 4):
                        calls["q%d" % k] = (lambda k=k: plan.xcorr_pool_phat_topk_dev(r, hop, C, r, hop, C, 0, 0, 0, C * C, lo, hi, k, a.sep,
                                                                                     lag, coef, peak, ret, sp))
                calls["pool"]()                       # the bank's first allocation, outside the timed calls
                plan.sync(sp)
                ms, res = summary(timed(torch, st, calls, a.runs, a.reps, a.warmup))
                res.update({"part": "pool", "N": n, "clips": C, "pairs": C * C, "group": group, "band": [lo, hi], "sep": a.sep, "runs": a.runs,
                            "reps": a.reps, "lib": a.lib or "this build", "per_further_pass_ms": further(ms, "q1", ("q2", "q4"))})
                print(json.dumps(res), flush=True)
                lines.append(res)
            del rec
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
