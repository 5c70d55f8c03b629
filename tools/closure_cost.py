#!/usr/bin/env python3
"""What triangle closure over a clip pool (asx_pool_closure_dev: k_closure_votes, k_closure_confirm, k_closure_root,
k_closure_offsets) costs, next to the pool top-k call that produces its input.

    python3 tools/closure_cost.py [--shapes 16x4,64x8,256x8] [--runs 21] [--warmup 3] [--n 144000] [--out FILE]

Per shape C x k a synthetic device-resident table: clip offsets T, per ordered pair the true lag T_b - T_a with +-1 frame of jitter
at a random entry and random decoys with the higher coefficient in the others, the diagonal as the pool call returns it.  The call
runs with tolerance 2, min_confirm 1 and a chosen root, with and without d_votes, ALTERNATING within each of --runs rounds, each
between two events on the stream.  Then, in the same process, the call that produces a 16 x 16 x 4 table: asx_xcorr_pool_topk_f32_dev
over one pool of 16 clips of 2N frames as both sides (k = 4, min_separation 1000), --runs times between two events.
Prints median, minimum and maximum in milliseconds, and appends the same text to --out."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def synthetic(C, k, seed):
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 100000, size=C)
    true = (T[None, :] - T[:, None]).astype(np.int64)
    lag = rng.integers(-200000, 200000, size=(C, C, k)).astype(np.int64)
    coef = rng.uniform(0.6, 0.9, size=(C, C, k))
    j = rng.integers(0, k, size=(C, C, 1))
    np.put_along_axis(lag, j, (true + rng.integers(-1, 2, size=(C, C)))[:, :, None], axis=2)
    np.put_along_axis(coef, j, rng.uniform(0.3, 0.5, size=(C, C, 1)), axis=2)
    d = np.arange(C)
    lag[d, d, 0], coef[d, d, 0] = 0, 1.0
    return lag, coef, np.zeros((C, C, k), dtype=np.int32), true


def timed(torch, st, calls, runs, warmup):
    times = {name: [] for name in calls}
    for run in range(warmup + runs):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            if run >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x4,64x8,256x8")
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    lines = ["asx_pool_closure_dev, tolerance 2, min_confirm 1, root chosen, %d alternating calls, %s" % (a.runs, torch.cuda.get_device_name(0))]
    with torch.cuda.stream(st):
        for shape in a.shapes.split(","):
            C, k = (int(v) for v in shape.split("x"))
            lag, coef, ret, true = synthetic(C, k, 2024)
            d_in = [torch.from_numpy(x).cuda() for x in (lag, coef, ret)]
            i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")      # noqa: E731
            i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")      # noqa: E731
            votes, best_lag, best_coef = i32(C * C * k), i64(C * C), torch.zeros(C * C, dtype=torch.float64, device="cuda")
            best_ret, best_entry, confirm, root = i32(C * C), i32(C * C), i32(C * C), i32(1)
            offset, support, placed = i64(C), i32(C), i32(C)
            torch.cuda.synchronize()

            def closure(with_votes):
                asx.pool_closure_dev(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), C, k, 2, 1, -1, best_lag.data_ptr(),
                                     best_coef.data_ptr(), best_ret.data_ptr(), best_entry.data_ptr(), confirm.data_ptr(),
                                     root.data_ptr(), offset.data_ptr(), support.data_ptr(), placed.data_ptr(),
                                     d_votes=votes.data_ptr() if with_votes else 0, stream=sp)

            times = timed(torch, st, {"votes": lambda: closure(True), "no votes": lambda: closure(False)}, a.runs, a.warmup)
            st.synchronize()
            got = best_lag.cpu().numpy().reshape(C, C)
            off = ~np.eye(C, dtype=bool)
            assert (np.abs(got - true)[off] <= 1).all() and placed.cpu().numpy().all(), "the picks are not the planted lags"
            r = int(root.cpu()[0])
            assert (np.abs(offset.cpu().numpy() - true[r]) <= 2).all(), "the clips are not at their offsets"
            for name, v in times.items():
                v = sorted(v)
                lines.append("  C = %3d, k = %d, %-8s median %9.4f  min %9.4f  max %9.4f ms" % (C, k, name, v[len(v) // 2], v[0], v[-1]))
        # the producer of a 16 x 16 x 4 table
        n, C, k = a.n, 16, 4
        with asx.Plan(n, C * C, 0) as plan:
            gen = torch.Generator(device="cuda").manual_seed(2024)
            rec = torch.randn(2 * n + 15 * 4000, dtype=torch.float32, device="cuda", generator=gen)
            clips = torch.stack([rec[4000 * i:4000 * i + 2 * n] for i in range(C)]).contiguous()
            lag, coef, ret = (torch.zeros(C * C * k, dtype=torch.int64, device="cuda"),
                              torch.zeros(C * C * k, dtype=torch.float64, device="cuda"),
                              torch.zeros(C * C * k, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()

            def topk():
                plan.xcorr_pool_topk_dev(clips.data_ptr(), 2 * n, C, clips.data_ptr(), 2 * n, C, 0, 0, 0, C * C, k, 1000, lag.data_ptr(),
                                         coef.data_ptr(), ret.data_ptr(), sp)

            v = sorted(timed(torch, st, {"topk": topk}, a.runs, a.warmup)["topk"])
            plan.sync(sp)
            got = lag.cpu().numpy().reshape(C, C, k)[:, :, 0]
            assert (got == 4000 * (np.arange(C)[None, :] - np.arange(C)[:, None])).all(), "the producer's lags are not the planted ones"
        lines.append("  asx_xcorr_pool_topk_f32_dev, N = %d, 16 clips as both pools, k = 4 (the producer of a 16 x 16 x 4 table): "
                     "median %9.4f  min %9.4f  max %9.4f ms" % (n, v[len(v) // 2], v[0], v[-1]))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
