#!/usr/bin/env python3
"""What placement over chains of usable pairs (asx_pool_place_dev: k_place_init, k_place_layer, k_place_sweep, k_place_verdict) costs,
next to triangle closure on the same tables and to the pool top-k call that produces such tables.

    python3 tools/place_cost.py [--shapes 16:1,64:10,256:40,256:1] [--runs 21] [--warmup 3] [--n 144000] [--out FILE]

Per shape C:H a synthetic device-resident [C, C, 2] table of one long event: clips `spacing` apart, the true lag with +-1 frame of
jitter (and a decoy with the higher coefficient) between clips less than `reach` apart, (0, NaN, -3) between the others; the spacing is
chosen so that the clip that starts first is about H hops from the one that starts last, and that clip is the root.  Closure (tolerance
4, min_confirm 1, that root) and placement behind it (max_hops 64, sweeps 0 and 3, closure's d_root) run ALTERNATING within each of
--runs rounds, each between two events on the stream; the hops that placement needed are read back.  An empty layer: placement with
max_hops 1024 against max_hops 64 on the same table, the difference over 960 launches.  Then, in the same process, the call that
produces a 16 x 16 x 4 table, as tools/closure_cost.py times it.
Prints median, minimum and maximum in milliseconds, and appends the same text to --out."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

REACH = 100000


def band(C, hops, seed, k=2):
    rng = np.random.default_rng(seed)
    spacing = max(1, int(REACH * hops * 0.8 / C))
    T = spacing * np.arange(C, dtype=np.int64) + rng.integers(-(spacing // 10), spacing // 10 + 1, size=C)
    T = T[rng.permutation(C)]
    true = T[None, :] - T[:, None]
    inside = (np.abs(true) < REACH) & ~np.eye(C, dtype=bool)
    lag = rng.integers(-REACH, REACH, size=(C, C, k)).astype(np.int64)
    coef = rng.uniform(0.6, 0.9, size=(C, C, k))
    ret = np.zeros((C, C, k), dtype=np.int32)
    j = rng.integers(0, k, size=(C, C, 1))
    np.put_along_axis(lag, j, (true + rng.integers(-1, 2, size=(C, C)))[:, :, None], axis=2)
    np.put_along_axis(coef, j, rng.uniform(0.3, 0.5, size=(C, C, 1)), axis=2)
    out = ~inside & ~np.eye(C, dtype=bool)
    lag[out], coef[out], ret[out] = 0, np.nan, -3
    d = np.arange(C)
    lag[d, d, 0], coef[d, d, 0] = 0, 1.0
    return lag, coef, ret, T


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


def stats(v):
    v = sorted(v)
    return "median %9.4f  min %9.4f  max %9.4f ms" % (v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:1,64:10,256:40,256:1")
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    lines = ["asx_pool_place_dev behind asx_pool_closure_dev, tolerance 4, min_confirm 1, k = 2, max_hops 64, %d alternating calls, %s"
             % (a.runs, torch.cuda.get_device_name(0))]
    with torch.cuda.stream(st):
        for shape in a.shapes.split(","):
            C, want_hops = (int(v) for v in shape.split(":"))
            k = 2
            lag, coef, ret, T = band(C, want_hops, 2024)
            first = int(np.argmin(T))
            d_in = [torch.from_numpy(x).cuda() for x in (lag, coef, ret)]
            i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")      # noqa: E731
            i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")      # noqa: E731
            best_lag, best_coef = i64(C * C), torch.zeros(C * C, dtype=torch.float64, device="cuda")
            best_ret, best_entry, confirm, root = i32(C * C), i32(C * C), i32(C * C), i32(1)
            c_offset, c_support, placed = i64(C), i32(C), i32(C)
            scratch, offset, hops, support, degree, step = i64(C), i64(C), i32(C), i32(C), i32(C), i64(C)
            resid, state = i64(C * C), i32(C * C)
            torch.cuda.synchronize()

            def closure():
                asx.pool_closure_dev(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), C, k, 4, 1, first, best_lag.data_ptr(),
                                     best_coef.data_ptr(), best_ret.data_ptr(), best_entry.data_ptr(), confirm.data_ptr(),
                                     root.data_ptr(), c_offset.data_ptr(), c_support.data_ptr(), placed.data_ptr(), stream=sp)

            def place(max_hops, sweeps):
                asx.pool_place_dev(best_lag.data_ptr(), best_ret.data_ptr(), confirm.data_ptr(), C, 4, 1, root.data_ptr(), max_hops,
                                   sweeps, offset.data_ptr(), hops.data_ptr(), support.data_ptr(), degree.data_ptr(), step.data_ptr(),
                                   resid.data_ptr(), state.data_ptr(), d_scratch=scratch.data_ptr(), stream=sp)

            closure()
            place(64, 0)
            st.synchronize()
            h = hops.cpu().numpy()
            by_closure = int(placed.cpu().numpy().sum())
            assert (h >= 0).all(), "placement did not reach every clip within 64 hops"
            assert (np.abs(offset.cpu().numpy() - (T - T[first])) <= h).all(), "the clips are not within a frame per hop of their offsets"
            calls = {"closure": closure, "place, sweeps 0": lambda: place(64, 0), "place, sweeps 3": lambda: place(64, 3)}
            if want_hops == 1:
                calls["place, max_hops 1024"] = lambda: place(1024, 0)
            times = timed(torch, st, calls, a.runs, a.warmup)
            st.synchronize()
            lines.append("  C = %3d, hops needed %2d (closure alone places %d of %d clips)" % (C, int(h.max()), by_closure, C))
            for name, v in times.items():
                lines.append("    %-22s %s" % (name, stats(v)))
            med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
            lines.append("    place / closure: %.2f (sweeps 0), %.2f (sweeps 3)"
                         % (med["place, sweeps 0"] / med["closure"], med["place, sweeps 3"] / med["closure"]))
            if want_hops == 1:
                lines.append("    one empty layer launch: %.2f us ((max_hops 1024 - max_hops 64) / 960)"
                             % (1000.0 * (med["place, max_hops 1024"] - med["place, sweeps 0"]) / 960.0))
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

            v = timed(torch, st, {"topk": topk}, a.runs, a.warmup)["topk"]
            plan.sync(sp)
            got = lag.cpu().numpy().reshape(C, C, k)[:, :, 0]
            assert (got == 4000 * (np.arange(C)[None, :] - np.arange(C)[:, None])).all(), "the producer's lags are not the planted ones"
        lines.append("  asx_xcorr_pool_topk_f32_dev, N = %d, 16 clips as both pools, k = 4 (the producer of a 16 x 16 x 4 table): %s"
                     % (n, stats(v)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
