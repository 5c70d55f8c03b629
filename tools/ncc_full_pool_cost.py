#!/usr/bin/env python3
"""What the pool form of the full-range normalised cross-correlation costs: all pairs of one pool of C clips, next to the strided
full-range call on the same pairs materialised, on one plan.

    python3 tools/ncc_full_pool_cost.py [--n 144000] [--clips 8,16,32] [--runs 11] [--warmup 2] [--out FILE]

Clip c is fixture-C-like (tests/ncc_topk_model.py), as in tools/ncc_pool_cost.py: its sample is unit noise + 0.25, its source unit
noise plus 0.3 / 1.0 / 0.6 times the sample at lags N/10, N/2 and 8N/10 and a level step of 2.0 from frame 1.3 N on.  The C x C pairs
are every source against every sample.  The method is tools/ncc_cost.py's: the calls ALTERNATE within each of --runs rounds, each
between two events on the stream, for k = 1 and k = 4 (min_separation N / 100, min_overlap (N + 1) / 2):
  full       asx_xcorr_ncc_full_f32_dev / asx_xcorr_ncc_full_topk_f32_dev on the materialised pairs [C * C][2N], [C * C][N]
  pool_full  asx_xcorr_pool_ncc_full_f32_dev / asx_xcorr_pool_ncc_full_topk_f32_dev
The tool asserts that the pool call's four outputs are the bytes of the strided call's.  Prints median, minimum and maximum in
milliseconds and the ratio, and appends the same text to --out."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=144000)
    ap.add_argument("--clips", default="8,16,32")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    asx = graft.load()
    n = a.n
    lags = (n // 10, n // 2, (8 * n) // 10)
    sep, mo = n // 100, (n + 1) // 2
    lines = []
    with asx.Plan(n, 4096, 0) as plan:
        for c in [int(v) for v in a.clips.split(",")]:
            b = c * c
            gen = torch.Generator(device="cuda").manual_seed(3000)
            smp = torch.randn((c, n), dtype=torch.float32, device="cuda", generator=gen) + 0.25
            src = torch.randn((c, 2 * n), dtype=torch.float32, device="cuda", generator=gen)
            for gain, lag in zip((0.3, 1.0, 0.6), lags):
                src[:, lag:lag + n] += gain * smp
            src[:, (13 * n) // 10:] += 2.0
            ia = torch.arange(c, device="cuda").repeat_interleave(c)
            ib = torch.arange(c, device="cuda").repeat(c)
            src_m, smp_m = src[ia].contiguous(), smp[ib].contiguous()
            kmax = 4
            out = (torch.empty(b * kmax, dtype=torch.int64, device="cuda"), torch.empty(b * kmax, dtype=torch.float64, device="cuda"),
                   torch.empty(b * kmax, dtype=torch.float64, device="cuda"), torch.empty(b * kmax, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            st = torch.cuda.Stream()
            sp = st.cuda_stream
            S, T, SM, TM = src.data_ptr(), smp.data_ptr(), src_m.data_ptr(), smp_m.data_ptr()
            out4 = tuple(t.data_ptr() for t in out)
            calls = {}
            for k in (1, 4):
                calls["full k = %d" % k] = (lambda k=k: plan.xcorr_ncc_full_topk_dev(SM, 2 * n, TM, n, 0, 0, b, 1e-3, mo, k, sep, *out4, sp))
                calls["pool_full k = %d" % k] = (lambda k=k: plan.xcorr_pool_ncc_full_topk_dev(S, 2 * n, c, T, n, c, 0, 0, 0, b, 1e-3, mo,
                                                                                               k, sep, *out4, sp))
            times = {name: [] for name in calls}
            with torch.cuda.stream(st):
                for run in range(a.warmup + a.runs):
                    for name, fn in calls.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(st)
                        fn()
                        e1.record(st)
                        e1.synchronize()
                        if run >= a.warmup:
                            times[name].append(e0.elapsed_time(e1))
                for k in (1, 4):
                    calls["full k = %d" % k]()
                    plan.sync(sp)
                    want = [t[:b * k].cpu().numpy().tobytes() for t in out]
                    calls["pool_full k = %d" % k]()
                    plan.sync(sp)
                    assert [t[:b * k].cpu().numpy().tobytes() for t in out] == want, "the pool call is not the strided call's bits"
                top = out[0][:4 * b].cpu().reshape(c, c, 4)
                for i in range(c):
                    assert top[i, i, :3].tolist() == [lags[1], lags[2], lags[0]], (i, top[i, i])
            med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
            lines.append("N = %d, C = %d clips, %d pairs (plan group %d; full-range groups of %d), split %s (%s), %d alternating calls, %s"
                         % (n, c, b, plan.group, max(1, min(plan.group, (1 << 30) // (72 * n))), plan.split, plan.layout, a.runs,
                            torch.cuda.get_device_name(0)))
            for name, v in times.items():
                v = sorted(v)
                lines.append("  %-16s median %10.4f  min %10.4f  max %10.4f ms" % (name, v[len(v) // 2], v[0], v[-1]))
            lines.append("  pool_full / full: k = 1 %.2f, k = 4 %.2f (medians); per pair: full %.2f / %.2f us, pool_full %.2f / %.2f us"
                         % (med["pool_full k = 1"] / med["full k = 1"], med["pool_full k = 4"] / med["full k = 4"],
                            1e3 * med["full k = 1"] / b, 1e3 * med["full k = 4"] / b, 1e3 * med["pool_full k = 1"] / b,
                            1e3 * med["pool_full k = 4"] / b))
            del src, smp, src_m, smp_m, out
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
