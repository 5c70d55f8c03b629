#!/usr/bin/env python3
"""tools/group_launches.py -- one call of every entry point that reaches run_group (csrc/asx_api.hip), for a launch-for-launch
comparison of two builds of the library:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/group_launches.py
    python3 tools/group_launches.py --list <dir> > launches.txt

The first line makes the calls (fixed inputs, no torch: the device buffers come from the library's own allocator, so every kernel
of the trace is the library's); the second prints the trace's dispatches in order, one `kernel  grid  block  dynamic LDS` line
each, without timings.  Two builds launch the same groups exactly when the two lists are the same bytes.

Shapes: N = 144 000 (the smallest real-column length) in groups of 3 pairs, every entry point, and a pair whose near-tie list
overflows (a source periodic in 8 frames: tests/test_gpu_exact_peak.py) through the float32, top-k and double calls, so that the
second look runs; N = 1000 on a packed plan; N = 960 000, the smallest length with the partial-store kernel, 2 pairs under
set_qstore(2), one of them the comb pair whose stored set falls short (tests/test_qstore_model.py), so that the redo runs."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def listing(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%s  grid %s %s %s  block %s %s %s  lds %s" % (
            r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
            r["Workgroup_Size_Z"], r.get("LDS_Block_Size", "-")))
    print("%d dispatches" % len(rows))


def calls():
    import numpy as np
    import __graft_entry__ as g
    import oracle
    asx = g.load()
    from audiosync_amd.hipxcorr import _Staging

    def pairs(n, count, seed=2024):
        got = [oracle.synth_pair(seed, i, n, 1) for i in range(count)]
        return np.stack([p[0] for p in got]), np.stack([p[1] for p in got])

    def periodic(n):
        per = np.tile(np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32), 2 * n // 8)
        return per, per[:n].copy()

    def batch_dev(plan, src, smp):
        with _Staging(plan) as st:
            d = [st.upload(np.ascontiguousarray(src)), st.upload(np.ascontiguousarray(smp))]
            out = [st.output((len(smp),), dt) for dt in (np.int64, np.float64, np.int32)]
            plan.xcorr_batch_dev(d[0], d[1], len(smp), *out)
            return st.fetch()

    def dumps(plan, src, smp, phat):
        n = plan.sample_len
        with _Staging(plan) as st:
            d_s, d_t = st.upload(np.ascontiguousarray(src)), st.upload(np.ascontiguousarray(smp))
            d_r = st.output((2 * n,), np.float32)
            lag, coef, peak, ret = (st.output((1,), dt) for dt in (np.int64, np.float64, np.float64, np.int32))
            plan.debug_r_dev(d_s, d_t, d_r, lag, coef, ret)
            if phat:
                plan.phat_debug_r_dev(d_s, d_t, d_r, lag, coef, peak, ret)
                plan.phat_band_debug_r_dev(d_s, d_t, n // 100, n // 3, d_r, lag, coef, peak, ret)
            st.fetch()

    def common(plan, src, smp):
        """the calls a plan of either layout takes"""
        n, b = plan.sample_len, len(smp)
        rows = np.array([[-n, n - 1], [-100, 5000], [7, 3]][:b], dtype=np.int64)   # (the last row is not a window)
        print("batch exact", batch_dev(plan, src, smp)[0])
        plan.set_exact(False)
        print("batch asynchronous", batch_dev(plan, src, smp)[0])
        plan.set_exact(True)
        print("strided", plan.xcorr_broadcast_f32(src[0], smp)[0], plan.xcorr_broadcast_f32(src, smp[0])[0],
              plan.xcorr_broadcast_f32(src[0], smp[0])[0])
        print("windowed", plan.xcorr_windowed_f32(src, smp, rows)[0])
        print("top-k", plan.xcorr_topk_f32(src, smp, 3, n // 30)[0].ravel())
        print("host float32", plan.xcorr_batch_f32(src, smp)[0])
        print("double narrowed", plan.xcorr_f64(src[0].astype(np.float64), smp[0].astype(np.float64)))
        print("double", plan.xcorr_f64(src[0].astype(np.float64) + 1e-11, smp[0].astype(np.float64) - 1e-11))
        dumps(plan, src[0], smp[0], plan.layout == "real-column")

    n = 144000
    src, smp = pairs(n, 3)
    with asx.Plan(n, 3, 0) as plan:
        assert plan.layout == "real-column"
        common(plan, src, smp)
        listed = np.array([[0, 0], [1, 1], [0, 2]], dtype=np.int32)
        print("pool", plan.xcorr_pool_f32(src[:2], smp, listed)[0])
        print("pool top-k", plan.xcorr_pool_topk_f32(src[:2], smp, 2, n // 30, listed)[0].ravel())
        print("PHAT", plan.xcorr_phat_f32(src, smp)[0], plan.xcorr_phat_f32(src[0], smp)[0])
        print("PHAT band", plan.xcorr_phat_band_f32(src, smp, n // 100, n // 3)[0])
        print("pool PHAT", plan.xcorr_pool_phat_f32(src[:2], smp, listed)[0],
              plan.xcorr_pool_phat_f32(src[:2], smp, listed, band=(n // 100, n // 3))[0])
        # the second look: the middle pair's near-tie list overflows
        per, per_smp = periodic(n)
        tied_src, tied_smp = np.stack([src[0], per, src[2]]), np.stack([smp[0], per_smp, smp[2]])
        print("second look", batch_dev(plan, tied_src, tied_smp)[0], plan.xcorr_topk_f32(tied_src, tied_smp, 2, 4)[0].ravel(),
              plan.xcorr_f64(per.astype(np.float64), per_smp.astype(np.float64)))
        print("pairs that took the second look:", plan.peak_repairs())

    n = 1000
    src, smp = pairs(n, 3)
    with asx.Plan(n, 3, 0) as plan:
        assert plan.layout == "packed"
        common(plan, src, smp)

    n = 960000
    from test_qstore_model import comb_pair
    m1 = n // 2400
    comb = comb_pair(n, m1, m1 // 3, 8, 123456, 300700, 77)
    one = oracle.synth_pair(20260101, 9, n, 1)
    with asx.Plan(n, 2, 0) as plan:
        plan.set_qstore(2)
        print("partial storing", batch_dev(plan, np.stack([one[0], comb[0]]), np.stack([one[1], comb[1]]))[0])
        print("pairs with a list, storing everything, run again; tiles stored:", plan.qstore_stats())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        calls()
