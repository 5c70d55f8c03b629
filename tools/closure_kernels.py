#!/usr/bin/env python3
"""The kernels' shares of asx_pool_closure_dev from a kernel trace of tools/closure_cost.py.

    rocprofv3 --kernel-trace --stats -d DIR -o t -- python3 tools/closure_cost.py --runs 11
    python3 tools/closure_kernels.py DIR/t_results.db [--out profiles/closure/kernels.txt]

Reads the `kernels` view of the trace's database in launch order.  A call is k_closure_votes, k_closure_confirm, k_closure_root,
k_closure_offsets in a row; the votes launch has C blocks in y, which names the pool size of the three launches behind it (the
root kernel is one block whatever C is).  Prints, per kernel and C, the grid in work-items, the launches and their mean time."""
import argparse
import os
import sqlite3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = sqlite3.connect(a.db).execute("select name, grid_x, grid_y, workgroup_y, end - start from kernels "
                                         "where name like 'k_closure_%' order by start").fetchall()
    stats, clips = {}, None
    for name, gx, gy, wy, ns in rows:
        kernel = name.split("(")[0]
        if kernel == "k_closure_votes":
            clips = gy // max(wy, 1)
        s = stats.setdefault((kernel, clips, gx, gy), [0, 0])
        s[0] += 1
        s[1] += ns
    lines = ["rocprofv3 --kernel-trace --stats -- python3 tools/closure_cost.py --runs 11, reduced by tools/closure_kernels.py:",
             "mean microseconds per launch, grid in work-items (a run of its own, not the run of cost.txt)"]
    for (kernel, c, gx, gy), (count, total) in sorted(stats.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        lines.append("  %-18s C = %4d  grid %8d x %4d  launches %3d  mean %9.1f us" % (kernel, c, gx, gy, count, total / count / 1000.0))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
