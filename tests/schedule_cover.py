"""Which run-time transform schedules the GPU suite runs (test helper, not a conftest; host-only: planmath_describe and
planmath_kernels, no GPU).

Every length outside the kernel table (csrc/kernel_table.h) runs k_fwd_cols<MAXR>, k_rows<MAXR> and k_inv_cols<MAXR, void, ...> of
csrc/xcorr_kernels.hip on the AsxStages that asx_make_stages builds.  What such a plan exercises is a set of FEATURES:

  (family, MAXR, radix, role)  a radix of lds_fft.h in a stage role (first / middle / last / only) inside the MAXR = 10 / 12 / 16
                               instance that asx_launch_*_any picks from the schedule's largest radix; family "cols" or "rows"
  (family, "stages", n)        the number of stages
  (family, "block", nt)        the block size (plan.threads[0] for the columns, [1] for the rows)
  ("cols", "T", t)             the tile width
  ("rows", "M2", parity)       even: the 16-byte form of k_rows' loads and stores, odd: the 4-byte form
  ("rows", "steps", s)         ceil(M2 / block), the bins a thread owns: 1 .. ASX_ROW_STEPS

universe() lists every feature the planner can produce: the forced splits M1 x T x T of every {2,3,5}-smooth M1 with a tile that
fits ASX_LDS_COLS_MAX for the columns, 2 x M2 x 2 of every smooth M2 <= 2048 for the rows; a half that resolves to a compiled-in
entry of the kernel table is left out, it does not run these kernels.  CASES is a greedy cover of that universe, committed as
data: tests/test_schedule_cover.py fails, with the features named, when the planner or asx_make_stages changes and the list
no longer equals the universe; `python tests/schedule_cover.py` prints a fresh one.
tests/test_gpu_schedule_cover.py runs every entry on the device."""
import os
import sys

LDS_COLS_MAX = 80 * 1024          # csrc/plan_math.h: ASX_LDS_COLS_MAX
LDS_ROWS_MAX = 64 * 1024          # ASX_LDS_ROWS_MAX: 4 * M2 * 8
ROW_STEPS = 5                     # csrc/asx_internal.h: ASX_ROW_STEPS
TILES = (2, 4, 8, 16, 32, 64)
M1_MAX = 8192                     # the planner's own bound on M1
N_MIN, N_MAX = 1000, 100000       # a case's length: a fraction of a second on the device, the oracle's float64 transform included
MARGIN_MIN = 1.0 + 1e-9           # oracle's peak margin below which a float32 answer may differ: no case's pair is that close
PLAN_ENV = ("ASX_LAYOUT", "ASX_GENERIC", "ASX_THREADS_COLS", "ASX_THREADS_ROWS", "ASX_STAGE_ORDER")  # read when a plan is built

# ---- the committed lists -------------------------------------------------------------------------------------------------------

# (M1, M2, T, seed): the forced split "M1xM2xT" of N = M1 * M2 (2N smooth, F = 2N); oracle.synth_pair(seed, 0..2, N, 1) are the
# three pairs of the batch check, every one with an oracle margin >= MARGIN_MIN.  Output of `python tests/schedule_cover.py`.
CASES = [
    (2, 2048, 2, 1), (2, 1944, 4, 1), (2, 1536, 8, 1), (2, 1280, 16, 1), (2, 1152, 32, 1), (2, 1024, 64, 1),
    (3, 972, 2, 1), (4, 960, 2, 1), (5, 768, 2, 1), (6, 750, 2, 1), (8, 675, 2, 1), (9, 625, 2, 1),
    (10, 600, 2, 1), (12, 400, 2, 1), (15, 375, 2, 1), (16, 270, 2, 1), (18, 256, 2, 1), (20, 216, 2, 1),
    (25, 192, 2, 1), (27, 180, 2, 1), (27, 160, 32, 1), (32, 150, 2, 1), (54, 144, 2, 1), (60, 135, 2, 1),
    (64, 128, 2, 1), (75, 125, 2, 1), (96, 120, 2, 1), (100, 108, 2, 1), (108, 100, 2, 1), (120, 96, 2, 1),
    (125, 75, 2, 1), (125, 64, 16, 1), (125, 60, 32, 1), (128, 54, 2, 1), (135, 32, 2, 1), (144, 27, 2, 1),
    (150, 25, 2, 1), (160, 20, 2, 1), (162, 18, 2, 1), (180, 16, 2, 1), (192, 15, 2, 1), (216, 12, 2, 1),
    (256, 10, 2, 1), (320, 9, 2, 1), (375, 8, 2, 1), (500, 6, 2, 1), (625, 5, 2, 1), (625, 160, 8, 1),
    (675, 4, 2, 1), (750, 3, 2, 1), (768, 2, 2, 1), (960, 100, 2, 1), (972, 100, 2, 1), (1024, 96, 2, 1),
    (1152, 75, 2, 1), (1280, 75, 2, 1), (1536, 64, 2, 1), (3125, 32, 2, 1), (3840, 25, 2, 1),
]

# (N, M1, M2, T, seed): 2N is not smooth, so the plan is embedded in F = the next smooth even length >= 3N - 1 and M1 * M2 = F / 2.
# Between them: both parities of N, T = 2 and T = 64, a column transform of three and more stages, an odd M2.
EMBEDDED_CASES = [
    (1001, 512, 3, 2, 1), (1006, 24, 64, 64, 1), (3331, 8, 625, 8, 1), (12345, 30, 625, 64, 1), (14000, 2160, 10, 2, 1),
    (33334, 81, 625, 64, 1), (44100, 1350, 50, 2, 1),
]

# N: (F, (M1, M2, T), (column block, row block)) as the planner itself plans the longest lengths (no forced split).
LONG = {
    1953125: (3906250, (3125, 625, 2), (320, 256)),
    2097152: (4194304, (1024, 2048, 8), (512, 512)),
    3999971: (12000000, (3000, 2000, 2), (320, 512)),
    4000000: (8000000, (3200, 1250, 2), (448, 256)),
}


# ---- features ------------------------------------------------------------------------------------------------------------------

def smooth_numbers(lo, hi):
    out = []
    a = 1
    while a <= hi:
        b = a
        while b <= hi:
            c = b
            while c <= hi:
                if c >= lo:
                    out.append(c)
                c *= 5
            b *= 3
        a *= 2
    return sorted(out)


def split_string(m1, m2, t):
    return "%dx%dx%d" % (m1, m2, t)


def maxr_instance(radices):
    """the MAXR of the kernel instance asx_launch_*_any launches (csrc/xcorr_kernels.hip: max_radix)"""
    m = max([2] + list(radices))
    return 10 if m <= 10 else 12 if m <= 12 else 16


def stage_roles(radices):
    if len(radices) == 1:
        return [(radices[0], "only")]
    return [(r, "first" if i == 0 else "last" if i == len(radices) - 1 else "middle") for i, r in enumerate(radices)]


def column_features(d, k):
    """features of the column half of a plan (d = planmath_describe, k = planmath_kernels); empty on a compiled-in schedule"""
    if k["layout"] != "packed" or k["cols"] is not None:
        return set()
    inst = maxr_instance(d["radix1"])
    f = {("cols", inst, r, role) for r, role in stage_roles(d["radix1"])}
    return f | {("cols", "stages", len(d["radix1"])), ("cols", "block", k["threads"][0]), ("cols", "T", d["T"])}


def row_features(d, k):
    if k["layout"] != "packed" or k["rows"] is not None:
        return set()
    inst = maxr_instance(d["radix2"])
    nt = k["threads"][1]
    f = {("rows", inst, r, role) for r, role in stage_roles(d["radix2"])}
    return f | {("rows", "stages", len(d["radix2"])), ("rows", "block", nt), ("rows", "M2", "odd" if d["M2"] & 1 else "even"),
                ("rows", "steps", (d["M2"] + nt - 1) // nt)}


def plan_of(mod, n, split=None):
    """(describe, kernels) of the host-only planner; the caller keeps PLAN_ENV out of the environment"""
    return mod.planmath_describe(n, split), mod.planmath_kernels(n, split)


def features(mod, n, split=None):
    d, k = plan_of(mod, n, split)
    return column_features(d, k) | row_features(d, k)


def case_features(mod, case):
    m1, m2, t = case[:3]
    return features(mod, m1 * m2, split_string(m1, m2, t))


def column_universe(mod):
    """{(M1, T): features} of every column configuration that runs the run-time kernels"""
    out = {}
    for m1 in smooth_numbers(2, M1_MAX):
        for t in TILES:
            if m1 * t * 8 > LDS_COLS_MAX:
                continue
            d, k = plan_of(mod, m1 * t, split_string(m1, t, t))
            f = column_features(d, k)
            if f:
                out[(m1, t)] = f
    return out


def row_universe(mod):
    out = {}
    for m2 in smooth_numbers(2, LDS_ROWS_MAX // 32):
        d, k = plan_of(mod, 2 * m2, split_string(2, m2, 2))
        f = row_features(d, k)
        if f:
            out[m2] = f
    return out


def universe(mod):
    u = set()
    for f in column_universe(mod).values():
        u |= f
    for f in row_universe(mod).values():
        u |= f
    return u


def carriers(mod, cases):
    """{feature: [the cases that run it]}"""
    out = {}
    for c in cases:
        for f in case_features(mod, c):
            out.setdefault(f, []).append(c)
    return out


# ---- a fresh cover ---------------------------------------------------------------------------------------------------------------

def greedy(configs, cost):
    """configs {key: features}: keys that cover every feature, each step the key with the least cost per newly covered feature"""
    todo = set()
    for f in configs.values():
        todo |= f
    picked = []
    while todo:
        best = min((k for k in configs if configs[k] & todo), key=lambda k: (cost(k) / len(configs[k] & todo), cost(k), k))
        picked.append(best)
        todo -= configs[best]
    return picked


def pair_up(cols, rows):
    """column configurations in ascending M1 against row lengths in descending M2; a partner outside N_MIN .. N_MAX or with
    M2 < T gives way to the next one that fits, and what is left over of either list takes a partner a second time"""
    cols = sorted(cols)
    rows = sorted(rows, reverse=True)

    def fits(c, m2):
        return N_MIN <= c[0] * m2 <= N_MAX and m2 >= c[1]

    cases, left = [], list(rows)
    for c in cols:
        m2 = next((m for m in left if fits(c, m)), None)
        if m2 is None:
            m2 = next(m for m in rows if fits(c, m))
        else:
            left.remove(m2)
        cases.append((c[0], m2, c[1]))
    for m2 in left:
        c = next(c for c in cols if fits(c, m2))
        cases.append((c[0], m2, c[1]))
    return cases


def margins(n, seed, count=3):
    import oracle
    return [oracle.cross_correlation(*oracle.synth_pair(seed, i, n, 1)[:2], want_results=True)[4] for i in range(count)]


def pick_seed(n, count=3):
    return next(s for s in range(1, 100) if min(margins(n, s, count)) >= MARGIN_MIN)


def fresh_cases(mod):
    cu, ru = column_universe(mod), row_universe(mod)
    cols = greedy(cu, lambda k: k[0] * k[1])
    rows = greedy(ru, lambda k: k)
    return cols, rows, [c + (pick_seed(c[0] * c[1]),) for c in pair_up(cols, rows)]


def radix_report(mod, cases):
    """per radix and family: the cases that run it, with the stage role"""
    car = carriers(mod, cases)
    lines = []
    for r in (16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2):
        for fam in ("cols", "rows"):
            hits = sorted((f[1], f[3], split_string(*c[:3])) for f, cs in car.items() if f[0] == fam and f[2] == r and
                          isinstance(f[1], int) for c in cs[:2])
            lines.append("radix %2d %s: %s" % (r, fam, ", ".join("%s in <%d> %s" % (role, inst, s) for inst, role, s in hits)))
    return lines


if __name__ == "__main__":
    for name in PLAN_ENV:
        os.environ.pop(name, None)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from util import asx
    m = asx()
    cols, rows, cases = fresh_cases(m)
    print("# universe: %d features; %d column configurations, %d row lengths, %d cases" % (len(universe(m)), len(cols), len(rows),
                                                                                         len(cases)))
    print("# columns (M1, T):", sorted(cols))
    print("# rows M2:", sorted(rows))
    print("CASES = [")
    for i in range(0, len(cases), 6):
        print("    " + " ".join("(%d, %d, %d, %d)," % c for c in cases[i:i + 6]))
    print("]")
    print("LONG = {")
    for n in sorted(LONG) or (1953125, 2097152, 3999971, 4000000):
        d, k = plan_of(m, n)
        print("    %d: (%d, (%d, %d, %d), %r)," % (n, d["F"], d["M1"], d["M2"], d["T"], tuple(k["threads"])))
    print("}")
    for line in radix_report(m, cases):
        print("# " + line)
