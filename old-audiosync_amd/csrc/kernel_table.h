// csrc/kernel_table.h -- which transform kernels are compiled in: the one statement of it.  Four lists of entries, each entry the
// constants of one kernel instance.  plan_math.cpp matches a host plan against them once, when the plan is built (AsxKernelChoice:
// an index into the layout's two lists, or -1); the launchers of rlayout.hip and xcorr_kernels.hip look the index up
// (asx_with_entry) and name the instance from the entry's constants.  An entry added here is built where a launcher names its
// list; tests/test_plan_math.py reads the lists (asx_planmath_kernel_table) and fails on an entry no plan reaches.
#pragma once

#include "lds_fft.h"

template <class... E> struct AsxEntries {};

// go(Entry{}) for the entry at `index`; false: the list has no such entry
template <class... E, class F> bool asx_with_entry(AsxEntries<E...>, int index, F go)
{
    int i = 0;
    return ((i++ == index && (go(E{}), true)) || ...);
}
// index of the first entry with pred(Entry{}), or -1
template <class... E, class Pred> int asx_match_entry(AsxEntries<E...>, Pred pred)
{
    int at = 0, found = -1;
    (void)((pred(E{}) ? (found = at, true) : (++at, false)) || ...);
    return found;
}
// the run-time schedule `st` is the compile-time schedule S
template <class S> bool schedule_is(const AsxStages &st)
{
    if (st.n != S::n || st.nstages != S::nstages) return false;
    for (int i = 0; i < S::nstages; i++)
        if (st.radix[i] != S::radix(i)) return false;
    return true;
}
// an entry's constants in the order its list states them, then its radices, then a 0 (the diagnostics); out holds ASX_ENTRY_INTS
constexpr int ASX_ENTRY_INTS = 4 + ASX_MAX_STAGES + 1;
template <class E> void asx_entry_spell(E, int *out)
{
    for (int v : E::head) *out++ = v;
    for (int i = 0; i < E::sched::nstages; i++) *out++ = E::sched::radix(i);
    *out = 0;
}

// row pairs a lane group of k_fwd_cols_r<Sched<m1, ...>, t, nt> loads = half the rows of a band (AsxKernelChoice::band_rows)
__host__ __device__ constexpr int rcol_rows_per_group(int m1, int nt, int t) { return (m1 + nt / (t / 4) - 1) / (nt / (t / 4)); }

// ---- the real-column kernels (rlayout.hip) ----
// Column schedules of the production sample lengths (plan_math.cpp's tuned table):  (M1, tile width in real columns, block size,
// radices...).  (1200- and 800-row tiles hold only eight real columns: 32-byte input pieces, measured 25 % slower in k_fwd_cols_r,
// and a fed first stage of radix 10 needs 20 rows in flight per thread: the two longest lengths use 600 / 400 rows with 2400-point
// rows instead.)  Block sizes are measured (profiles/r4_experiments/10_*, 11_*): 400-row tiles 512 threads (320, the packed
// kernels' choice: 12 % slower at N = 480 000), 300-row tiles 256 (320 / 384 / 512: 20-35 % slower).
template <int M1, int T, int NT, int... Rs> struct AsxRCol {
    using sched = Sched<M1, Rs...>;
    static constexpr int t = T, nt = NT, head[] = { M1, T, NT };
};
using AsxRCols = AsxEntries<AsxRCol<600, 16, 512, 10, 10, 6>, AsxRCol<400, 16, 512, 10, 8, 5>, AsxRCol<300, 16, 256, 10, 6, 5>>;

// Row schedules: (block size of a (sub-)row, two-half form, (sub-)row length, radices...); the plan's row length M2 is the
// sub-row's, twice in the two-half form.  Chosen by the row length alone: these kernels carry their own schedule and only read the
// plan's w_M2 table.
// 480-point rows: ONE wave per block -- a block is 11.5 KB of traffic and a chain of five short phases, so what counts is how many
// are in flight: sixteen single-wave blocks per CU against eight of two waves (rows 0.93 -> 0.83 ms per 1024 pairs of N = 144 000,
// same box)
#ifndef ASX_ROWS2_SCHED
#define ASX_ROWS2_SCHED 12, 10, 10 // diagnostic builds (tools/mkr.sh): the schedule of the two-half form's 1200-point sub-rows
// (tools/mkr.sh gives it to rlayout.hip alone: the entry's index is the same -- rows match by length -- and the kernel runs the
// variant's radices, but the diagnostics, spelled by plan_math.cpp, go on showing the default's)
#endif
template <int NT, bool TWO, int N, int... Rs> struct AsxRRow {
    using sched = Sched<N, Rs...>;
    static constexpr int nt = NT, m2 = TWO ? 2 * N : N, head[] = { NT, TWO, N };
    static constexpr bool two = TWO;
};
using AsxRRows = AsxEntries<AsxRRow<128, false, 1200, 12, 10, 10>, AsxRRow<128, true, 1200, ASX_ROWS2_SCHED>, AsxRRow<64, false, 480, 10, 8, 6>>;

// ---- the packed-sample kernels (xcorr_kernels.hip) ----
// Column schedules of the production sample lengths:  (M1, tile width, block size, MAXR for the launch bounds, radices...)
template <int M1, int T, int NT, int MAXR, int... Rs> struct AsxPCol {
    using sched = Sched<M1, Rs...>;
    static constexpr int t = T, nt = NT, maxr = MAXR, head[] = { M1, T, NT, MAXR };
};
using AsxPCols = AsxEntries<AsxPCol<1200, 8, 512, 12, 12, 10, 10>, AsxPCol<800, 8, 320, 10, 10, 10, 8>, AsxPCol<600, 16, 512, 10, 10, 10, 6>,
                            AsxPCol<400, 16, 320, 10, 10, 8, 5>, AsxPCol<300, 16, 256, 10, 10, 6, 5>>;
// Row lengths of the production sample lengths:  (block size, MAXR, row length, radices...)
template <int NT, int MAXR, int N, int... Rs> struct AsxPRow {
    using sched = Sched<N, Rs...>;
    static constexpr int nt = NT, maxr = MAXR, head[] = { NT, MAXR, N };
};
using AsxPRows = AsxEntries<AsxPRow<256, 12, 1200, 12, 10, 10>, AsxPRow<128, 10, 480, 10, 8, 6>>;
