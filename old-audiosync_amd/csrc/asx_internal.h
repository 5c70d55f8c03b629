// csrc/asx_internal.h — shared between the host side of the HIP layer
// (asx_api.hip) and the gfx950 kernels (xcorr_kernels.hip).
//
// Notation (also used in DESIGN.md and tests/model_fourstep.py):
//   N   sample_len                      F   real transform length (even)
//   M   F/2, complex transform length   M = M1*M2
//   j = j1*M2 + j2  (time index of the packed complex sequence)
//   k = k1 + M1*k2  (frequency index)
//   every intermediate in HBM is row-major [M1][M2] per pair
//   rows of the spectra sit at the DIGIT-REVERSED position pos1[k1]
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define ASX_MAX_STAGES 12
#define ASX_TW_LOG 11                       // two-level twiddle: low table has 2^11 entries
#define ASX_TW_LO (1u << ASX_TW_LOG)
#define ASX_THREADS 256                     // block size of the streaming kernels
#define ASX_FFT_THREADS_MAX 512             // upper bound for the three transform kernels
#define ASX_COL_LOADS 10                    // tile loads a thread keeps in flight in the column kernels
#define ASX_ROW_STEPS 5                     // max ceil(M2 / blockDim) in k_rows (bins a thread owns in the load / combine / store phases)
#define ASX_PEARSON_BLOCKS_MAX 512          // upper limit of the partial-sum blocks per pair (asx_pearson_blocks: by the length alone)
#define ASX_DC_STATS_DOUBLES (4 + 2 * 128)  // second look: {mean, sum, shift, -} + the per-block partials of k_dc_partial
// Peak refinement (src/cross_correlation.c:52-67 is a float64 scan).  The transforms run in float32, so
// every float32 r[k] is off by at most B = ASX_BOUND_C * eps32 * log2(F) * |source|_2 * |sample|_2
// (a worst-case bound of the three transforms is ~3 eps log2 F; measured maximum 0.4 eps log2 F).
// Every lag whose float32 key is within 2B of the float32 maximum is re-evaluated EXACTLY (float64
// dot product of the inputs, compensated summation) and the reference's rule is applied to the exact
// values -- for any number of such lags up to the per-pair capacity below (pure tones at N = 1 440 000
// have ~5 000).  The norms come for free from k_fwd_cols (it reads every input sample anyway).
#define ASX_BOUND_C 4.0f
// Pruned inverse pass (rlayout.hip: k_tile_bounds): a column tile of r whose bound ub = sqrt(4 M1 E) (1 + ASX_PRUNE_DELTA) lies under the
// near-maximum window is not transformed.  What the factor has to cover, in units of eps32 = 2^-23, derived as ASX_BOUND_C is:
//   the computed E against the exact energy of the float32 Q: |Q|^2 two roundings, four levels of additions of non-negative terms
//     (a balanced tree over the tile's sixteen columns: k_rows_re's four DPP steps inside a row of sixteen lanes pair the columns as
//     tree_sum<16> does, so this stands for them as written), the float64 sum over the rows and the square root nothing: 6 u = 3 eps
//     on E, 1.5 eps on its root;
//   the computed tile r^ against the exact transform r of that Q: no element of r^ exceeds its column's 2-norm, and the float32
//     c2r transform of length 2 M1 <= 1200 delivers a column whose 2-norm is off by at most C eps log2(2 M1) of it -- the worst-case
//     constant of one transform is ~1 (a third of the three transforms' ~3 in ASX_BOUND_C's note), taken as ASX_BOUND_C = 4 here as
//     there: 4 * 10.3 = 41 eps, the tangling's few roundings included.
//   a block of k_rows_rm whose pair has a list (rlayout.hip: ASX_QTW_LATE) squares S, the output of the last radix-2 combine, and not
//     the Q = S conj(g) that is stored, g the four-step twiddle as the kernel forms it: up to three table pairs (w_F^(k1 j), w_F^(k1 n),
//     leg[t]), six entries each rounded once per component, whose modulus is 1 to within u = 2^-24 each, joined by up to five complex
//     products, plus the product S conj(g) itself -- six products at sqrt(5) u each at the most (2 u each as fused here).  |Q| and |S|
//     therefore differ by at most (6 + 6 sqrt(5)) u = 19.4 u relatively, |Q|^2 and |S|^2 by 39 u: 20 eps on E, 10 eps on its root,
//     in either direction.  (Typical: a few u; the roundings do not line up.)
// 43 + 10 = 53 eps = 6.3e-6 = 2^-17.3 (43 eps = 2^-17.6 for the blocks that square Q itself).  The bound has a factor 1.8 to spare on
// the generator's pairs (the second-largest bound is <= 0.56 of the peak), so the factor is rounded up generously: 2^-14 = 512 eps,
// nearly ten times what the derivation asks for; the late twiddle fits inside it and does not change it.
// All of the above are RELATIVE roundings.  |Q|^2 = re * re + im * im can also underflow: each of the two products loses up to
// FLT_MIN absolutely when it is flushed or denormal (r itself, a sum of 2 M1 such Q, is then still an ordinary float32: tracks of
// amplitude 1e-16 give |r| ~ 5e-23 and every |Q|^2 = 0).  A tile's energy is a sum of n = 16 (M1 + 1) terms, so its absolute error
// from underflow is at most 2 n FLT_MIN; with E >= 2^25 n FLT_MIN that is 2^-24 E = eps / 2 more on E, inside the factor.  Below
// that floor (ASX_PRUNE_FLOOR_PER_TERM per term: 2^25 * 2^-126 = 2^-101) k_tile_bounds states no bound: ub = +infinity, the tile is
// transformed.  (The floor in r: sqrt(4 M1 n 2^-101) = 3e-12 at M1 = 600 -- pairs that quiet lose the pruning, nothing else.)
#define ASX_PRUNE_DELTA 6.103515625e-5f
#define ASX_PRUNE_FLOOR_PER_TERM 3.944304526105059e-31
#define ASX_PRUNE_T 16                      // the tile width the row pass sums energies for (every real-column schedule's)
// Partial storing of Q (rlayout.hip: k_rows_rm, k_q_predict).  A pair's stored column tiles travel as one 64-bit
// word: four 16-bit tile indices, tile 0 first, 0xFFFF = no tile; ASX_Q_ALL = every tile (the whole of Q, as k_rows_re stores it).
// ASX_QSTORE_C: a tile is predicted when its energy over the predictor rows exceeds this many medians of the pair's tiles.  Derived on
// the CPU with tests/model_fourstep.py (tests/test_qstore_model.py restates it): over eight predictor rows the LARGEST tile of
// unrelated Gaussian tracks reaches 1.37 medians at most over 300 pairs of 30 tiles (99 %: 1.34; the sum of 8 x 16 values of |Q|^2 has
// a relative deviation of about 0.09, and more rows or fewer tiles only narrow it: 1.17 over 32 rows), while the peak's tile of the
// bench generator's pairs stands at 3.8 ... 9.3 medians at noise shift 1 and 2.2 ... 4.3 at noise shift 0 with 30 tiles, every other
// tile under 1.3; with the 150 tiles of the two-half form a planted delay's tile stands at about 36 medians (the peak's energy is in
// one tile of five times as many).  1.75 leaves a quarter above the noise and a quarter below the weakest generator pair.  A wrong
// prediction costs time, never a result: k_prune_select checks the stored set against the exact bounds and sends the pair through
// the full-store path again.
#define ASX_Q_ALL 0xFFFFFFFFFFFFFFFFull
#define ASX_QSTORE_C 1.75
#define ASX_QSTORE_REDO 0x80000000u         // an entry of the overflow list with this bit: run the pair again with partial storing off
__host__ __device__ inline bool asx_q_stored(unsigned long long w, int tile)
{
    const unsigned t = (unsigned)tile;
    return w == ASX_Q_ALL || (unsigned)(w & 0xFFFFu) == t || (unsigned)((w >> 16) & 0xFFFFu) == t ||
           (unsigned)((w >> 32) & 0xFFFFu) == t || (unsigned)((w >> 48) & 0xFFFFu) == t;
}
// The rows of one k_rows_rm launch: `count` rows of every pair, block r of a pair taking row r, or r + hop from r = row_a on -- one
// compare and one add, so that one kernel serves the predictor rows (row_a = 0, hop = the first of them) and the rest (row_a = the
// first predictor row, hop = their number).
struct AsxRowRun {
    int row_a = 0, count = 0, hop = 0;
};
#define ASX_CAND_MAX 16384                  // upper limit of a plan's per-pair candidate capacity
#define ASX_CAND_MIN 2048
#define ASX_DOT_BLOCKS 128                  // blocks per pair that walk the pair's candidate list

// Radix schedule of one in-LDS transform of length n.
// DIF stage i works on sub-blocks of length ns[i] = n / (radix[0]*...*radix[i-1]).
struct AsxStages {
    int n;
    int nstages;
    int radix[ASX_MAX_STAGES];
    int ns[ASX_MAX_STAGES];                 // sub-block length at DIF stage i
    int q[ASX_MAX_STAGES];                  // ns / radix  (butterflies per sub-block, and the leg stride)
    int nbf[ASX_MAX_STAGES];                // n / radix   (butterflies per transform)
    int twmul[ASX_MAX_STAGES];              // n / ns      (step in the w_n table for this stage)
    float inv_q[ASX_MAX_STAGES];            // 1/q and 1/nbf for the exact float division helper
    float inv_nbf[ASX_MAX_STAGES];
};

// Everything a kernel needs to know about a plan.  Kernels get a POINTER to a device copy:
// passed by value, the dynamically indexed stage arrays made hipcc spill the whole struct to scratch.
struct AsxDev;
struct AsxDev {
    uint32_t N;            // sample_len
    uint32_t F, M;         // real / complex transform length
    int M1, M2;            // M = M1*M2
    int T, logT;           // tile width (columns per block) of the column kernels, power of two
    int ntiles;            // ceil(M2 / T)
    int threads_cols, threads_rows; // block sizes of the column / row kernels
    uint32_t src_valid;    // how many leading real samples of the (periodically extended) source are non-zero
    uint32_t src_period;   // 2N
    uint32_t nout;         // 2N: lags searched
    float bound_scale;     // 2 * ASX_BOUND_C * eps32 * log2(F) * F: bound2 = bound_scale * |source|_2 * |sample|_2 (r is scaled by F)
    AsxStages st1, st2;    // schedules for length M1 and M2
    const float2 *tw1;     // w_{M1}^q, q < M1
    const float2 *tw2;     // w_{M2}^q, q < M2
    const float2 *tw2s;    // the same in slot order: tw2s[pos2_of_k2[k2]] = w_{M2}^k2
    const float2 *tw_lo;   // w_F^q, q < 2^ASX_TW_LOG
    const float2 *tw_hi;   // w_F^(h * 2^ASX_TW_LOG)
    const int *k1_of_pos1; // row slot -> k1
    const int *pos1_of_k1; // k1 -> row slot
    const int *pos2_of_k2; // k2 -> slot inside a row after the forward row transform
    const int4 *row_tasks; // [M1/2+1] {slot of row k1, slot of row M1-k1, k1, M1-k1}: one load starts a k_rows block
    int band_rows, nbands; // spectral Pearson form: rows of the [2 M1][M2] sample matrix per band (what one lane group of k_fwd_cols_r
                           // loads: AsxKernelChoice::band_rows), bands of the source = 2 M1 / band_rows; 0 = not available
    int rlayout;           // 1: this plan runs the real-column kernels (rlayout.hip); 0: the packed-sample kernels (xcorr_kernels.hip)
    const int4 *col_pairs; // real-column kernels (rlayout.hip): [M1/2 + 1] {u, slot of u, slot of M1 - u, 0}; null = not available
    const float2 *col_tw;  // w_{2 M1}^u, same order
    const AsxDev *self_dev; // device copy of this struct (what the kernels read)
    unsigned long long *stamps; // diagnostic builds (-DASX_STAMPS) only: per-block phase clocks, 8 slots per block
    int stamp_kernel;      // which kernel records them: 0 k_rows, 1 k_fwd_cols, 2 k_inv_cols ($ASX_STAMPS = 1 | fwd | inv)
    int kcols, krows;      // host only (no kernel reads them): the plan's entries of its layout's lists in kernel_table.h, what the
                           // launchers look up (AsxKernelChoice::cols / rows; -1, packed plans only: the run-time-schedule kernel)
};

// Peak-search partial: order-preserving key in the high word, ~index in the low word,
// so that a plain unsigned max picks the largest key and, among equals, the smallest index
// (src/cross_correlation.c:60 uses a strict '>').
typedef unsigned long long asx_peak_t;

struct AsxSeg {           // per pair, produced by k_finalize
    long long lag;        // wrapped lag (src/cross_correlation.c:256-271)
    uint32_t src_off;     // first source frame of the compared segment
    uint32_t smp_off;     // first sample frame
    uint32_t len;         // segment length (N, or N-|lag|; may be 0)
    uint32_t peak;        // raw argmax index in [0, 2N)
    uint32_t flags;       // ASX_SEG_INEXACT: the pair's near-tie list overflowed, `peak` is the float32 argmax (to be looked at again)
};
#define ASX_SEG_INEXACT 1u

// Lag window of the peak search (asx_plan_set_lag_window).  Lags lo..hi are the indices a, a+1, ..., a+w of r modulo n = 2N
// (lag l >= 0 is index l, lag l < 0 index 2N + l: the inverse of the wrap at src/cross_correlation.c:256-263) -- one range, or two
// when the window holds lag 0 and a negative lag.  seed = the smallest in-window index: the element that starts the reference's
// running maximum with its SIGNED value (arr[0], :56), 0 for every window that holds lag 0.  The full window (a = N, w = 2N - 1,
// seed = 0) runs the kernels without a window; the others run k_inv_cols_r<..., AsxWin> / k_inv_cols<..., AsxWin>, which mask every
// key they form with asx_win_has.  Travels by value as a kernel argument: it is its own selection (see "Selections" below).
struct AsxWin {
    uint32_t a, w, seed, n;
    static constexpr bool masks = true;
    __device__ __forceinline__ AsxWin window_of(size_t, uint32_t) const { return *this; }
};
__host__ __device__ inline bool asx_win_has(const AsxWin &z, uint32_t idx)
{
    if (idx >= z.n) return false; // (packed plans: the embedding's lags past 2N)
    const uint32_t d = idx >= z.a ? idx - z.a : idx + (z.n - z.a);
    return d <= z.w;
}
__host__ __device__ inline AsxWin asx_win_of(int64_t lo, int64_t hi, uint32_t N)
{
    AsxWin z;
    z.n = 2u * N;
    z.a = (uint32_t)(lo >= 0 ? lo : (int64_t)z.n + lo);
    z.w = (uint32_t)(hi - lo);
    z.seed = (lo < 0 && hi >= 0) ? 0u : z.a;
    return z;
}

// Per-pair lag windows (asx_xcorr_windowed_f32_dev): pair k of a group reads its row {lag_min, lag_max} at rows + 2 k step, in device
// memory, when its kernels run (step 0: one row for every pair).  The group's pointer is already offset to its first pair
// (Pairs::at, asx_api.hip).  The per-pair kernels (the <..., AsxWinRows> instances of k_inv_cols_r, k_inv_cols, k_finalize
// and k_refine_pick; k_pearson_prep_p, _pl) form their AsxWin from it with asx_win_row instead of taking one by value: it is a selection too.
struct AsxWinRows;
__device__ inline bool asx_win_row(const AsxWinRows &R, size_t pair, uint32_t N, AsxWin &z);
struct AsxWinRows {
    const int64_t *rows;
    size_t step;
    static constexpr bool masks = true;
    __device__ __forceinline__ AsxWin window_of(size_t pair, uint32_t N) const
    {
        AsxWin z;
        (void)asx_win_row(*this, pair, N, z);
        return z;
    }
    __device__ __forceinline__ uint32_t seed_of(size_t pair, uint32_t N) const { return window_of(pair, N).seed; }
};
// A valid row (-N <= lag_min <= lag_max <= N-1) gives asx_win_of's window.  Any other row gives n = 0, a window that holds no index:
// nothing competes, nothing is listed, the running maximum stays empty (seed 0), and k_invalid_rows writes (0, NaN, -2) behind the
// Pearson kernels.
__device__ inline bool asx_win_row(const AsxWinRows &R, size_t pair, uint32_t N, AsxWin &z)
{
    const int64_t *row = R.rows + 2 * pair * R.step;
    const int64_t lo = row[0], hi = row[1], n = (int64_t)N;
    const bool ok = -n <= lo && lo <= hi && hi <= n - 1;
    if (ok) z = asx_win_of(lo, hi, N);
    else z.a = z.w = z.seed = z.n = 0u;
    return ok;
}

// Top-k peaks (asx_xcorr_topk_f32_dev): pass 1 is the strided / windowed call's peak search; pass j >= 2 searches the same Q again
// with A_j = the call's window minus the zones |lag - lag_i| <= min_separation around the entries i < j (lags, not indices: -N and
// N-1 are far apart).  k_topk_step (xcorr_kernels.hip) writes entry j and prepares pass j + 1 in the group's AsxTopkPair records; the
// pass kernels (k_inv_cols_r / k_inv_cols<..., AsxSelTopk<ZC>>, k_finalize / k_refine_pick<AsxSelTopkSeed>, k_pearson_prep_x, _xl)
// read them.
#define ASX_TOPK_MAX 8
#define ASX_TK_EMPTY 1u   // A_j is empty: this entry and every later one are (0, NaN, -3)
#define ASX_TK_INVALID 2u // the pair's row is not a window: every entry is (0, NaN, -2)
#define ASX_TK_INEXACT 4u // a pass of this call overflowed its near-tie list: counted and listed once; ret = 1 from that entry on
struct AsxTopkPair {
    AsxWin z;                     // the next pass's window: the call's, with seed = the smallest index of A_j (n = 0: nothing competes)
    int32_t lo[ASX_TOPK_MAX - 1]; // zone i: lags lo[i] .. lo[i] + wd[i] (an earlier entry +- min_separation, clipped to [-N, N-1])
    uint32_t wd[ASX_TOPK_MAX - 1];
    uint32_t nz;                  // zones so far
    uint32_t flags;               // ASX_TK_*
    int32_t wlo, whi;             // the call's window in lags
};
// What the top-k inverse kernels hand their body as Z: an AsxWin whose asx_win_has also leaves out the zones.  The bodies only ask
// Z.seed and asx_win_has(Z, idx), so they compile unchanged against it.  An in-window index at distance d from a is the lag
// wlo + d, so zone i is the distances zo[i] .. zo[i] + wd[i] (zo[i] = lo[i] - wlo, wrapping): two operations per zone and index,
// for ZC zones -- the kernel's capacity, chosen per pass by the launcher (1, 3 or 7); the unused ones are (~0, 0), which hold
// no distance (d - ~0 = d + 1 > 0).  (Testing only the first nz zones under a run-time guard kept the lane masks in VGPRs and
// spilled the top-k inverse kernel to scratch.)
template <int ZC> struct AsxWinX {
    uint32_t a, w, seed, n;
    uint32_t zo[ZC];
    uint32_t wd[ZC];
};
template <int ZC> __host__ __device__ inline bool asx_win_has(const AsxWinX<ZC> &z, uint32_t idx)
{
    if (idx >= z.n) return false;
    const uint32_t d = idx >= z.a ? idx - z.a : idx + (z.n - z.a);
    bool in = d <= z.w;
#pragma unroll
    for (int i = 0; i < ZC; i++) in = in && d - z.zo[i] > z.wd[i];
    return in;
}
template <int ZC> __host__ __device__ inline AsxWinX<ZC> asx_win_x(const AsxTopkPair *X, size_t pair)
{
    const AsxTopkPair &t = X[pair];
    AsxWinX<ZC> z;
    z.a = t.z.a; z.w = t.z.w; z.seed = t.z.seed; z.n = t.z.n;
#pragma unroll
    for (int i = 0; i < ZC; i++) {
        const bool used = (uint32_t)i < t.nz;
        z.zo[i] = used ? (uint32_t)(t.lo[i] - t.wlo) : ~0u;
        z.wd[i] = used ? t.wd[i] : 0u;
    }
    return z;
}
// per-lane top-k workspace: the records and pass j's results, which k_topk_step moves to entry j of the caller's arrays
struct AsxTopkWs {
    AsxTopkPair *pairs;          // [pairs]
    int64_t *lag;                // [pairs]
    double *coef;                // [pairs]
    int32_t *ret;                // [pairs]
    unsigned long long *sink;    // [1] where k_finalize's top-k form counts the later overflows of a pair already counted in this call
};

// Which lags compete for pair i of a group, and what seeds its running maximum: the host's one statement of that choice.  Host only,
// never a kernel argument: asx_with_selection (below) turns it into the selection object a kernel template takes; launch_prep
// (pearson_spectral.hip), whose family keeps a kernel per flavour, switches on `kind`.
//   ALL     every lag, seed 0 (<..., AsxSelAll>; <AsxSelSeed> with seed 0).  The plan's full window is this: it launches exactly the
//           kernels of a plan that never had one.
//   WINDOW  the plan's window (asx_plan_set_lag_window), by value, the seed inside it (k_inv_cols_r / k_inv_cols<..., AsxWin>;
//           k_finalize and k_refine_pick<AsxSelSeed> and k_pearson_prep take the seed)
//   ROWS    per-pair windows, which replace the plan's: each pair's row and seed from device memory (<AsxWinRows>, k_pearson_prep_p)
//   TOPK    a top-k pass >= 2, which replaces both: each pair's window, seed and zones from its record (<AsxSelTopk<ZC>>,
//           <AsxSelTopkSeed>, k_pearson_prep_x)
struct AsxSearch {
    enum Kind { ALL, WINDOW, ROWS, TOPK } kind;
    int64_t lo, hi;              // the plan's window in lags ...
    AsxWin win;                  // ... and as indices
    AsxWinRows rows;             // the call's per-pair windows (rows.rows null: none)
    const AsxTopkPair *tk;       // TOPK: the group's records,
    int tk_zones;                //   the most zones one of them holds in this pass (asx_with_selection picks the zone capacity by it)
    unsigned long long *tk_sink; //   and AsxTopkWs::sink
    // the index an empty running maximum stands for, and the one whose exact value competes signed -- where a kernel takes it by
    // value (the ROWS and TOPK kernels read each pair's own)
    uint32_t seed() const { return kind == WINDOW ? win.seed : 0u; }
    // pass 0: the call's own search (the strided / windowed call's; what k_topk_step starts the records from); pass j >= 1 of a
    // top-k call: the records of lane workspace T, which by then hold at most j zones
    static AsxSearch of(int64_t lo, int64_t hi, uint32_t N, const int64_t *rows, size_t rows_step, const AsxTopkWs &T, int pass)
    {
        AsxSearch q{ ALL, lo, hi, asx_win_of(lo, hi, N), { rows, rows_step }, nullptr, 0, nullptr };
        if (pass > 0) { q.kind = TOPK; q.tk = T.pairs; q.tk_zones = pass; q.tk_sink = T.sink; }
        else if (rows) q.kind = ROWS;
        else if (lo != -(int64_t)N || hi != (int64_t)N - 1) q.kind = WINDOW;
        return q;
    }
};

// Pool calls (asx_xcorr_pool_f32_dev, asx_xcorr_pool_topk_f32_dev): pair i of a call is source a_i of one pool against sample b_i of another.  Every track of both
// pools has its forward column pass in the plan's bank (written once per call); k_pool_resolve (rlayout.hip) turns each pair of a launch
// group into one of these records in the lane's workspace, and the listed kernels (k_rows_rl; the <..., AsxAtList> instances of
// k_refine_dots and k_pearson_partial; k_pearson_prep_l, _pl, _xl) read pair i's slots and inputs from it instead of from i * pitch.  An index
// outside its pool gives slot 0 and ASX_POOL_INVALID: k_rows_rl writes a NaN Q and a zero bound for it -- every inverse tile of every
// pass leaves at once, whatever the pair's window, zones or seed, so its running maximum stays empty and it can never overflow -- and
// k_invalid_pairs writes (0, NaN, -4) behind the Pearson kernels (top-k: k_invalid_pairs_k, all k entries, behind the last step).
// A PHAT pool group (asx_xcorr_pool_phat_f32_dev) is the same with k_rows_rlp / k_rows_rlb, and k_invalid_pairs also writes a NaN peak.
#define ASX_POOL_INVALID 1u
struct AsxPoolPair {
    uint32_t sx, sy;        // bank slots: source a, sample b (0 for an invalid pair)
    uint32_t flags, pad;    // ASX_POOL_INVALID
    uint64_t src_off;       // a * source_stride: the source's first float in the source pool
    uint64_t smp_off;       // b * sample_stride
};
// what k_pool_resolve reads: the caller's rows (null: every combination, source-major), the pools' sizes and strides, and the
// bank's norm partials and band sums (AsxPeakWs layout: source slot a at operand 0 of "pair" a, sample slot b at operand 1 of b)
struct AsxPoolArgs {
    const int32_t *rows;
    uint64_t first;         // the group's first pair in the call
    uint64_t nsrc, nsmp, src_stride, smp_stride;
    const float *nrm;
    const float2 *band;
};

// Where pair i's inputs are, for the exact passes over float or double inputs: src + i * src_pitch and smp + i * smp_pitch (elements;
// 0 = one track for every pair), or, in a pool call (pl not null, float inputs only), src + pl[i].src_off and smp + pl[i].smp_off
// (the listed kernels).  Host only: asx_with_inputs turns it into the inputs object a launcher hands on to k_refine_dots and
// k_pearson_partial<..., Where>; launch_prep unpacks the pitches or the list for k_pearson_prep's forms.
template <typename TIn> struct AsxInputs {
    const TIn *src, *smp;
    size_t src_pitch, smp_pitch;
    const AsxPoolPair *pl;
};
// Inputs: where pair i's tracks start, in elements from src / smp
struct AsxAtPitch {
    size_t src_pitch, smp_pitch; // 0 = one track for every pair
    __device__ __forceinline__ const AsxPoolPair *list() const { return nullptr; }
    __device__ __forceinline__ size_t src_off(size_t pair) const { return pair * src_pitch; }
    __device__ __forceinline__ size_t smp_off(size_t pair) const { return pair * smp_pitch; }
};
struct AsxAtList {
    const AsxPoolPair *__restrict__ pl;
    __device__ __forceinline__ const AsxPoolPair *list() const { return pl; }
    __device__ __forceinline__ size_t src_off(size_t pair) const { return pl[pair].src_off; }
    __device__ __forceinline__ size_t smp_off(size_t pair) const { return pl[pair].smp_off; }
};
// go(the inputs object of `in`): listed in a pool call (float inputs only), else pitched
template <typename TIn, class F> void asx_with_inputs(const AsxInputs<TIn> &in, F go)
{
    if constexpr (std::is_same<TIn, float>::value) {
        if (in.pl) return go(AsxAtList{ in.pl });
    }
    go(AsxAtPitch{ in.src_pitch, in.smp_pitch });
}

// kernel launchers (defined in xcorr_kernels.hip, called from asx_api.hip)
struct AsxCand {          // one near-maximum lag found by a column tile
    uint32_t idx;
    float key;
};

// per-group scratch of the peak search
struct AsxPeakWs {
    float *nrm_part;       // [pairs][2][ntiles] sum of squares of the samples a k_fwd_cols block loaded
    float *bound2;         // [pairs] 2B: width of the "as large as the maximum" window (k_rows, row 0)
    asx_peak_t *pairmax;   // [pairs] running float32 maximum (atomicMax by the column tiles), zeroed by k_rows
    uint32_t *cand_n;      // [pairs] candidates appended by the tiles (may exceed cap), zeroed by k_rows
    AsxCand *cand;         // [pairs][cap]
    uint32_t *refine_n;    // [pairs] lags to re-evaluate (0 = the float32 argmax stands)
    uint32_t *refine_idx;  // [pairs][cap]
    double *refine_val;    // [pairs][cap] exact r[idx]
    unsigned long long *overflows; // [1] pairs whose candidate list did not fit, cumulative
    uint32_t *over_list;   // [over_cap] or null: indices (pair_base + pair) of those pairs since the list was last emptied --
    uint32_t *over_n;      // [1] ... and their number: what the entry points read to take the second look (asx_api.hip)
    uint32_t *over_host;   // [1] or null: the same count in page-locked HOST memory (system-scope add, only when a pair overflows):
                           // the entry points read it behind a stream synchronisation, with no device-to-host copy in the way
    uint32_t over_cap;
    const double *shift;   // [pairs] or null: c with r[k] = (what the transforms deliver) + c for every k -- the second look at a pair
                           // runs the transforms on (source - mean), see second_look (asx_api.hip); null / 0 everywhere else
    uint32_t cap;          // candidate capacity per pair
    // spectral Pearson (pearson_spectral.hip), both null when the plan does not use it:
    float2 *band;          // [pairs][2][ntiles][nbands] {sum, sum of squares} of the samples of band x tile a k_fwd_cols_r block loaded
                           // (band = AsxDev::band_rows consecutive rows of the [2 M1][M2] sample matrix; the sample fills the first half)
    float *tile_peak;      // [pairs][M2 / T] SIGNED float32 r (times F) at the best lag of each k_inv_cols_r tile
};
// The views of a peak workspace a group's kernels are handed (run_group and second_look, asx_api.hip): the fields a kernel finds
// null are how it is told.  Without the overflow list: k_finalize marks and counts an overflowing pair but lists nothing.
inline AsxPeakWs asx_peak_unlisted(AsxPeakWs W)
{
    W.over_list = nullptr; W.over_n = nullptr; W.over_host = nullptr; W.over_cap = 0;
    return W;
}
// Without the band sums and tile peaks: the transform kernels leave nothing for the spectral Pearson form.
inline AsxPeakWs asx_peak_unbanded(AsxPeakWs W)
{
    W.band = nullptr; W.tile_peak = nullptr;
    return W;
}

// Per-lane workspace of the pruned inverse pass (rlayout.hip: k_rows_re, k_tile_bounds, k_prune_select, k_inv_cols_r<..., AsxSelPrune>)
struct AsxPrune {
    float *eng;            // [pairs][M1 + 1][ntiles] sum of |Q[k1][j2]|^2 over the tile's columns (k_rows_re)
    float *ub;             // [pairs][ntiles] upper bound of |r^| over the tile
    int *best;             // [pairs] the tile with the largest bound
    double *part;          // [pairs][1024] = [slices][tiles rounded up to 32]: a slice's float64 sum over its rows (k_tile_bounds)
    unsigned *ticket;      // [pairs] slices of the pair that have left their sums; zero between launches
    unsigned char *skip;   // [pairs][ntiles] 1 = the second launch leaves the tile out
    unsigned long long *stats; // [2] tiles transformed, tiles in all: cumulative over the plan's life (asx_plan_prune_stats)
    // Partial storing of Q.  list null (a group without it: run_group hands the kernels a copy that says so): Q is whole.
    unsigned long long *list;  // [pairs] the tiles of Q launch B stored (k_q_predict), read by launch B and by the pruned pass of the SAME group
    unsigned char *redo;       // [pairs] 1 = k_prune_select found the stored set short: the pair's results are discarded and it runs again
    unsigned long long *qstats; // [4] pairs given a list, pairs given ASX_Q_ALL, pairs redone (kept by the host), tiles stored; cumulative
    int q_rows, q_row_a;       // the predictor rows: q_rows rows from q_row_a (set per group)
    uint32_t pair_base;        // the group's first pair in the caller's overflow window (set per group)
};

// Selections: the device-side partners of AsxSearch, the last argument of a kernel template <..., Sel>.  Every method is
// __forceinline__: emitted as a function and called, window_of changed the inverse kernels by thousands of instructions.
//   k_inv_cols_r masks: Sel::masks, and sel.window_of(pair, N) is what asx_win_has is asked and whose .seed competes signed --
//   AsxSelAll, AsxWin, AsxWinRows, AsxSelTopk<ZC>, and the pruned pass's AsxSelPrune<FIRST>.
//   k_inv_cols (the packed-sample kernels) the same, with AsxSelTopk<ASX_TOPK_MAX - 1> alone and without the pruned pass.
//   k_finalize and k_refine_pick ask sel.seed_of(pair, N) alone: AsxSelSeed (ALL and WINDOW), AsxWinRows,
//   AsxSelTopkSeed (k_finalize reads the record's flags as well, and takes the sink as a trailing argument).
struct AsxSelAll {
    static constexpr bool masks = false;
    __device__ __forceinline__ AsxWin window_of(size_t, uint32_t) const { return AsxWin{}; }
};
template <int ZC> struct AsxSelTopk { // ZC: the zones the kernel tests
    const AsxTopkPair *__restrict__ X;
    static constexpr bool masks = true;
    __device__ __forceinline__ AsxWinX<ZC> window_of(size_t pair, uint32_t) const { return asx_win_x<ZC>(X, pair); }
};
struct AsxSelSeed {
    uint32_t seed;
    __device__ __forceinline__ uint32_t seed_of(size_t, uint32_t) const { return seed; }
};
struct AsxSelTopkSeed {
    const AsxTopkPair *__restrict__ X;
    __device__ __forceinline__ uint32_t seed_of(size_t pair, uint32_t) const { return X[pair].z.seed; }
};
// The pruned inverse pass (AsxPrune): every lag competes, nothing is dumped (the kernel has no r_out argument), and the block's tile
// is not its place in the grid.  FIRST: grid (npairs, 2) -- y = 0 the pair's largest-bound tile, which holds the peak on all but
// contrived inputs, y = 1 the seed's tile (tile 0: lag 0 competes signed), gone when that is the same tile.  !FIRST: the full grid;
// a block whose flag is set leaves before it asks for anything else.
template <bool FIRST> struct AsxSelPrune {
    const int *__restrict__ best;
    const unsigned char *__restrict__ skip;
    const unsigned long long *__restrict__ list; // partial storing: the pair's stored tiles (null: Q is whole)
    static constexpr bool masks = false;
    __device__ __forceinline__ AsxWin window_of(size_t, uint32_t) const { return AsxWin{}; }
};
// The block's tile, from the tile of its place in the grid (tile width T, rows of M2 columns): asx_sel_takes false = the block
// leaves.  (The pruned pass's are written as they are -- one || and one && -- because that is the shape the kernels they replace
// compiled from: the same tests stated the other way round gave other branches.)
template <class Sel> __device__ __forceinline__ bool asx_sel_takes(const Sel &, int, int, int) { return true; }
template <class Sel> __device__ __forceinline__ int asx_sel_tile(const Sel &, int grid_tile) { return grid_tile; }
template <bool FIRST> __device__ __forceinline__ bool asx_sel_takes(const AsxSelPrune<FIRST> &q, int grid_tile, int M2, int T)
{
    if constexpr (FIRST) {
        // (the largest-bound tile may not be stored: its block leaves at once, k_prune_select then sends the pair round again)
        const int bt = q.best[blockIdx.x];
        if (blockIdx.y == 0) return !q.list || asx_q_stored(q.list[blockIdx.x], bt);
        return bt != 0;
    } else {
        return grid_tile * T < M2 && !q.skip[(size_t)blockIdx.x * (size_t)(M2 / T) + grid_tile];
    }
}
template <bool FIRST> __device__ __forceinline__ int asx_sel_tile(const AsxSelPrune<FIRST> &q, int grid_tile)
{
    if constexpr (FIRST) return blockIdx.y == 0 ? q.best[blockIdx.x] : 0;
    else return grid_tile;
}
// go(the selection object of q).  ZC...: the zone capacities the kernel family's top-k instances are compiled for, ascending, the
// last one ASX_TOPK_MAX - 1 -- a pass runs the first that holds its zones; none: the family asks for the seed alone.
template <int... ZC, class F> void asx_with_selection(const AsxSearch &q, F go)
{
    if constexpr (sizeof...(ZC) == 0) {
        if (q.kind == AsxSearch::TOPK) go(AsxSelTopkSeed{ q.tk });
        else if (q.kind == AsxSearch::ROWS) go(q.rows);
        else go(AsxSelSeed{ q.seed() });
    } else {
        if (q.kind == AsxSearch::TOPK) (void)((q.tk_zones <= ZC && (go(AsxSelTopk<ZC>{ q.tk }), true)) || ...);
        else if (q.kind == AsxSearch::ROWS) go(q.rows);
        else if (q.kind == AsxSearch::WINDOW) go(q.win);
        else go(AsxSelAll{});
    }
}

// Where forward column passes are (real-column plans), and how the pairs of a launch group find theirs: the host's one statement of
// that.  Host only, never a kernel argument: the launchers of rlayout.hip unpack it.
//   As a set of passes -- the lane's workspace, the plan's broadcast slot, the plan's bank -- track t has C_x / C_y at cx / cy +
//   t (M1 + 1) M2 and its norm partials and band sums at slot t of the AsxPeakWs layouts (source: operand 0, sample: operand 1).
//   asx_launch_fwd_cols_r fills tracks of one.
//   As a group's spectra it adds where pair i's rows are: cx + i pitch and cy + i pitch (the lane's workspace); one track for every
//   pair for the operands of `bc` (bit 0: cx, bit 1: cy -- the broadcast slot's, pitch 0); or rows pl[i].sx of cx and pl[i].sy of cy
//   (a pool group: cx / cy are the bank's).  nrm and band are then the group's own places (the lane's), whatever cx / cy are: a
//   broadcast or listed operand's are copied there (k_bcast_aux, k_pool_resolve).
struct AsxSpectra {
    float2 *cx, *cy;
    float *nrm;
    float2 *band;                 // may be null: no band sums
    int bc = 0;
    const AsxPoolPair *pl = nullptr;
};
// How the product spectrum is weighted before the inverse passes (run_group's GroupOpts::weight; the scope rules: asx_group_form).
// ASX_W_PHAT (asx_xcorr_phat_f32_dev): every bin of X conj(Y) divided by its magnitude in the row pass (k_rows_rp), the tiny bound, and
// k_phat_finalize in place of the exactness machinery.  In a pool group (asx_xcorr_pool_phat_f32_dev): the listed forms, k_rows_rlp
// and k_rows_rlb.
// ASX_W_PHAT_BAND (asx_xcorr_phat_band_f32_dev): the same, but only the bins whose frequency min(k, F - k) lies in the band vote
// (k_rows_rb sets the others to zero), and k_phat_finalize divides by the number of voters.  The full band is ASX_W_PHAT.
enum AsxWeight { ASX_W_NONE = 0, ASX_W_PHAT = 1, ASX_W_PHAT_BAND = 2 };
// The band of an ASX_W_PHAT_BAND group, bins of the F = 2N point transform: lo <= min(k, F - k) <= lo + span, lo + span <= N.  Kept
// as the two operands of the kernel's unsigned range compare; passed to k_rows_rb by value.
struct AsxBand {
    uint32_t lo = 0, span = 0;
    // bins k of [0, F) inside: a bin and its mirror both vote, bins 0 and N are their own mirrors
    double votes(uint32_t N) const { return 2.0 * ((double)span + 1.0) - (lo == 0) - (lo + span == N); }
};
// Which row pass a group runs (asx_group_form, plan_math.h), the weight beside it: the packed-sample k_rows; k_rows_r in the broadcast
// form bc (weighted: k_rows_rp / k_rows_rb); k_rows_re, which leaves the tile energies of the pruned pass (or k_rows_rm under partial
// storing); k_rows_rl, C_x / C_y at the pairs' bank slots (weighted: k_rows_rlp / k_rows_rlb).
enum AsxRowFlavour { ASX_ROWS_PACKED, ASX_ROWS_PLAIN, ASX_ROWS_ENERGY, ASX_ROWS_LISTED };
// float2 elements of one track's column spectrum: rows k1 = 0 .. M1 of M2 columns, the pitch between the tracks of a set
inline size_t asx_spectrum_len(const AsxDev &P) { return ((size_t)P.M1 + 1) * (size_t)P.M2; }

// Spectral Pearson: the coefficient from r[peak] and window sums instead of a second pass over the inputs.
// Modes a pair can take (k_pearson_prep decides, k_pearson_partial / k_pearson_final_spec act on it):
#define ASX_PM_FAST 0    // lag >= 0: cross term = r[peak], window sums from the band sums + two band edges; nothing else is read
#define ASX_PM_CORR 1    // lag < 0:  cross term = r[peak] - (wrap-around part, |lag| products, exact), sums as above
#define ASX_PM_DIRECT 2  // the reference's own reduction over the segment (src/cross_correlation.c:74-116): the error bound of the
                         // spectral form is not below the tolerance, or the segment is shorter than the wrap-around part
#define ASX_PM_NMODES 3
#ifndef ASX_PREP_BLOCKS
#define ASX_PREP_BLOCKS 4 // blocks of k_pearson_prep that share a pair's window sums on the long tracks (a function of the plan alone)
#endif
#define ASX_PREP_BLOCKS_MAX 16 // what the workspaces are sized for
#define ASX_SPEC_HDR 4    // per pair: r[peak] (plain sum scale), the bound on its error, 1.0 = "the direct reduction, whatever it yields", the mode k_pearson_partial's block 0 used (read by k_pearson_final_spec)
// What k_pearson_prep leaves and what reads it: the blocks' SHARES of the four window sums and a header -- no merged record.  The mode of a
// pair (asx_spec_pick, xcorr_dev.h: a few dozen float64 operations on 4 * nb + 3 numbers) is worked out again by every block of
// k_pearson_partial and by k_pearson_final_spec: a merge by the last block to arrive cost a device-scope fence per block (28.8 against
// 19.5 us per launch of 124 pairs, profiles/r5_experiments/22_*).
struct AsxSpecWs {
    double *part;          // [pairs][nb][4] the blocks' shares of Sx, Sxx, Sy, Syy, added in block order by whoever reads them
    double *hdr;           // [pairs][ASX_SPEC_HDR]
    unsigned long long *mode_count; // [ASX_PM_NMODES] cumulative
    double tol;            // a pair leaves the spectral form when its error bound exceeds this (1e-5: north_star's tolerance)
    int nb;                // blocks of k_pearson_prep per pair (set by the launcher: 1 or ASX_PREP_BLOCKS)
    uint32_t N;            // sample_len (set by the launcher)
};

// xcorr_kernels.hip: the packed-sample decomposition, each pass on the instance P.kcols / P.krows names
void asx_launch_fwd_cols(const AsxDev &P, const float *src, const float *smp, float2 *zxa,
                         float2 *zya, const AsxPeakWs &W, int npairs, hipStream_t s);
void asx_launch_rows(const AsxDev &P, float2 *zxa, float2 *zya, float2 *ga,
                     const AsxPeakWs &W, int npairs, hipStream_t s);
// q: which flavour of the inverse column kernel runs (AsxSearch)
void asx_launch_inv_cols(const AsxDev &P, const float2 *ga, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                         const AsxSearch &q);
// rlayout.hip: the real-column decomposition (production lengths), each pass on the instance P.kcols / P.krows names.  Which flavour
// of it runs is the group's form (asx_group_form): the row launcher is told, the inverse launcher takes it from the search and from
// U (the AsxPrune of a pruned group, else null), the forward launcher from the operands it is given (null: not that operand) --
// tracks first .. first + count - 1 of each, into the same tracks of dst.
void asx_launch_fwd_cols_r(const AsxDev &P, const float *src, size_t src_stride, const float *smp, size_t smp_stride, size_t first,
                           int count, const AsxSpectra &dst, bool temporal, hipStream_t s);
// rows: ASX_ROWS_PLAIN (C.bc), _LISTED (C.pl) or _ENERGY (U: the group's AsxPrune, whose q_rows > 0 asks for partial storing; null
// otherwise); fband: the band that votes when weight is ASX_W_PHAT_BAND
void asx_launch_rows_r(const AsxDev &P, const AsxSpectra &C, AsxRowFlavour rows, AsxWeight weight, const AsxBand &fband, const AsxPrune *U,
                       float2 *q, const AsxPeakWs &W, int npairs, hipStream_t s);
// partial storing: the predictor rows a pruned group of npairs pairs gets under `mode` (asx_plan_set_qstore), 0 = the group keeps k_rows_re
int asx_qstore_rows(const AsxDev &P, int npairs, int mode);
// behind the Pearson kernels of a group with partial storing: the discarded pass of every pair U.redo marks leaves the counters
void asx_launch_qstore_takeback(const AsxPrune &U, const AsxSpecWs &S, int npairs, hipStream_t s);
void asx_launch_inv_cols_r(const AsxDev &P, const float2 *q, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                           const AsxSearch &search, const AsxPrune *U);
// the tail of a PHAT group (rlayout.hip: k_phat_finalize), behind the inverse column pass and in front of the direct Pearson launch:
// seg from the float32 running maximum alone, refine_n = 0, peak[pair] = |r_phat[lag]| / f (peak may be null); f: the number of bins
// that voted -- F, or AsxBand::votes in a banded group
void asx_launch_phat_finalize(const AsxDev &P, const AsxPeakWs &W, AsxSeg *seg, double *peak, double f, int npairs, hipStream_t s,
                              const AsxSearch &q);
// behind it, when the call asked for the peak's neighbourhood (asx_xcorr_phat_sub_f32_dev; rlayout.hip: k_phat_near): r_phat / f at
// the 2h + 1 indices around seg[pair].peak from the group's whole Q' (q), to near[pair * (2h + 1) ..] (may be null), and the parabolic
// vertex of the three centre values to frac[pair]; 1 <= h <= ASX_NEAR_MAX and 2h + 1 <= P.M2.  find: the pass's search, whose invalid
// rows get NaN; pl: the pool group's records (null: no pool), whose invalid pairs get NaN.  It only reads what the group left.
#define ASX_NEAR_MAX 8
void asx_launch_phat_near(const AsxDev &P, const float2 *q, const AsxSeg *seg, double f, int h, const AsxSearch &find,
                          const AsxPoolPair *pl, double *frac, double *near, int npairs, hipStream_t s);
// The entries of a call of the curve, the lag track or the warped correlation, as their kernels take them, by value.  Entry e = pair *
// entries + j is centred on the lag center[e]; pair i is tracks (i, i) at the strides of the strided form (nsrc == 0), or the tracks
// of row i of `rows` (null: every combination, source-major) in the pool form (nsrc > 0: a pool call with pairs never has an empty
// pool).
struct AsxLagEntries {
    const int64_t *center;  // [batch * entries] lags, the convention of every d_lag
    uint32_t N;
    int entries, h;         // h: the half width, 2 h + 1 values around each centre
    const int32_t *rows;
    uint64_t nsrc, nsmp, src_stride, smp_stride;
};
// The curve around given lags (asx_xcorr_curve_f32_dev, asx_xcorr_pool_curve_f32_dev; xcorr_kernels.hip: k_curve_dots): one call's
// arguments as its kernels take them, by value.
#define ASX_CURVE_N (2 * ASX_NEAR_MAX + 1)
struct AsxCurve {
    AsxLagEntries E;
    double *r;              // [batch * entries][2 h + 1]
    double *frac;           // [batch * entries]
    int32_t *ret;           // [batch * entries]
};
// blocks of k_curve_dots per entry: by the length alone, as asx_pearson_blocks, and as many as leave their ASX_CURVE_N partial sums
// in a pair's share of the lane's psums (6 doubles per Pearson block); one block writes its entry's results itself
unsigned asx_curve_blocks(uint32_t N);
// r and frac (and ret) of entries first .. first + count - 1, count at most a launch group: the pool form's records go to pl (the
// lane's, [count]), the blocks' partial sums to part (the lane's psums)
void asx_launch_curve_r(const float *src, const float *smp, const AsxCurve &A, size_t first, int count, AsxPoolPair *pl, double *part,
                        hipStream_t s);
// the coefficient curve's virtual pairs first .. first + count - 1 (virtual pair e (2 h + 1) + d + h: entry e at its neighbour d),
// count at most a launch group: each one's segment to seg and its tracks' offsets to pl, what asx_launch_pearson's listed form reads.
// An invalid entry's get an empty segment at offset 0: nothing is read and the coefficient is NaN.
void asx_launch_curve_segs(const AsxLagEntries &E, size_t first, int count, AsxSeg *seg, AsxPoolPair *pl, hipStream_t s);
// The lag track (asx_xcorr_track_f32_dev, asx_xcorr_pool_track_f32_dev; xcorr_kernels.hip: k_track_dots, k_track_fit): one call's
// arguments as its kernels take them, by value.  S time segments, segment s the sample's frames [floor(s N / S), floor((s + 1) N / S)).
#define ASX_TRACK_HALF_MAX 64
#define ASX_TRACK_SEG_MAX 64
struct AsxTrack {
    AsxLagEntries E;
    int S;
    double *r;              // [batch * entries][S][2 h + 1]
    double *seg;            // [batch * entries][S][2] {off, w}, or null
    double *fit;            // [batch * entries][3] {drift, lag0, rms}
    int32_t *used;          // [batch * entries]
    int32_t *ret;           // [batch * entries]
};
// blocks of k_track_dots per (segment, lag tile): floor(asx_curve_blocks(N) / (S * tiles)), tiles = ceil((2h + 1) / ASX_CURVE_N), so
// that an entry's partial sums fit its share of the lane's psums as the curve's do; at least one, which writes its values itself.
// By N, S and h alone: the reduction tree of an entry does not depend on the batch or the plan's max_batch.
unsigned asx_track_blocks(uint32_t N, int segments, int half_width);
// every output of entries first .. first + count - 1, count at most a launch group: the pool form's records go to pl (the lane's,
// [count]), the blocks' partial sums to part (the lane's psums); k_track_fit runs last and owns an invalid entry's outputs
void asx_launch_track(const float *src, const float *smp, const AsxTrack &A, size_t first, int count, AsxPoolPair *pl, double *part,
                      hipStream_t s);
// The warped correlation (asx_xcorr_warp_f32_dev, asx_xcorr_pool_warp_f32_dev; xcorr_kernels.hip: k_warp_dots, k_warp_final): one
// call's arguments as its kernels take them, by value.  Entry e's line is {line[e * line_stride], line[e * line_stride + 1]} =
// {drift a, lag0 b}: sample frame n meets source frame n + centre + k_n, k_n = floor((b + a n) + 0.5).
#define ASX_WARP_DRIFT_MAX 0.015625
struct AsxWarp {
    AsxLagEntries E;
    const double *line;     // entry e's {a, b} at e * line_stride
    uint64_t line_stride;   // in doubles: 0, 2, 3, ...
    double *r;              // [batch * entries][2 h + 1]
    double *frac;           // [batch * entries]
    double *coef;           // [batch * entries]
    int64_t *len;           // [batch * entries], or null
    int32_t *ret;           // [batch * entries]
};
// blocks of k_warp_dots per entry: by the length alone, as asx_curve_blocks, and as many as leave their ASX_CURVE_N partial sums and
// their Pearson record (6 doubles) in a pair's share of the lane's psums; one block leaves its sums in r and its record in part[le * 6]
unsigned asx_warp_blocks(uint32_t N);
// every output of entries first .. first + count - 1, count at most a launch group: the pool form's records go to pl (the lane's,
// [count]), the blocks' partial sums and records to part (the lane's psums); k_warp_final runs last and owns an invalid entry's outputs
void asx_launch_warp(const float *src, const float *smp, const AsxWarp &A, size_t first, int count, AsxPoolPair *pl, double *part,
                     hipStream_t s);
void asx_launch_bcast_aux(const AsxDev &P, const float *snrm, const float2 *sband, float *nrm, float2 *band, int npairs,
                          unsigned which, hipStream_t s);
// pool calls: each pair's record (out) and its two slots' norm partials and band sums (band may be null) into the group's places
void asx_launch_pool_resolve(const AsxDev &P, const AsxPoolArgs &A, AsxPoolPair *out, float *nrm, float2 *band, int npairs,
                             hipStream_t s);
// behind the Pearson kernels of a pool group: (0, NaN, -4) for every pair flagged ASX_POOL_INVALID, and NaN in peak (null but in a
// PHAT pool group)
void asx_launch_invalid_pairs(const AsxPoolPair *pl, int64_t *lag, double *coef, int32_t *ret, double *peak, int npairs, hipStream_t s);
// the same behind the last k_topk_step of a pool group with top-k: all k entries of such a pair (entry stride k; peak: null but in a
// PHAT pool group that was asked for the heights)
void asx_launch_invalid_pairs_k(const AsxPoolPair *pl, int k, int64_t *lag, double *coef, int32_t *ret, double *peak, int npairs,
                                hipStream_t s);
void asx_launch_finalize(const AsxDev &P, const AsxPeakWs &W, AsxSeg *seg, int npairs, hipStream_t s, uint32_t pair_base,
                         const AsxSearch &q);
// behind the Pearson kernels of pass j of a top-k group: entry j of the caller's arrays (entry stride k) from the pass's results,
// then pass j + 1's records (call: the call's own search, pass 0's -- the plan's window, used when it has no rows)
void asx_launch_topk_step(AsxTopkWs T, const AsxSeg *seg, const AsxPeakWs &W, const AsxSearch &call, uint32_t N, int npairs, int j,
                          int k, int64_t sep, int64_t *lag, double *coef, int32_t *ret, hipStream_t s);
// in FRONT of that step in a PHAT top-k group (k_topk_peak): entry j's peak height (entry stride k) from the pass's running maximum,
// which the step zeroes -- per voter (f: what asx_launch_phat_finalize takes), NaN where the step writes -2 or -3; peak is not null
void asx_launch_topk_peak(const AsxTopkWs &T, const AsxPeakWs &W, const AsxSearch &call, uint32_t N, int npairs, int j, int k, double f,
                          double *peak, hipStream_t s);
// behind the Pearson kernels of a group with per-pair windows: (lag, coef, ret) = (0, NaN, -2) for every pair whose row is invalid
void asx_launch_invalid_rows(const AsxWinRows &rows, uint32_t N, int64_t *lag, double *coef, int32_t *ret, int npairs, hipStream_t s);
// The exact passes over float or double inputs (instances for both next to the kernels, xcorr_kernels.hip).
// refine: pick = false: the exact values only; the caller's next kernel applies the rule (k_pearson_prep)
template <typename TIn>
void asx_launch_refine(const AsxDev &P, const AsxInputs<TIn> &in, const AsxPeakWs &W, AsxSeg *seg, int npairs, hipStream_t s,
                       int dot_blocks, bool pick, const AsxSearch &q);
template <typename TIn>
void asx_launch_pearson(const AsxInputs<TIn> &in, uint32_t basis_len, const AsxSeg *seg, double *psums, int64_t *lag, double *coef,
                        int32_t *ret, int npairs, hipStream_t s);
// the partial-sum kernel alone (the spectral form runs it on its own segment list, pearson_spectral.hip)
void asx_launch_pearson_partial_spec_f32(const AsxInputs<float> &in, uint32_t basis_len, const AsxSeg *seg, const AsxSpecWs &S,
                                         double *psums, int npairs, hipStream_t s);
// pearson_spectral.hip: float32 inputs, real-column plans (W.band and W.tile_peak filled by this group's transform kernels)
void asx_launch_pearson_spectral_f32(const AsxDev &P, const AsxInputs<float> &in, const AsxSearch &q, const AsxPeakWs &W,
                                     const AsxSpecWs &S, AsxSeg *seg, double *psums, int64_t *lag, double *coef, int32_t *ret,
                                     int npairs, hipStream_t s);
// diagnostic: asx_spec_pick of `pair` on the device, out (device, 8 doubles) = {mode, n, Sx, Sxx, Sy, Syy, r, bound}; returns the
// blocks of k_pearson_prep per pair (the shares AsxSpecWs::part holds for it)
int asx_launch_debug_spec_pick(const AsxDev &P, const AsxSpecWs &S, const AsxSeg *seg, size_t pair, double *out, hipStream_t s);
void asx_launch_results_to_ms(const int64_t *lag, const double *coef, const int32_t *ret, size_t batch,
                              double min_confidence, double sample_rate, int64_t *lag_ms, int32_t *accept,
                              hipStream_t s);
// asx_topk_best_dev: per pair the entry with ret == 0 and the largest signed coefficient (none: entry 0), to index pair
void asx_launch_topk_best(const int64_t *lag, const double *coef, const int32_t *ret, size_t batch, int k, int64_t *best_lag,
                          double *best_coef, int32_t *best_ret, int32_t *best_entry, hipStream_t s);
// asx_pool_closure_dev over the [C][C][k] tables of one pool (C * C * k <= INT32_MAX, 1 <= k <= ASX_TOPK_MAX, 0 <= tol <=
// ASX_CLOSURE_LAG_MAX): k_closure_votes (votes, may be NULL, and the pick to best_*), k_closure_confirm, k_closure_root (root in
// [0, C) or -1: chosen), k_closure_offsets -- four launches in this order on s, each reading the outputs of those before it
// ASX_CLOSURE_LAG_LIMIT: the kernels' copy of ASX_CLOSURE_LAG_MAX of include/audiosync/xcorr_hip.h, which this header does not
// include; asx_api.hip includes both and holds them together with a static_assert (tests/test_closure.py reads both too)
#define ASX_CLOSURE_LAG_LIMIT ((int64_t)1 << 40)
void asx_launch_pool_closure(const int64_t *lag, const double *coef, const int32_t *ret, uint32_t C, int k, int64_t tol,
                             int min_confirm, int root, int32_t *votes, int64_t *best_lag, double *best_coef, int32_t *best_ret,
                             int32_t *best_entry, int32_t *confirm, int32_t *d_root, int64_t *offset, int32_t *support,
                             int32_t *placed, hipStream_t s);
// asx_pool_place_dev over the picked [C][C] tables of that call (C * C <= INT32_MAX, 0 <= tol <= ASX_CLOSURE_LAG_MAX, 1 <= max_hops,
// 0 <= sweeps; scratch may be NULL when sweeps == 0), place.hip: k_place_init, max_hops times k_place_layer, sweeps times
// k_place_sweep, k_place_verdict -- 2 + max_hops + sweeps launches on s whatever the tables hold; the root is read on the device
void asx_launch_pool_place(const int64_t *lag, const int32_t *ret, const int32_t *confirm, uint32_t C, int64_t tol, int min_confirm,
                           const int32_t *d_root, int max_hops, int sweeps, int64_t *scratch, int64_t *offset, int32_t *hops,
                           int32_t *support, int32_t *degree, int64_t *step, int64_t *resid, int32_t *state, hipStream_t s);
// Normalised cross-correlation (asx_xcorr_ncc_f32_dev; the k_ncc_* kernels, ncc.hip).  A track is cut into chunks of ASX_NCC_CHUNK
// frames and the lags 0..N-1 into chunks of as many lags: the reduction trees follow from N alone.  The workspace of one NCC group
// (plan-owned, lazy, whole or absent: asx_plan::Ncc): nsrc source and nsmp sample tracks -- the group's pairs, or 1 for the call's
// broadcast track, whose moments the call's first group computes (do_src / do_smp) and the later ones read.
#define ASX_NCC_CHUNK 2048
#define ASX_NCC_STAT 4 // doubles per track: {mu, Vmax (source), Sy, Vy (sample)}
__host__ __device__ inline uint32_t asx_ncc_chunks(uint32_t frames) { return (frames + ASX_NCC_CHUNK - 1) / ASX_NCC_CHUNK; }
// a row of this call: 0 <= lag_min <= lag_max <= N-1
__host__ __device__ inline bool asx_ncc_row_ok(int64_t lo, int64_t hi, uint32_t N) { return 0 <= lo && lo <= hi && hi <= (int64_t)N - 1; }
// A pair's record in the top-k NCC calls (asx_xcorr_ncc_topk_f32_dev): the lags of the entries decided so far, whose zones the next
// pass leaves out, and the entry whose coefficient the direct Pearson pass is forming (k_ncctop_step writes and reads it, k_ncctop_scan
// reads the lags).
#define ASX_NCC_TK_EMPTY 1u   // A_j is empty from entry `n` on: (0, NaN, NaN, -3)
#define ASX_NCC_TK_INVALID 2u // the pair's row is not a row of the call: every entry is (0, NaN, NaN, -2)
struct AsxNccTopk {
    int64_t lag[ASX_TOPK_MAX]; // entries 0 .. n - 1
    double peak;               // of entry n - 1
    uint32_t n, flags;
};
struct AsxNccWs {
    float *r;              // [pairs][2N] what the group's inverse pass left (run_group's r_out); a top-k group keeps c32 of the lags
                           // 0..N-1 in the upper half (the negative lags, which no NCC kernel reads) behind k_ncc_peak
    double2 *table;        // [nsrc][N] per lag {Sx' = sum of the window's frames minus mu, Vx}
    double *raw, *m1, *m2; // chunk sums: source track t's at t * chunks(2N), sample track t's behind all of them at t * chunks(N)
    double *sstat, *ystat; // [nsrc][ASX_NCC_STAT], [nsmp][ASX_NCC_STAT]
    asx_peak_t *best;      // [pairs] the packed (|c32|, smallest lag) maximum; 0: no lag competes
    AsxNccTopk *tk;        // [pairs] the top-k calls' records
    uint32_t nsrc, nsmp;
    bool do_src, do_smp;
};
// the moments of the group's tracks (those of do_src / do_smp): k_ncc_sums, k_ncc_moments, k_ncc_table
void asx_launch_ncc_moments(const AsxNccWs &W, const float *src, size_t src_pitch, const float *smp, size_t smp_pitch, uint32_t N,
                            hipStream_t s);
// the same over the tracks of two pools (asx_xcorr_pool_ncc_f32_dev), once per call: T holds the plan's track set (table, chunk sums
// and statistics of nsrc source and nsmp sample tracks); at most 65 535 tracks per launch (grid.y), each launch on its own share
void asx_launch_ncc_pool_moments(const AsxNccWs &T, const float *srcs, size_t src_pitch, size_t nsrc, const float *smps, size_t smp_pitch,
                                 size_t nsmp, uint32_t N, hipStream_t s);
// k_ncc_peak and k_ncc_finalize: each pair's winner among the lags of its row (rows null: 0..N-1) to seg and peak; c_out: null, or
// c32 of every lag ([pairs][N], NaN where the lag does not compete); scale: what r carries against the plain sum (F).  pl: null, or
// a pool group's records, whose slots name each pair's table and statistics (W.table, W.sstat, W.ystat: the plan's track set).
// k > 1 (a top-k group): c32 goes to the upper half of each pair's r instead, k_ncc_finalize does not run and seg and peak are left
// alone: asx_launch_ncctop_step(j = 0) takes the pass's winner from W.best.
void asx_launch_ncc_peak(const AsxNccWs &W, const float *r, size_t r_pitch, uint32_t N, double scale, double min_energy,
                         const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak, int npairs, hipStream_t s,
                         const AsxPoolPair *pl = nullptr, int k = 1);
// pass j >= 1 of a top-k group (k_ncctop_scan): the packed maximum over c32 as pass 0 left it in the upper half of r, among the lags
// of the row that lie outside the zones +- sep around the record's j earlier entries, to W.best
void asx_launch_ncctop_scan(const AsxNccWs &W, size_t r_pitch, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j,
                            int npairs, hipStream_t s);
// between the passes of a top-k group (k_ncctop_step), a thread per pair, 0 <= j <= k.  j > 0: entry j - 1 (entry stride k) from the
// direct Pearson pass's results in tmp_* and the record's peak, or (0, NaN, NaN, -3 / -2).  j < k: entry j from W.best -- the winner,
// or the smallest lag of A_j with peak 0, or A_j is empty -- to the record and seg, and W.best back to 0.
void asx_launch_ncctop_step(const AsxNccWs &W, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j, int k, AsxSeg *seg,
                            const int64_t *tmp_lag, const double *tmp_coef, const int32_t *tmp_ret, int64_t *lag, double *coef,
                            double *peak, int32_t *ret, int npairs, hipStream_t s);
// behind the Pearson kernels: (0, NaN, NaN, -2) for every pair whose row is not a row of this call
void asx_launch_ncc_invalid(uint32_t N, const int64_t *rows, size_t rows_step, int64_t *lag, double *coef, double *peak, int32_t *ret,
                            int npairs, hipStream_t s);
// Full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev; the k_nccfull_* kernels, ncc.hip): the lags -(N-1)..N-1, as
// the indices i = l + N - 1 of one curve of 2N - 1 values (the smallest index is the smallest lag).  The lags >= 0 are the NCC call's
// in every bit: W holds what that call's group holds, filled by the same kernels (pass A).  A lag l < 0 overlaps in m = N + l frames,
// source[0, m) against sample[N - m, N): its r comes from a second correlation (pass B) of the sample against the staged source x_lo
// (the first N frames, then zeros: nothing wraps around), its sums from prefix tables over the source and suffix tables over the sample.
struct AsxNccFullWs {
    float *rlo;    // [pairs][2N] r of (x_lo, y): index 2N + l = N + m holds the m products of lag l; the indices 0..N are read by nobody
    float *stage;  // [nsrc][pitch] x_lo of the group's source tracks (the call's one broadcast track: staged by its first group)
    size_t pitch;  // 2N rounded up to whole 16-byte vectors
    double2 *ptab; // [nsrc][N] at index m = 1..N-1: {P1[m] = sum_{n<m} (x[n] - mu), Vx of x[0, m)}
    double2 *ttab; // [nsmp][N] at index m = 1..N-1: {T1[m] = sum_{n>=N-m} (y[n] - mean y), Vy of y[N - m, N)}
};
// a row of the full-range calls: -(N-1) <= lag_min <= lag_max <= N-1
__host__ __device__ inline bool asx_nccfull_row_ok(int64_t lo, int64_t hi, uint32_t N)
{
    return -((int64_t)N - 1) <= lo && lo <= hi && hi <= (int64_t)N - 1;
}
// k_nccfull_stage: x_lo of W.nsrc source tracks (src_pitch apart) into F.stage
void asx_launch_nccfull_stage(const AsxNccFullWs &F, const float *src, size_t src_pitch, uint32_t nsrc, uint32_t N, hipStream_t s);
// k_nccfull_prefix, behind asx_launch_ncc_moments on the same W and tracks (it starts from the chunk sums m1 / m2 and the means that
// those kernels left): F.ptab of the source tracks (W.do_src) and F.ttab of the sample tracks (W.do_smp)
void asx_launch_nccfull_prefix(const AsxNccWs &W, const AsxNccFullWs &F, const float *src, size_t src_pitch, const float *smp,
                               size_t smp_pitch, uint32_t N, hipStream_t s);
// k_nccfull_peak and k_nccfull_finalize: asx_launch_ncc_peak over the signed curve.  rows under asx_nccfull_row_ok (null: every lag);
// a lag l < 0 competes only with an overlap of at least min_overlap frames.  c_out: null, or c32 of one pair's 2N - 1 lags.  k > 1: the
// curve stays in the halves of the two r buffers that nothing reads (index i < N - 1 at F.rlo[i], the others at W.r[i + 1]),
// k_nccfull_finalize does not run and asx_launch_nccfull_step(j = 0) takes the winner from W.best.
void asx_launch_nccfull_peak(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, double scale, double min_energy,
                             int64_t min_overlap, const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak,
                             int npairs, hipStream_t s, int k = 1);
// asx_launch_ncctop_scan / asx_launch_ncctop_step over the signed curve: the records hold indices, the zones do not wrap
void asx_launch_nccfull_scan(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, const int64_t *rows, size_t rows_step,
                             int64_t sep, int j, int npairs, hipStream_t s);
void asx_launch_nccfull_step(const AsxNccWs &W, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j, int k, AsxSeg *seg,
                             const int64_t *tmp_lag, const double *tmp_coef, const int32_t *tmp_ret, int64_t *lag, double *coef,
                             double *peak, int32_t *ret, int npairs, hipStream_t s);
void asx_launch_nccfull_invalid(uint32_t N, const int64_t *rows, size_t rows_step, int64_t *lag, double *coef, double *peak,
                                int32_t *ret, int npairs, hipStream_t s);
// The pool form (asx_xcorr_pool_ncc_full_f32_dev).  Behind asx_launch_ncc_pool_moments on the same pools and the same track set T:
// x_lo of every source track into F.stage (k_nccfull_stage), F.ptab of every source and F.ttab of every sample track
// (k_nccfull_prefix), F being the plan's full-range track set (its rlo is not touched); at most 65 535 tracks per launch, in
// asx_launch_ncc_pool_moments' shares.
void asx_launch_nccfull_pool_tracks(const AsxNccWs &T, const AsxNccFullWs &F, const float *srcs, size_t src_pitch, size_t nsrc,
                                    const float *smps, size_t smp_pitch, size_t nsmp, uint32_t N, hipStream_t s);
// k_nccfp_peak and k_nccfull_finalize: asx_launch_nccfull_peak for a pool group -- W.table, W.sstat, W.ystat, F.ptab and F.ttab are
// the track sets', indexed by the slots of pl, the group's records; W.r, F.rlo, W.best and W.tk are the group's.  The scan, step and
// invalid launches behind it are the strided call's.
void asx_launch_nccfp_peak(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, double scale, double min_energy,
                           int64_t min_overlap, const int64_t *rows, size_t rows_step, AsxSeg *seg, double *peak, int npairs,
                           hipStream_t s, const AsxPoolPair *pl, int k = 1);
// Ragged NCC (asx_xcorr_ncc_ragged_f32_dev; the k_nccrag_* kernels, ncc.hip): the full-range curve of 2N - 1 indices for a pair whose
// tracks hold Ls <= 2N and Lm <= N frames.  Every pair has staged copies of its own (x' = x[0, Ls) then zeros, x_lo' = x[0, min(Ls, N))
// then zeros, y' = y[0, Lm) then zeros), which the two transform passes read, and prefix tables over the frames that count.
// A pair's lengths: row {Ls, Lm} at rows + 2 * pair * step in device memory (step 0: one row for every pair), or, rows null, (ls, lm).
struct AsxRagLens {
    const int64_t *rows;
    size_t step;
    int64_t ls, lm;
};
// a row that is no pair of lengths (false) counts as (0, 0): nothing of its tracks is read and no lag exists
__host__ __device__ inline bool asx_nccrag_lens(const AsxRagLens &L, size_t pair, uint32_t N, uint32_t &Ls, uint32_t &Lm)
{
    const int64_t a = L.rows ? L.rows[2 * pair * L.step] : L.ls, b = L.rows ? L.rows[2 * pair * L.step + 1] : L.lm;
    const bool ok = 1 <= a && a <= 2 * (int64_t)N && 1 <= b && b <= (int64_t)N;
    Ls = ok ? (uint32_t)a : 0u;
    Lm = ok ? (uint32_t)b : 0u;
    return ok;
}
struct AsxNccRagWs {
    float *xs, *xlo;       // [pairs][xpitch] x' and x_lo'
    float *ys;             // [pairs][ypitch] y'
    size_t xpitch, ypitch; // 2N and N rounded up to whole 16-byte vectors
    float *r, *rlo;        // [pairs][2N] r of (x', y') and of (x_lo', y'); a top-k group keeps the curve where the full-range call does
    double2 *pa;           // [pairs][2N + 1] {PA1[j], PA2[j]} = sums of (x[n] - mu) and its square over n < j, j = 0..Ls
    double2 *pb;           // [pairs][N + 1] the same over y - my, j = 0..Lm
    double *raw, *m1, *m2; // chunk sums: pair i's source chunks at i * (chunks(2N) + chunks(N)), its sample chunks behind them
    double *stat;          // [pairs][ASX_NCC_STAT] {mu, Vmax, my, -}
    asx_peak_t *best;      // [pairs]
    AsxNccTopk *tk;        // [pairs]
};
// k_nccrag_stage, k_nccrag_moments, k_nccrag_prefix, k_nccrag_vmax: the staged copies, means, prefix tables and Vmax of npairs pairs
void asx_launch_nccrag_tracks(const AsxNccRagWs &R, const AsxRagLens &L, const float *src, size_t src_pitch, const float *smp,
                              size_t smp_pitch, uint32_t N, int npairs, hipStream_t s);
// k_nccrag_peak and k_nccrag_finalize: asx_launch_nccfull_peak for ragged pairs (seg: the overlap of the winner's lag in the caller's
// tracks).  k > 1: the curve stays where k_nccfull_scan reads it and k_nccrag_finalize does not run.
void asx_launch_nccrag_peak(const AsxNccRagWs &R, const AsxRagLens &L, uint32_t N, double scale, double min_energy, int64_t min_overlap,
                            const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak, int npairs, hipStream_t s,
                            int k = 1);
// behind asx_launch_nccfull_step(j) of a ragged top-k group (k_nccrag_seg): entry j's segment by the pair's lengths, an empty one where
// the entry is not to be
void asx_launch_nccrag_seg(const AsxNccRagWs &R, const AsxRagLens &L, uint32_t N, int j, AsxSeg *seg, int npairs, hipStream_t s);
// last of a group (k_nccrag_invalid): (0, NaN, NaN, -5) in all k entries of every pair whose row is no pair of lengths
void asx_launch_nccrag_invalid(const AsxRagLens &L, uint32_t N, int k, int64_t *lag, double *coef, double *peak, int32_t *ret, int npairs,
                               hipStream_t s);
void asx_launch_cvt_f64_f32(const double *in, float *out, size_t n, hipStream_t s);
unsigned asx_pearson_blocks(uint32_t basis_len); // partial blocks per pair: psums holds 6 doubles per block and pair
// second look, DC removal: stats[0] = mean of source[0..2N), stats[1] = sum of sample[0..N), stats[2] = scale * stats[0] * stats[1]
// (scale = F: the device's r is F times the plain sum of products); out[i] = (float)(source[i] - stats[0]); stats holds
// ASX_DC_STATS_DOUBLES doubles
template <typename TIn>
void asx_launch_dc_remove(const TIn *src, const TIn *smp, uint32_t N, double scale, double *stats, float *out, hipStream_t s);
void asx_launch_synth(uint64_t seed, uint64_t first_pair, size_t count, uint32_t N,
                      int noise_shift, float *src, float *smp, int64_t *true_lag, hipStream_t s);
