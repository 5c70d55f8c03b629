// csrc/rlayout.hip -- the "real-column" decomposition of the cross-correlation path (production lengths).
//
// Same plan (F = 2N real samples, M = F/2 = M1*M2, the same twiddle tables and LDS engine) as xcorr_kernels.hip,
// different assignment of the real-input symmetry:
//
//   xcorr_kernels.hip  packs ADJACENT SAMPLES as complex (z[j] = x[2j] + i x[2j+1]); the k <-> M-k partners of the
//                      real-FFT untangling then sit in two different spectrum rows, so k_rows holds four rows per
//                      block and spends a phase (and its LDS passes) on the combine.
//   here               the real sequence is the matrix x[j1][j2], j = j1*M2 + j2, with 2*M1 rows of M2 samples.  The
//                      column transforms (over j1, length 2*M1, REAL input) are r2c transforms done inside the tile:
//                      rows 2m and 2m+1 are packed as one complex row, an M1-point complex transform runs in LDS and
//                      the untangling k1 <-> M1-k1 happens between slots of the SAME tile (k_fwd_cols_r).  What
//                      reaches HBM is C[k1][j2] for k1 = 0 .. M1 (M1+1 rows; the other half is its mirror image).
//                      Every row k1 is then an independent complex problem:
//                          X[k1 + 2*M1*k2] = DFT_M2( C[k1][.] * w_F^(k1 j2) )[k2]
//                      so k_rows_r takes ONE row of each spectrum per block (19.2 KB of LDS instead of 38.4: eight
//                      blocks of two waves per CU instead of four of four), multiplies X conj(Y)
//                      (src/cross_correlation.c:232-233) in the registers of the last forward stage -- no combine
//                      phase, no partner rows, no index tables -- and runs the inverse row transform on the single
//                      product row.  k_inv_cols_r undoes the column step: c2r of length 2*M1 from the M1+1 rows, with
//                      the tangling inside the tile, and searches the peak as k_inv_cols does.
//
// Algebra (checked in tests/model_fourstep.py::rlayout_*): with j = j1*M2 + j2 and k = k1 + 2*M1*k2,
//   forward  C[k1][j2]  = sum_j1 x[j1][j2] w_{2M1}^(j1 k1)                         (k_fwd_cols_r, k1 = 0..M1)
//            X[k]       = sum_j2 C[k1][j2] w_F^(k1 j2) w_M2^(j2 k2)                (k_rows_r)
//   inverse  Q[k1][j2]  = conj(w_F^(k1 j2)) sum_k2 P[k1 + 2M1 k2] conj(w_M2^(j2 k2)) (k_rows_r)
//            r[j1][j2]  = sum_{k1 < 2M1} Q[k1][j2] conj(w_{2M1}^(j1 k1)),  Q[2M1-k1] = conj Q[k1]   (k_inv_cols_r)
// r is F times the plain sum of products, like the other path (asx_api.hip: bound_scale).
//
// Replaces FFTW's r2c / c2r work of src/cross_correlation.c:34-39,237-239 and the scan of :52-67, :242.
#include "asx_internal.h"
#include "lds_fft.h"
#include "xcorr_dev.h"
#include "kernel_table.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <stdlib.h>

extern __shared__ __attribute__((aligned(16))) float2 asx_lds_r[];

// Diagnostic phase clocks (never in a shipped build; -DASX_STAMPS, tools/dbg/stamps_r.py): lane 0 of a block records the
// clock at phase boundaries into a buffer nothing else reads (kernel 0 = rows, 1 = forward columns, 2 = inverse columns).
#ifdef ASX_STAMPS
#define RSTAMP(kernel, block, slot)                                                                  \
    do {                                                                                             \
        if (P.stamps && P.stamp_kernel == (kernel) && threadIdx.x == 0)                              \
            P.stamps[(size_t)(block) * 8 + (slot)] = clock64();                                      \
    } while (0)
#else
#define RSTAMP(kernel, block, slot) do {} while (0)
#endif

// What these kernels need from the plan, BY VALUE in the kernel arguments.  Read through the plan pointer (as the
// packed-sample kernels do) a block starts with a chain of dependent latencies -- plan struct (scalar loads) -> table
// pointers -> twiddle lookups, and in the inverse column kernel a bound load + branch before the tile loads were even
// issued: 4-5 k cycles, a fifth of a block's life (tools/dbg/stamps_r.py, round 4).  No arrays in here: nothing the
// compiler would index dynamically and send to scratch.
struct RArgs {
    const float2 *tw1, *tw2, *tw_lo, *tw_hi;
    uint32_t N, nout;
    int M1, M2, ntiles;
    float bound_scale;
    unsigned long long *stamps;
    int stamp_kernel;
};
static RArgs rargs_of(const AsxDev &P)
{
    RArgs a;
    a.tw1 = P.tw1; a.tw2 = P.tw2; a.tw_lo = P.tw_lo; a.tw_hi = P.tw_hi;
    a.N = P.N; a.nout = P.nout; a.M1 = P.M1; a.M2 = P.M2; a.ntiles = P.ntiles; a.bound_scale = P.bound_scale;
    a.stamps = P.stamps; a.stamp_kernel = P.stamp_kernel;
    return a;
}
// w_F^p from the two-level table (xcorr_dev.h's tw_F on the argument block)
__device__ __forceinline__ float2 tw_F(const RArgs &P, uint32_t p)
{
    const float2 lo = P.tw_lo[p & (ASX_TW_LO - 1u)];
    const float2 hi = P.tw_hi[p >> ASX_TW_LOG];
    return cmul(lo, hi);
}

// single-member values live in the first 8 bytes of a 16-byte slot: the wave-local stages rewrite exactly the
// slots they read, so no other wave's data is ever touched
__device__ __forceinline__ Cx1 lds_get1(const float4 *p)
{
    const float2 x = *reinterpret_cast<const float2 *>(p);
    return Cx1{ x.x, x.y };
}
__device__ __forceinline__ void lds_put1(float4 *p, Cx1 v) { *reinterpret_cast<float2 *>(p) = make_float2(v.re, v.im); }

__device__ __forceinline__ void wave_lds_sync()
{
    // same wave: the next stage reads what this one wrote (LDS executes a wave's operations in order; the
    // explicit wait does not lean on that)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Diagnostic builds only (tools/mkr.sh; never defined in the shipped library):
//   -DASX_EXP_PAIRMOD=<m>   every pair of a launch uses the C / Q workspaces of pair (pair % m): wrong results, the traffic
//                           of a launch whose intermediates never leave the 256 MiB Infinity Cache (upper bound of keeping
//                           them on die, EXPERIMENTS.md)
//   -DASX_ROWS2_SCHED=a,b,c the radix schedule of the 1200-point sub-rows of the two-half row kernel (kernel_table.h)
// sum over the four lanes of a quad (every lane gets it): two DPP steps
__device__ __forceinline__ float quad_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true)); // quad_perm [2,3,0,1]
    return v;
}
// sum over a DPP row of sixteen lanes (every lane gets it): the balanced tree tree_sum<16> is, ((0+1)+(2+3))+((4+5)+(6+7)) + the same of 8..15
__device__ __forceinline__ float row16_sum(float v)
{
    v = quad_sum(v);
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true)); // row_half_mirror: the other quad of the eight
    v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true)); // row_mirror: the other eight
    return v;
}
// p[0] + ... + p[N-1] as a balanced tree: ceil(log2 N) roundings on every path
template <int N> __device__ __forceinline__ float tree_sum(const float (&p)[N])
{
    if constexpr (N == 1) return p[0];
    else {
        float q[(N + 1) / 2];
        static_for<0, N / 2>([&](auto I) __attribute__((always_inline)) { q[I] = p[2 * decltype(I)::value] + p[2 * decltype(I)::value + 1]; });
        if constexpr (N & 1) q[N / 2] = p[N - 1];
        return tree_sum<(N + 1) / 2>(q);
    }
}

#ifdef ASX_EXP_PAIRMOD
#define RWS_PAIR(pair) ((pair) % (ASX_EXP_PAIRMOD))
#else
#define RWS_PAIR(pair) (pair)
#endif
// Non-temporal accesses for everything these kernels touch exactly once between its producer and its consumer: C written by
// k_fwd_cols_r (2) and read by k_rows_r (4), Q written by k_rows_r (8) and read by k_inv_cols_r (1).  All four together,
// same box, six alternating rounds: forward columns 1.019 -> 0.992 ms, rows 0.944 -> 0.926, inverse columns 0.325 -> 0.306,
// 51.6 -> 53.1 k/s (profiles/r5_experiments/10_*; the row LOADS alone slow the inverse kernel by 10 %: all or none).  The inputs stay
// temporal: the two tiles of a 128-byte input line meet in one XCD's L2 (rcol_tile_of_block); non-temporal, 0.987 -> 1.000 ms.
#ifndef ASX_RNT
#define ASX_RNT 15
#endif
typedef float asx_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_f4(const void *p, bool nt)
{
    if (nt) { const asx_f4v v = __builtin_nontemporal_load(reinterpret_cast<const asx_f4v *>(p)); return make_float4(v.x, v.y, v.z, v.w); }
    return *reinterpret_cast<const float4 *>(p);
}
__device__ __forceinline__ void st_f4(void *p, float4 v, bool nt)
{
    if (nt) { asx_f4v w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; __builtin_nontemporal_store(w, reinterpret_cast<asx_f4v *>(p)); }
    else *reinterpret_cast<float4 *>(p) = v;
}
typedef float asx_f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_f2(float2 *p, float2 v, bool nt)
{
    if (nt) { asx_f2v w; w.x = v.x; w.y = v.y; __builtin_nontemporal_store(w, reinterpret_cast<asx_f2v *>(p)); }
    else *p = v;
}

// k_rows_r, which table look-ups are issued ahead of the loads they would otherwise queue behind (vmcnt completes in order):
// bit 0 = the block's tw_step / leg entries BEFORE the row loads (the barrier in front of the load phase's arithmetic then waits for an
// L2 round trip that overlaps the HBM loads instead of following them); bit 1 = the twiddles of the two-half form's store phase at
// the top of the kernel instead of behind its last barrier
// Measured (profiles/r5_experiments/19_*, alternating rounds): bit 1 rows 0.931 -> 0.918 ms (the store phase started with an L2 round
// trip on the two waves that run it); bit 0 nothing (0.930); both 0.921.  Bit 2 (the load steps' w_M2 values in front of the rows, whole
// steps without a condition): 0.946 -> 0.912 ms on top of bit 1, 0.939 -> 0.904 at N = 960 000.  Bit 3 (EVERY table look-up of the thread in
// front of its row loads): 480-point rows 0.771 -> 0.742 ms per 1024 pairs of N = 144 000, 0.928 -> 0.899 at 288 000; two-half form 0.917 -> 0.911.
// Default: bits 1, 2 and 3.
#ifndef ASX_ROWS_EARLY
#define ASX_ROWS_EARLY 14
#endif
// k_rows_rm, a block of a pair with a list: 1 = the conjugate four-step twiddle is applied by the copy wave, to the <= 64 values that
// leave the block, and the tile energies are those of the untwiddled values (MSK below); 0 = by the store phase, to all 2400 (the
// form partial storing came with: for same-box A/B builds).  Measured (profiles/qtw_late/, alternating traces, three runs each):
// launch B 875 -> 848 us on one box, 895 -> 853 on another.
#ifndef ASX_QTW_LATE
#define ASX_QTW_LATE 1
#endif
#ifndef ASX_ROWSR_WAVES
#define ASX_ROWSR_WAVES 4 // waves per SIMD the register allocation must allow: 8 blocks of 2 waves per CU
#endif

// ---------------------------------------------------------------------------
// k_rows_r: grid ((M1 + 1) * npairs).  One block = row k1 of both spectra of one pair.
//   S = Sched<n, R0, R1, R2>: three DIF stages.  Stage 0 spans the (sub-)row (block-wide, barrier after it); stages 1
//   and 2 stay inside the R0 sub-blocks of length n/R0 ("units"), and so do the first two stages of the inverse:
//   a wave that owns whole units runs  forward 1 -> forward 2 -> product -> inverse 2 -> inverse 1  on them with no
//   block barrier in between.  Inverse stage 0 spans the (sub-)row again.
//   TWO = false: M2 = n, NT threads; the outputs of inverse stage 0 leave from registers.
//   TWO = true:  M2 = 2n, 2*NT threads.  The first radix-2 DIF stage of the 2n-point row transforms runs in the
//                registers of the load phase -- a[j] = c[j] + c[j+n], b[j] = (c[j] - c[j+n]) w_M2^j -- after which the
//                even bins (from a) and the odd bins (from b) are two independent n-point problems: threads
//                [0, NT) take a, threads [NT, 2NT) take b, each half in its own LDS region; they meet again in the
//                store phase, Q[j] = A[j] + conj(w_M2^j) B[j], Q[j+n] = A[j] - conj(w_M2^j) B[j].  This is how the two
//                longest reference lengths get 600- and 400-row column tiles of sixteen real columns (64-byte input
//                pieces, whole 128-byte lines of C and Q) instead of 1200 / 800 rows of eight.
//   BC: broadcast forms (asx_xcorr_strided_f32_dev).  Bit 0 = C_x is the plan's broadcast slot, one C for every pair (pair step
//   0, temporal loads: every pair reads it, it must stay in the caches), bit 1 = C_y is.  BC = 0: both have Q's pair step.
//   Bit 2 (k_rows_rl, pool calls; with PHAT k_rows_rlp, with PHAT and BAND k_rows_rlb): C_x / C_y are rows sx / sy of the plan's bank
//   (L[pair], AsxPoolPair), temporal like the slot.
//   ENG (k_rows_re, the pruned inverse pass): the block also leaves the energy of its row of Q per column tile of sixteen,
//   eng[pair][k1][tile] = sum of |Q[k1][j2]|^2 over the tile's columns, in float32, one contiguous run per block.  The store phase
//   holds every Q value in a register: its |Q|^2 goes to LDS, into the upper halves of the slots, which are free by then (the
//   single-member values of the inverse stages live in the first 8 bytes of a slot) -- column c at the third float of slot c itself,
//   so a thread's stores share one address and differ in the instruction's offset field: a value costs its two multiplications and
//   the store, no index arithmetic (round 7's layout, 17 * tile + column, took eight integer instructions per value; dropping them
//   took back about a fifth of what the energies cost the row pass, which is now the fifth barrier and the phase behind it,
//   EXPERIMENTS.md round 8) -- and behind a barrier ALL threads of the block read column tid + NTB i: sixteen consecutive lanes
//   hold a tile and add it in four DPP steps inside their row, the balanced tree ((0+1)+(2+3))+... that tree_sum<16> is; one lane
//   of the sixteen stores.  No atomics: the same Q gives the same bits.  Nothing is loaded for it.  (Lanes are four dwords apart:
//   a four-way bank conflict on these stores and loads, a few hundred LDS cycles per block.)
//   MSK (k_rows_rm, partial storing of Q; with ENG, the two-half form only): the launch holds some of a pair's rows (AsxRowRun), and a
//   pair may come with a list of up to four column tiles (asx_internal.h: ASX_Q_ALL), the only ones the pruned pass will read.  A block
//   of such a pair keeps its values in LDS -- {re, im} in front of the energy in slot c, written by the thread that alone has just
//   read that slot -- and behind the fifth barrier one wave copies the listed tiles to Q, sixteen lanes a tile.  Without a list the
//   store phase is ENG's.  What such a block keeps in LDS is the output of the last radix-2 combine, S = A +- conj(w_M2^i) B, WITHOUT
//   the conjugate four-step twiddle (ASX_QTW_LATE): of the row's 2400 values at most 64 leave the block, the others are only squared
//   for the tile energies, and the factor has modulus 1 -- |S|^2 stands for |Q|^2 (asx_internal.h, ASX_PRUNE_DELTA, says what that
//   costs the bound).  The store phase of a listed block therefore needs neither w_F^(k1 j) nor leg[]: its threads skip those
//   look-ups, and a lane of the copy wave, which holds column c = i + NS * upper, i = j + Q0 t, asks for w_F^(k1 j) of ITS column
//   instead -- behind the row loads, because which of the two a thread asks for hangs on list[pair], and a wait for that word must
//   not stand in front of the rows; the values are not needed before the block's end.  The lane then forms Q with the functions
//   of the register path on the same operand values, cmul(lo, hi), times wh for the upper half, times leg[t] for t > 0, mulwc: the
//   stored bits are k_rows_re's.
//   PHAT (k_rows_rp, asx_xcorr_phat_f32_dev): the phase transform.  Every bin of the product X conj(Y) is divided by its magnitude in
//   the registers where it is formed, between the product and the first inverse butterfly (phat_unit below), so that the inverse
//   passes deliver r_phat, whose every frequency has one vote.  Nothing of the float32 error bound holds for a whitened spectrum:
//   row 0's block leaves the smallest positive normal float as the pair's bound (zero for a silent track, as ever), with which the
//   unchanged k_inv_cols_r instances keep the float32 maximum and list exact float32 ties only.
//   BAND (k_rows_rb, asx_xcorr_phat_band_f32_dev; with PHAT): only a range of frequencies votes.  Behind phat_unit every bin of the
//   thread is kept when min(k, F - k) lies in [lo, lo + span] and set to zero otherwise.  Where a bin is at that point: forward
//   stage 0 is decimation in frequency, so unit u holds the bins k2 = u (mod R0); stage 1 leaves residue jl (mod R1) in the R2 slots
//   from jl * R2; stage 2's output T is the last digit: k2 = u + R0 (jl + R1 T) inside a (sub-)row (tests/model_fourstep.py:
//   position_table).  The two-half form's half 0 holds the even bins and half 1 the odd ones, k2 -> 2 k2 + half; and row k1 holds
//   k = k1 + 2 M1 k2.  From T to T + 1 the bin moves by a step that is the same for every thread: one multiply for the first bin,
//   then an addition, two subtractions, two unsigned compares and two selects per bin.  Rows hold bins above N too (rows 0 and
//   M1 hold a bin and its mirror; the mirrors of the other rows' bins are in NO row, the inverse column pass makes them up), hence
//   the test on both k and F - k.  The band arrives by value as a kernel argument: nothing is looked up, no load is added or moved.
// ---------------------------------------------------------------------------
// q / |q| for every finite non-zero float32 q, whatever its exponent: the exponent of max(|re|, |im|) is taken out first, so the
// larger component lies in [1/2, 1) and the sum of squares in [1/4, 2) -- re * re + im * im of the bin itself overflows from 2^64
// on and is flushed below 2^-63, inputs the plain path handles.  v_rsq_f32 is good to one ulp; one Newton step brings |q'| to
// within two roundings of 1.  q = 0 exactly gives 0 (a bin nobody has a phase for casts no vote); a NaN component makes both NaN.
__device__ __forceinline__ Cx1 phat_unit(Cx1 q)
{
    const float m = fmaxf(fabsf(q.re), fabsf(q.im));
    const int e = __builtin_amdgcn_frexp_expf(m);
    const float a = ldexpf(q.re, -e), b = ldexpf(q.im, -e);
    const float n2 = fmaf(a, a, b * b);
    float y = __builtin_amdgcn_rsqf(n2);
    y = fmaf(y, fmaf(-0.5f * n2 * y, y, 0.5f), y); // y + y (1/2 - n2 y^2 / 2)
    return m == 0.f ? Cx1{ 0.f, 0.f } : Cx1{ a * y, b * y };
}

// The body takes P and W by value: that call boundary loads their fields at the top of the kernel.  Written inside the __global__
// itself the instruction stream changes, and with it the float32 rounding of r (11 of the headline's 124 coefficients moved by
// about 1e-7).
template <class S, int NT, bool TWO, int BC, bool ENG = false, bool PHAT = false, bool BAND = false, bool MSK = false>
__device__ __forceinline__ void rows_r_body(const RArgs P, const float2 *__restrict__ cx, const float2 *__restrict__ cy,
                                            float2 *__restrict__ qo, int nrows, size_t pitch_x, size_t pitch_y, size_t pitch_q,
                                            AsxPeakWs W, const AsxPoolPair *__restrict__ L = nullptr, float *__restrict__ eng = nullptr,
                                            const AsxBand band = {}, const AsxRowRun run = {},
                                            const unsigned long long *__restrict__ list = nullptr)
{
    static_assert(!MSK || (ENG && TWO), "partial storing: the two-half form, with the tile energies");
    static_assert(S::nstages == 3, "three-stage row schedules only");
    static_assert(!BAND || PHAT, "a band is a band of the phase transform");
    constexpr int NS = S::n;                 // length of a (sub-)row transform
    constexpr int M2 = TWO ? 2 * NS : NS;    // row length
    constexpr int TWS = TWO ? 2 : 1;         // w_NS^q = tw2[TWS * q] (tw2 is the table of M2)
    constexpr int NTB = TWO ? 2 * NT : NT;   // block size
    constexpr StageK K0 = S::stage(0), K1 = S::stage(1), K2 = S::stage(2);
    constexpr int R0 = K0.R, R1 = K1.R, R2 = K2.R;
    constexpr int Q0 = K0.q;  // butterflies of stage 0 = length of a unit
    constexpr int UN = K1.ns; // = Q0
    static_assert(UN == R1 * R2 && Q0 == UN && K2.q == 1, "unit = R1 x R2");
    static_assert((NS & 1) == 0, "rows move as 16 bytes per lane");
    constexpr int HALF = NS / 2, WSTEPS = (HALF + NTB - 1) / NTB;
    constexpr int LPU = R1 > R2 ? R1 : R2, UPW = 64 / LPU, NW = NT / 64;
    static_assert(NT % 64 == 0 && UPW >= 1, "whole waves");
    constexpr bool XNT = (BC & 1) == 0, YNT = (BC & 2) == 0;

#ifdef ASX_STAMPS
    const long long t_entry = clock64(), w_entry = wall_clock64();
#endif
    const int task = blockIdx.x, tid = threadIdx.x;
    const int half = TWO ? tid / NT : 0, lt = tid - half * NT; // which sub-row, thread index inside its half
    float4 *A4 = reinterpret_cast<float4 *>(asx_lds_r) + half * NS;
    __shared__ float2 tw_step[WSTEPS]; // (1/2) w_F^(k1 * 2*NTB*i): the four-step twiddle from load step to load step
    __shared__ float2 leg[R0];         // w_F^(k1 * Q0*t): ... and from leg to leg of the last inverse stage

    // MSK: the launch holds run.count rows of every pair, k1 = r, or r + run.hop from r = run.row_a on (AsxRowRun)
    const int pair = MSK ? task / run.count : task / nrows;
    uint32_t k1 = (uint32_t)(task - pair * (MSK ? run.count : nrows));
    if constexpr (MSK) k1 += (int)k1 >= run.row_a ? (uint32_t)run.hop : 0u;
    // ... and the pair's stored tiles (ASX_Q_ALL, or no list at all: the whole row), asked for with the other early look-ups; block-uniform
    unsigned long long wl = ASX_Q_ALL;
    if constexpr (MSK) { if (list) wl = list[pair]; }
    [[maybe_unused]] const bool part = MSK && wl != ASX_Q_ALL;
    constexpr bool LATE = MSK && ASX_QTW_LATE != 0; // a listed block twiddles only what it stores (see MSK above)
    static_assert(!LATE || (ASX_ROWS_EARLY & 2) != 0, "ASX_QTW_LATE: the store phase's look-ups are the early ones");
    // the column of a listed tile that lane tid of the copy wave (tid < 64) holds; -1: an unused entry of the list names no tile
    [[maybe_unused]] auto copy_col = [&]() __attribute__((always_inline)) {
        const unsigned t = (unsigned)(wl >> (16 * (tid >> 4))) & 0xFFFFu;
        return t < (unsigned)(M2 / ASX_PRUNE_T) ? (int)t * ASX_PRUNE_T + (tid & 15) : -1;
    };
    const size_t row = (size_t)RWS_PAIR(pair) * pitch_q + (size_t)k1 * M2;
    size_t rowx, rowy;
    if constexpr ((BC & 4) != 0) {
        rowx = (size_t)L[pair].sx * pitch_x + (size_t)k1 * M2;
        rowy = (size_t)L[pair].sy * pitch_y + (size_t)k1 * M2;
    } else {
        rowx = (size_t)RWS_PAIR(pair) * pitch_x + (size_t)k1 * M2;
        rowy = (size_t)RWS_PAIR(pair) * pitch_y + (size_t)k1 * M2;
    }
    if (k1 == 0 && tid < 64) {
        // Row 0 of a pair also prepares the pair's peak search (k_inv_cols_r runs after this kernel): the float32
        // error bound from the norms k_fwd_cols_r left, the running maximum and the candidate count back to zero.
        const float *np = W.nrm_part + (size_t)pair * 2 * P.ntiles;
        float sx = 0.f, sy = 0.f;
        for (int t = tid; t < P.ntiles; t += 64) { sx += np[t]; sy += np[P.ntiles + t]; }
        sx = wave_sum_f32(sx); sy = wave_sum_f32(sy);
        if (tid == 0) {
            if constexpr (PHAT) W.bound2[pair] = (sx != 0.f && sy != 0.f) ? 1.17549435e-38f : 0.f; // FLT_MIN: exact ties only
            else W.bound2[pair] = P.bound_scale * sqrtf(sx) * sqrtf(sy);
            W.pairmax[pair] = 0;
            W.cand_n[pair] = 0;
        }
    }
    // bit 3 of ASX_ROWS_EARLY (see the row loads below): -3 ... -4 % for 480-point rows, -0.7 % for the two-half form, +0.6 % for 1200-point
    // rows in one piece, which keep the old order (profiles/r5_experiments/19_*)
    constexpr bool LOOKUPS_FIRST = (ASX_ROWS_EARLY & 8) != 0 && (TWO || NS != 1200);
    const bool is_step = tid < WSTEPS, is_leg = tid >= NTB - R0;
    static_assert(WSTEPS <= NTB - R0, "the threads that fill tw_step and leg are different threads");
    float2 pre_lo = make_float2(1.f, 0.f), pre_hi = pre_lo;
    if ((LOOKUPS_FIRST || (ASX_ROWS_EARLY & 1)) && (is_step || is_leg)) {
        const uint32_t p = is_step ? k1 * (uint32_t)(2 * NTB * tid) : k1 * (uint32_t)(Q0 * (tid - (NTB - R0)));
        pre_lo = P.tw_lo[p & (ASX_TW_LO - 1u)];
        pre_hi = P.tw_hi[p >> ASX_TW_LOG];
    }
    // the look-ups of the two-half form's store phase (threads [0, Q0): butterfly j = tid)
    float2 tail_w2 = make_float2(1.f, 0.f), tail_lo = tail_w2, tail_hi = tail_w2;
    if (TWO && (ASX_ROWS_EARLY & 2) && tid < Q0) {
        [[maybe_unused]] const uint32_t p = k1 * (uint32_t)tid;
        tail_w2 = P.tw2[tid];
        if constexpr (!LATE) { // (LATE: behind the row loads, see there)
            tail_lo = P.tw_lo[p & (ASX_TW_LO - 1u)];
            tail_hi = P.tw_hi[p >> ASX_TW_LOG];
        }
    }
    // (bit 2 of ASX_ROWS_EARLY: the two-half form's w_M2^(2q), w_M2^(2q+1) of every load step asked for HERE, in front of the rows, instead
    // of inside the step behind the barrier -- a table load and the wait for it between the arrival of the rows and their first use)
    float4 w2pre[TWO ? WSTEPS : 1];
    if constexpr (TWO && (ASX_ROWS_EARLY & 4) != 0) {
        static_for<0, WSTEPS>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            const int q = tid + i * NTB;
            w2pre[I] = make_float4(1.f, 0.f, 1.f, 0.f);
            if ((i + 1) * NTB <= HALF || q < HALF) w2pre[I] = *reinterpret_cast<const float4 *>(P.tw2 + 2 * q);
        });
    }
    // The row loads.  Bit 3 of ASX_ROWS_EARLY: issued BEHIND every table look-up of the thread (they used to come first, "the look-ups
    // overlap them" -- but vmcnt completes in order: a look-up issued behind the rows is not usable before the rows have arrived, and the
    // tw_step / leg threads then started an L2 round trip of their own in front of the block's barrier)
    float4 lx[WSTEPS], ly[WSTEPS], lx2[TWO ? WSTEPS : 1], ly2[TWO ? WSTEPS : 1];
    auto issue_row_loads = [&]() __attribute__((always_inline)) {
        const float2 *gx = cx + rowx, *gy = cy + rowy;
        static_for<0, WSTEPS>([&](auto I) __attribute__((always_inline)) {
            const int q = tid + decltype(I)::value * NTB;
            if (((ASX_ROWS_EARLY & 4) && (decltype(I)::value + 1) * NTB <= HALF) || q < HALF) { // (a whole step inside the row: no condition)
                lx[I] = ld_f4(gx + 2 * q, XNT && (ASX_RNT & 4));
                ly[I] = ld_f4(gy + 2 * q, YNT && (ASX_RNT & 4));
                if constexpr (TWO) {
                    lx2[I] = ld_f4(gx + NS + 2 * q, XNT && (ASX_RNT & 4));
                    ly2[I] = ld_f4(gy + NS + 2 * q, YNT && (ASX_RNT & 4));
                }
            }
        });
    };
    if constexpr (!LOOKUPS_FIRST) issue_row_loads();
    auto publish_step_and_leg = [&]() __attribute__((always_inline)) {
        if (is_step) {
            // ... times 1/2: k_fwd_cols_r stores 2 C (its untangling without the halving)
            const float2 t = (LOOKUPS_FIRST || (ASX_ROWS_EARLY & 1)) ? cmul(pre_lo, pre_hi) : tw_F(P, k1 * (uint32_t)(2 * NTB * tid));
            tw_step[tid] = make_float2(0.5f * t.x, 0.5f * t.y);
        }
        if (is_leg) { const int t = tid - (NTB - R0); leg[t] = (LOOKUPS_FIRST || (ASX_ROWS_EARLY & 1)) ? cmul(pre_lo, pre_hi) : tw_F(P, k1 * (uint32_t)(Q0 * t)); }
    };
    if constexpr (!LOOKUPS_FIRST) publish_step_and_leg();
    const float2 twa = tw_F(P, k1 * (uint32_t)(2 * tid < NS ? 2 * tid : 0)); // w_F^(k1 * 2 tid)
    const float2 wk1 = tw_F(P, k1);
    const float2 wh = TWO ? tw_F(P, k1 * (uint32_t)NS) : make_float2(1.f, 0.f); // w_F^(k1 n): from c[j] to c[j + n]
    // stage twiddle seeds (they depend on the thread only): stage 0 / inverse stage 0, and the wave-local stage 1
    const int j0 = lt < Q0 ? lt : 0;
    const float2 s0w1 = P.tw2[TWS * j0], s0w4 = P.tw2[TWS * 4 * j0];
    const float2 tw0base = TWO ? make_float2(1.f, 0.f) : tw_F(P, k1 * (uint32_t)j0); // four-step factor of the outputs of inverse stage 0 (!TWO)
    const int lane = tid & 63, wave = lt >> 6;
    const int ul = lane / LPU, jl = lane - ul * LPU;
    const int j1c = jl < R2 ? jl : 0;
    const float2 s1w1 = P.tw2[TWS * K1.twmul * j1c], s1w4 = P.tw2[TWS * (R1 > 4 ? 4 : 1) * K1.twmul * j1c];
    if constexpr (LOOKUPS_FIRST) issue_row_loads();
    if constexpr (LATE) {
        // w_F^(k1 j): of the thread's own butterfly j = tid, or in a listed block of the column the lane will copy.  list[pair] decides,
        // so these two look-ups stand behind the row loads; they are used behind the block's last barrier.
        int jq = tid < Q0 ? tid : -1;
        if (part) {
            const int c = tid < 64 ? copy_col() : -1;
            jq = c < 0 ? -1 : (c % NS) % Q0;
        }
        if (jq >= 0) {
            const uint32_t p = k1 * (uint32_t)jq;
            tail_lo = P.tw_lo[p & (ASX_TW_LO - 1u)];
            tail_hi = P.tw_hi[p >> ASX_TW_LOG];
        }
    }
    if constexpr (LOOKUPS_FIRST) publish_step_and_leg();
    RSTAMP(0, task, 0);
#ifdef ASX_STAMPS
    if (P.stamps && P.stamp_kernel == 0 && threadIdx.x == 0) { P.stamps[(size_t)task * 8 + 6] = t_entry; P.stamps[(size_t)task * 8 + 7] = w_entry; }
#endif
    __syncthreads(); // tw_step, leg
    static_for<0, WSTEPS>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value;
        const int q = tid + i * NTB;
        if (((ASX_ROWS_EARLY & 4) && (i + 1) * NTB <= HALF) || q < HALF) {
            const float2 wa0 = cmul(twa, tw_step[i]), wa1 = cmul(wa0, wk1);
            const Cx2 c0 = mulw(Cx2{ v2f{ lx[I].x, ly[I].x }, v2f{ lx[I].y, ly[I].y } }, wa0);
            const Cx2 c1 = mulw(Cx2{ v2f{ lx[I].z, ly[I].z }, v2f{ lx[I].w, ly[I].w } }, wa1);
            if constexpr (!TWO) {
                lds_put(A4 + 2 * q, c0);
                lds_put(A4 + 2 * q + 1, c1);
            } else {
                float4 *base = reinterpret_cast<float4 *>(asx_lds_r);
                const float2 wb0 = cmul(wa0, wh), wb1 = cmul(wa1, wh);
                const Cx2 d0 = mulw(Cx2{ v2f{ lx2[I].x, ly2[I].x }, v2f{ lx2[I].y, ly2[I].y } }, wb0);
                const Cx2 d1 = mulw(Cx2{ v2f{ lx2[I].z, ly2[I].z }, v2f{ lx2[I].w, ly2[I].w } }, wb1);
                const float4 w2 = (ASX_ROWS_EARLY & 4) ? w2pre[I] : *reinterpret_cast<const float4 *>(P.tw2 + 2 * q); // w_M2^(2q), w_M2^(2q+1)
                lds_put(base + 2 * q, c0 + d0);
                lds_put(base + 2 * q + 1, c1 + d1);
                lds_put(base + NS + 2 * q, mulw(c0 - d0, make_float2(w2.x, w2.y)));
                lds_put(base + NS + 2 * q + 1, mulw(c1 - d1, make_float2(w2.z, w2.w)));
            }
        }
    });
    __syncthreads();
    RSTAMP(0, task, 1);

    // ---- forward stage 0: butterflies j < Q0, legs Q0 apart ------------------------------------------------
    for (int j = lt; j < Q0; j += NT) {
        float4 *p = A4 + j;
        Cx2 v[R0];
        static_for<0, R0>([&](auto T) __attribute__((always_inline)) { v[T] = lds_get(p + decltype(T)::value * Q0); });
        float2 w1 = s0w1, w4 = s0w4;
        if (j != lt) { w1 = P.tw2[TWS * j]; w4 = P.tw2[TWS * 4 * j]; }
        float2 tww[R0];
        stage_twiddles_from<R0>(w1, w4, tww);
        Bfly<R0, false>::run(v);
        static_for<1, R0>([&](auto U) __attribute__((always_inline)) { v[U] = mulw(v[U], tww[U]); });
        static_for<0, R0>([&](auto T) __attribute__((always_inline)) { lds_put(p + decltype(T)::value * Q0, v[T]); });
    }
    __syncthreads();
    RSTAMP(0, task, 2);

    // ---- wave-local: forward 1, forward 2 + X conj(Y) + inverse 2, inverse 1 -------------------------------
    for (int u0 = wave * UPW; u0 < R0; u0 += NW * UPW) { // wave-uniform trip count
        const int unit = u0 + ul;
        const bool on = (ul < UPW) && (unit < R0);
        float4 *base = A4 + (on ? unit : 0) * UN;
        float2 tw1[R1];
        stage_twiddles_from<R1>(s1w1, s1w4, tw1);
        if (on && jl < R2) { // stage 1: butterfly jl of the unit, legs R2 apart, outputs times w_UN^(jl u)
            float4 *p = base + jl;
            Cx2 v[R1];
            static_for<0, R1>([&](auto T) __attribute__((always_inline)) { v[T] = lds_get(p + decltype(T)::value * R2); });
            Bfly<R1, false>::run(v);
            static_for<1, R1>([&](auto U) __attribute__((always_inline)) { v[U] = mulw(v[U], tw1[U]); });
            static_for<0, R1>([&](auto T) __attribute__((always_inline)) { lds_put(p + decltype(T)::value * R2, v[T]); });
        }
        wave_lds_sync();
        if (on && jl < R1) { // stage 2: R2 consecutive slots; the bins of X and Y meet in registers
            float4 *p = base + jl * R2;
            Cx2 v[R2];
            static_for<0, R2>([&](auto T) __attribute__((always_inline)) { v[T] = lds_get(p + decltype(T)::value); });
            Bfly<R2, false>::run(v);
            Cx1 pr[R2];
            static_for<0, R2>([&](auto T) __attribute__((always_inline)) {
                // src/cross_correlation.c:232-233: X * conj(Y); member x = source, member y = sample
                pr[T] = Cx1{ v[T].re.x * v[T].re.y + v[T].im.x * v[T].im.y, v[T].im.x * v[T].re.y - v[T].re.x * v[T].im.y };
            });
            if constexpr (PHAT) static_for<0, R2>([&](auto T) __attribute__((always_inline)) { pr[T] = phat_unit(pr[T]); });
            if constexpr (BAND) {
                // pr[T] is bin k2 = unit + R0 (jl + R1 T) of the (sub-)row, i.e. k = k1 + 2 M1 k2 (two-half form: 2 k2 + half for k2)
                constexpr uint32_t HS = TWO ? 2u : 1u;
                const uint32_t F = 2u * P.N, m2 = 2u * (uint32_t)P.M1;
                const uint32_t k0 = k1 + m2 * (HS * (uint32_t)(unit + R0 * jl) + (uint32_t)half), kstep = m2 * (HS * R0 * R1);
                static_for<0, R2>([&](auto T) __attribute__((always_inline)) {
                    const uint32_t k = k0 + (uint32_t) decltype(T)::value * kstep;
                    const bool in = (k - band.lo <= band.span) || (F - k - band.lo <= band.span); // min(k, F - k) in [lo, lo + span]
                    pr[T] = in ? pr[T] : Cx1{ 0.f, 0.f };
                });
            }
            Bfly<R2, true>::run(pr);
            static_for<0, R2>([&](auto T) __attribute__((always_inline)) { lds_put1(p + decltype(T)::value, pr[T]); });
        }
        wave_lds_sync();
        if (on && jl < R2) { // inverse stage 1
            float4 *p = base + jl;
            Cx1 v[R1];
            static_for<0, R1>([&](auto T) __attribute__((always_inline)) { v[T] = lds_get1(p + decltype(T)::value * R2); });
            static_for<1, R1>([&](auto U) __attribute__((always_inline)) { v[U] = mulwc(v[U], tw1[U]); });
            Bfly<R1, true>::run(v);
            static_for<0, R1>([&](auto T) __attribute__((always_inline)) { lds_put1(p + decltype(T)::value * R2, v[T]); });
        }
    }
    __syncthreads();
    RSTAMP(0, task, 3);

    // ---- inverse stage 0 from LDS, the outputs leave from registers -------------------------------------------------
    float2 *go = qo + row;
    // ENG: |Q|^2 of column c into the third float of LDS slot c (see above).  eng_put(ej, c0, y) is column j + c0, c0 a compile-time
    // constant at every call: one address per thread, the rest is the instruction's offset field (16 * (M2 - 1) + 8 < 2^16)
    static_assert(!ENG || (ASX_PRUNE_T == 16 && M2 % ASX_PRUNE_T == 0 && NTB % ASX_PRUNE_T == 0 && 16 * M2 < 65536),
                  "tile energies: tiles of sixteen columns, a tile per row of sixteen lanes");
    auto eng_base = [](int j) __attribute__((always_inline)) { return reinterpret_cast<float *>(asx_lds_r) + 4 * j + 2; };
    auto eng_put = [](float *ej, int c0, Cx1 y) __attribute__((always_inline)) { ej[4 * c0] = fmaf(y.re, y.re, y.im * y.im); };
    if constexpr (!TWO) {
        for (int j = lt; j < Q0; j += NT) {
            [[maybe_unused]] float *const ej = eng_base(j);
            const float4 *p = A4 + j;
            Cx1 v[R0];
            static_for<0, R0>([&](auto T) __attribute__((always_inline)) { v[T] = lds_get1(p + decltype(T)::value * Q0); });
            float2 w1 = s0w1, w4 = s0w4, fb = tw0base;
            if (j != lt) { w1 = P.tw2[j]; w4 = P.tw2[4 * j]; fb = tw_F(P, k1 * (uint32_t)j); }
            float2 tww[R0];
            stage_twiddles_from<R0>(w1, w4, tww);
            static_for<1, R0>([&](auto U) __attribute__((always_inline)) { v[U] = mulwc(v[U], tww[U]); });
            Bfly<R0, true>::run(v);
            // conjugate four-step twiddle, straight to HBM
            static_for<0, R0>([&](auto T) __attribute__((always_inline)) {
                constexpr int t = decltype(T)::value;
                const Cx1 y = mulwc(v[t], t == 0 ? fb : cmul(fb, leg[t]));
                st_f2(go + j + t * Q0, make_float2(y.re, y.im), ASX_RNT & 8);
                if constexpr (ENG) eng_put(ej, t * Q0, y);
            });
        }
    } else {
        // Both halves at once, as ONE pair of sequences (A, B) per thread: the butterfly j of inverse stage 0 of the
        // even-bin and of the odd-bin problem share their twiddles, and their outputs A[j + Q0 t], B[j + Q0 t] are exactly
        // what the last radix-2 stage combines:  Q[i] = A[i] + conj(w_M2^i) B[i],  Q[i + n] = A[i] - conj(w_M2^i) B[i]
        // (w_M2^(j + Q0 t) = w_M2^j times the compile-time root w_{2 R0}^t), then the conjugate four-step twiddles.
        // Only Q0 threads work here; the others are done.
        const float4 *base = reinterpret_cast<const float4 *>(asx_lds_r);
        static_assert(Q0 <= NT, "one butterfly per thread of the first half");
        for (int j = tid; j < Q0; j += NTB) {
            [[maybe_unused]] float *const ej = eng_base(j);
            Cx2 v[R0];
            static_for<0, R0>([&](auto T) __attribute__((always_inline)) {
                const Cx1 a = lds_get1(base + j + decltype(T)::value * Q0), b = lds_get1(base + NS + j + decltype(T)::value * Q0);
                v[T] = Cx2{ v2f{ a.re, b.re }, v2f{ a.im, b.im } };
            });
            float2 tww[R0];
            if constexpr (ASX_ROWS_EARLY & 2) stage_twiddles_from<R0>(s0w1, s0w4, tww); // j = tid = lt here: the seeds of forward stage 0
            else stage_twiddles_from<R0>(P.tw2[TWS * j], P.tw2[TWS * 4 * j], tww);
            static_for<1, R0>([&](auto U) __attribute__((always_inline)) { v[U] = mulwc(v[U], tww[U]); });
            Bfly<R0, true>::run(v);
            const float2 w2 = (ASX_ROWS_EARLY & 2) ? tail_w2 : P.tw2[j];                                  // w_M2^j
            const float2 fa = (ASX_ROWS_EARLY & 2) ? cmul(tail_lo, tail_hi) : tw_F(P, k1 * (uint32_t)j);  // w_F^(k1 j)
            const float2 fbh = cmul(fa, wh);                  // w_F^(k1 (j + n))
            // PART (MSK, a pair with a list): Q stays in LDS, {re, im} in front of the energy in slot c -- the slots j + Q0 t and
            // NS + j + Q0 t are exactly the ones this thread alone has just read, so no barrier is needed -- and the listed tiles leave
            // behind the fifth barrier (below).  Otherwise Q leaves from registers, as ever.  LATE: what stays is A +- Bw, the
            // twiddle is the copy wave's; fa and fbh are then not this butterfly's and not used.
            auto leave = [&](auto PART) __attribute__((always_inline)) {
                static_for<0, R0>([&](auto T) __attribute__((always_inline)) {
                    constexpr int t = decltype(T)::value;
                    const Cx1 A = Cx1{ v[t].re.x, v[t].im.x };
                    const Cx1 Bw = mul_root<2 * R0, t, true>(mulwc(Cx1{ v[t].re.y, v[t].im.y }, w2)); // conj(w_M2^(j + Q0 t)) B
                    if constexpr (decltype(PART)::value && LATE) {
                        const Cx1 sp = A + Bw, sm = A - Bw;
                        ej[4 * (t * Q0) - 2] = sp.re; ej[4 * (t * Q0) - 1] = sp.im;
                        ej[4 * (NS + t * Q0) - 2] = sm.re; ej[4 * (NS + t * Q0) - 1] = sm.im;
                        eng_put(ej, t * Q0, sp); eng_put(ej, NS + t * Q0, sm);
                        return;
                    }
                    const float2 lg = leg[t];
                    const Cx1 y = mulwc(A + Bw, t == 0 ? fa : cmul(fa, lg));
                    const Cx1 z = mulwc(A - Bw, t == 0 ? fbh : cmul(fbh, lg));
                    if constexpr (decltype(PART)::value) {
                        ej[4 * (t * Q0) - 2] = y.re; ej[4 * (t * Q0) - 1] = y.im;
                        ej[4 * (NS + t * Q0) - 2] = z.re; ej[4 * (NS + t * Q0) - 1] = z.im;
                    } else {
                        st_f2(go + j + t * Q0, make_float2(y.re, y.im), ASX_RNT & 8);
                        st_f2(go + NS + j + t * Q0, make_float2(z.re, z.im), ASX_RNT & 8);
                    }
                    if constexpr (ENG) { eng_put(ej, t * Q0, y); eng_put(ej, NS + t * Q0, z); }
                });
            };
            if constexpr (MSK) {
                if (part) leave(std::true_type{});
                else leave(std::false_type{});
            } else {
                leave(std::false_type{});
            }
        }
    }
    if constexpr (ENG) {
        // every thread of the block: column tid + NTB i of step i, sixteen consecutive lanes = one tile, added inside their DPP row
        __syncthreads();
        constexpr int NTILE = M2 / ASX_PRUNE_T, ESTEPS = (M2 + NTB - 1) / NTB;
        const float *er = eng_base(tid);
        float *eo = eng + ((size_t)pair * nrows + k1) * NTILE + (tid >> 4);
        float v[ESTEPS];
        static_for<0, ESTEPS>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            v[I] = ((i + 1) * NTB <= M2 || tid + i * NTB < M2) ? er[4 * NTB * i] : 0.f; // (whole rows of sixteen lanes are in or out)
        });
        static_for<0, ESTEPS>([&](auto I) __attribute__((always_inline)) { v[I] = row16_sum(v[I]); });
        if ((tid & 15) == 0)
            static_for<0, ESTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                if ((i + 1) * NTB <= M2 || tid + i * NTB < M2) eo[(NTB / 16) * i] = v[I];
            });
        if constexpr (MSK) {
            // the listed tiles from LDS to Q: one wave, sixteen lanes a tile, 8 bytes per lane, 128 bytes per tile row (an unused
            // entry of the list names no tile)
            if (part && tid < 64) {
                const int c = copy_col();
                if (c >= 0) {
                    const float *sl = reinterpret_cast<const float *>(asx_lds_r) + 4 * c;
                    if constexpr (LATE) {
                        // the register path's expressions for column c = j + Q0 t (+ NS): y = mulwc(A + Bw, t == 0 ? fa : cmul(fa, leg[t])),
                        // z the same with fbh = cmul(fa, wh) for fa
                        const int i = c >= NS ? c - NS : c, t = i / Q0;
                        const float2 fa = cmul(tail_lo, tail_hi); // w_F^(k1 j), j = i mod Q0: asked for at the top
                        const float2 f = c >= NS ? cmul(fa, wh) : fa;
                        const Cx1 y = mulwc(Cx1{ sl[0], sl[1] }, t == 0 ? f : cmul(f, leg[t]));
                        st_f2(go + c, make_float2(y.re, y.im), ASX_RNT & 8);
                    } else {
                        st_f2(go + c, make_float2(sl[0], sl[1]), ASX_RNT & 8);
                    }
                }
            }
        }
    }
    RSTAMP(0, task, 4);
#ifdef ASX_STAMPS
    if (P.stamps && P.stamp_kernel == 0 && threadIdx.x == 0) P.stamps[(size_t)task * 8 + 5] = wall_clock64();
#endif
}

template <class S, int NT, bool TWO, int BC>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_r(const RArgs P, const float2 *__restrict__ cx,
                                                                                const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                int nrows, size_t pair_pitch, AsxPeakWs W)
{
    rows_r_body<S, NT, TWO, BC>(P, cx, cy, qo, nrows, (BC & 1) ? 0 : pair_pitch, (BC & 2) ? 0 : pair_pitch, pair_pitch, W);
}

// The row pass of the pruned inverse pass (asx_launch_rows_r, a group whose AsxSpectra carries the lane's AsxPrune): k_rows_r<S, NT, TWO, 0> that also leaves the tile energies of Q (ENG
// above).  A kernel name of its own: the twelve k_rows_r instances stay the kernels they were.
template <class S, int NT, bool TWO>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_re(const RArgs P, const float2 *__restrict__ cx,
                                                                                 const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                 int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                 float *__restrict__ eng)
{
    rows_r_body<S, NT, TWO, 0, true>(P, cx, cy, qo, nrows, pair_pitch, pair_pitch, pair_pitch, W, nullptr, eng);
}

// The row pass with partial storing (asx_launch_rows_r, a pruned group whose AsxPrune carries a list): k_rows_re on the rows of `run`,
// which stores of a pair with a list only the listed column tiles of Q (MSK above) -- list null, or a pair's entry ASX_Q_ALL: every
// column, from registers, as k_rows_re does.  The energies are k_rows_re's either way.  Two-half form only.
template <class S, int NT, bool TWO>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rm(const RArgs P, const float2 *__restrict__ cx,
                                                                                 const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                 int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                 float *__restrict__ eng, const AsxRowRun run,
                                                                                 const unsigned long long *__restrict__ list)
{
    rows_r_body<S, NT, TWO, 0, true, false, false, true>(P, cx, cy, qo, nrows, pair_pitch, pair_pitch, pair_pitch, W, nullptr, eng, {}, run,
                                                          list);
}

// The row pass of a PHAT group (asx_launch_rows_r, weight ASX_W_PHAT): k_rows_r<S, NT, TWO, BC> with the whitened product
// (PHAT above).  A kernel name of its own, like k_rows_re: the twelve k_rows_r instances stay the kernels they were.
template <class S, int NT, bool TWO, int BC>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rp(const RArgs P, const float2 *__restrict__ cx,
                                                                                 const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                 int nrows, size_t pair_pitch, AsxPeakWs W)
{
    rows_r_body<S, NT, TWO, BC, false, true>(P, cx, cy, qo, nrows, (BC & 1) ? 0 : pair_pitch, (BC & 2) ? 0 : pair_pitch, pair_pitch, W);
}

// The row pass of a banded PHAT group (weight ASX_W_PHAT_BAND): k_rows_rp<S, NT, TWO, BC> that lets only the bins of
// `band` vote (BAND above).  Again a kernel name of its own: the k_rows_r and k_rows_rp instances stay the kernels they were.
template <class S, int NT, bool TWO, int BC>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rb(const RArgs P, const float2 *__restrict__ cx,
                                                                                 const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                 int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                 const AsxBand band)
{
    rows_r_body<S, NT, TWO, BC, false, true, true>(P, cx, cy, qo, nrows, (BC & 1) ? 0 : pair_pitch, (BC & 2) ? 0 : pair_pitch, pair_pitch, W,
                                                   nullptr, nullptr, band);
}

// What the listed row kernels do for a pair flagged ASX_POOL_INVALID (k_rows_rl below): the block's row of Q becomes NaN and row 0's
// block leaves a zero bound and an empty running maximum.  true (block-uniform): the block is done.
template <class S, int NT, bool TWO>
__device__ __forceinline__ bool rows_rl_invalid(float2 *__restrict__ qo, int nrows, size_t pair_pitch, const AsxPeakWs &W,
                                                const AsxPoolPair *__restrict__ L)
{
    const int pair = blockIdx.x / nrows;
    if (!(L[pair].flags & ASX_POOL_INVALID)) return false;
    constexpr int M2 = TWO ? 2 * S::n : S::n, NTB = TWO ? 2 * NT : NT;
    const int k1 = blockIdx.x - pair * nrows;
    float2 *go = qo + (size_t)pair * pair_pitch + (size_t)k1 * M2;
    for (int j = threadIdx.x; j < M2; j += NTB) go[j] = make_float2(NAN, NAN);
    if (k1 == 0 && threadIdx.x == 0) {
        W.bound2[pair] = 0.f;
        W.pairmax[pair] = 0;
        W.cand_n[pair] = 0;
    }
    return true;
}

// The listed form (asx_xcorr_pool_f32_dev): pair p's C_x / C_y are rows L[p].sx / L[p].sy of the bank (cx, cy: its source and sample
// spectra, pair_pitch apart), both loaded temporal -- consecutive pairs may share a slot.  The same body: the same float32 Q, bit for
// bit, as k_rows_r on the same C rows.  A pair flagged ASX_POOL_INVALID (an index outside its pool) gets a NaN Q and a zero bound instead: every
// inverse tile of every pass leaves at the zero bound before it scans anything (k_inv_cols_r), whatever the pair's window, zones
// or seed, so its running maximum stays empty and it is never counted, listed or re-evaluated -- and k_invalid_pairs (top-k:
// k_invalid_pairs_k) overwrites its results.
template <class S, int NT, bool TWO>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rl(const RArgs P, const float2 *__restrict__ cx,
                                                                                 const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                 int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                 const AsxPoolPair *__restrict__ L)
{
    if (rows_rl_invalid<S, NT, TWO>(qo, nrows, pair_pitch, W, L)) return;
    rows_r_body<S, NT, TWO, 7>(P, cx, cy, qo, nrows, pair_pitch, pair_pitch, pair_pitch, W, L);
}

// The listed form of a PHAT group (asx_xcorr_pool_phat_f32_dev over the full band): k_rows_rl with the whitened product, the float32
// Q' of k_rows_rp on the same C rows.  An invalid pair leaves what k_rows_rl leaves: k_phat_finalize then finds an empty maximum, and
// k_invalid_pairs overwrites the pair's results, its peak included.  Names of their own: the k_rows_rl instances stay the kernels they were.
template <class S, int NT, bool TWO>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rlp(const RArgs P, const float2 *__restrict__ cx,
                                                                                  const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                  int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                  const AsxPoolPair *__restrict__ L)
{
    if (rows_rl_invalid<S, NT, TWO>(qo, nrows, pair_pitch, W, L)) return;
    rows_r_body<S, NT, TWO, 7, false, true>(P, cx, cy, qo, nrows, pair_pitch, pair_pitch, pair_pitch, W, L);
}

// ... and of a banded PHAT group: k_rows_rlp that lets only the bins of `band` vote, the float32 Q' of k_rows_rb.
template <class S, int NT, bool TWO>
__global__ __launch_bounds__(TWO ? 2 * NT : NT, ASX_ROWSR_WAVES) void k_rows_rlb(const RArgs P, const float2 *__restrict__ cx,
                                                                                  const float2 *__restrict__ cy, float2 *__restrict__ qo,
                                                                                  int nrows, size_t pair_pitch, AsxPeakWs W,
                                                                                  const AsxPoolPair *__restrict__ L, const AsxBand band)
{
    if (rows_rl_invalid<S, NT, TWO>(qo, nrows, pair_pitch, W, L)) return;
    rows_r_body<S, NT, TWO, 7, false, true, true>(P, cx, cy, qo, nrows, pair_pitch, pair_pitch, pair_pitch, W, L, nullptr, band);
}

// ---------------------------------------------------------------------------
// Column tiles of the real-column kernels: T REAL columns j2 = c0 .. c0+T-1 of the [2 M1][M2] sample matrix, held
// in LDS as [M1][T/2] float4 slots: slot (m, g) = { x[2m][c0+2g], x[2m+1][c0+2g], x[2m][c0+2g+1], x[2m+1][c0+2g+1] },
// i.e. the complex sequences z[m] = x[2m] + i x[2m+1] of two adjacent columns side by side (the pair-planar form
// of lds_fft.h).  A tile row is 4T bytes of the input (32 / T tiles share a 128-byte line: blocks b, b+8, ... of
// one XCD, as in col_tile_of_block) and 8T bytes of C / Q.
// ---------------------------------------------------------------------------
__device__ __host__ constexpr int rcol_line_log(int logT) { return logT >= 5 ? 0 : 5 - logT; } // log2(tiles per input line)
__device__ __forceinline__ int rcol_tile_of_block(int b, int logT)
{
    const int ll = rcol_line_log(logT);
    const int grp = 8 << ll;
    return (b & ~(grp - 1)) + ((b & 7) << ll) + ((b >> 3) & ((1 << ll) - 1));
}
static inline unsigned rcol_grid_x(int ntiles, int logT)
{
    const unsigned grp = 8u << rcol_line_log(logT);
    return ((unsigned)ntiles + grp - 1) / grp * grp;
}

// The work items v = 0 of the column kernels' register stage (the butterflies that pair with themselves: H of (MB / 2) H items, a branch
// of their own) sit in the LAST H threads of the block when that leaves them a wave of their own (600- and 400-row tiles: 392 / 312
// regular items, 512 threads): with them in threads [0, H), wave 0 ran both branches one after the other -- in k_fwd_cols_r at the very
// end of the block's life, in k_inv_cols_r with a row load of its own behind the others.  Forward / inverse columns 0.989 -> 0.978 /
// 0.314 -> 0.310 ms at 600 rows, 2.766 -> 2.746 / 1.049 -> 1.019 at 400; 300-row tiles (256 threads, no idle wave): +1.5 % / 0, left alone
// (profiles/r5_experiments/21_*; -DASX_SPECIAL_LAST=0: the old order everywhere).
#ifndef ASX_SPECIAL_LAST
#define ASX_SPECIAL_LAST 1
#endif
// item of thread t: regular items e = H .. NITEMS-1 in threads [0, NITEMS - H), the H special ones in threads [NT - H, NT); -1 = none
template <int NITEMS, int H, int NT> __device__ __forceinline__ int rcol_item_of_thread(int t)
{
    constexpr bool own_wave = NITEMS - H <= NT - 64;
    if (!ASX_SPECIAL_LAST || !own_wave) return t < NITEMS ? t : -1;
    return t < NITEMS - H ? t + H : t >= NT - H ? t - (NT - H) : -1;
}
#ifndef ASX_INV_WU
#define ASX_INV_WU 1 // k_inv_cols_r: see WU_FRONT
#endif
#ifndef ASX_RCOL_LOADS
#define ASX_RCOL_LOADS 5 // row-pair pieces (two 16-byte loads each) a thread keeps in flight
#endif

// k_fwd_cols_r: grid (tiles, nops, npairs).  r2c column transforms of length 2 M1 (the zero half of the
// sample -- rows j1 >= M1 -- is never loaded, src/cross_correlation.c:159-166): M1-point complex transform of the
// packed rows, untangling between the slots of u and M1 - u, rows u and M1 - u of C (twice its value: the factor
// is taken back by k_rows_r) stored in natural row order.
// A block transforms operand op0 + blockIdx.y (0 source, 1 sample) of pair blockIdx.z, whose inputs are src_stride / smp_stride
// floats apart (0 = one track for every pair).  NTS = non-temporal stores of C (false for the plan's broadcast slot, which every
// pair's k_rows_r block reads).
template <class S1, int TC, int NT, bool NTS>
__global__ __launch_bounds__(NT, 4) void k_fwd_cols_r(const RArgs P, const float *__restrict__ src, const float *__restrict__ smp,
                                                       size_t src_stride, size_t smp_stride, float2 *__restrict__ cx,
                                                       float2 *__restrict__ cy, float *__restrict__ nrm_part, size_t pair_pitch,
                                                       float2 *__restrict__ band, unsigned op0)
{
    constexpr int M1 = S1::n, T = TC, logT = asx_ilog2(TC), H = T / 2, logH = logT - 1, Q4 = T / 4, logQ4 = logT - 2;
    static_assert(T >= 4 && (M1 & 1) == 0, "four real columns per 16-byte load, an even number of packed rows");
    __shared__ float nrm_red[NT / 64];
    const unsigned which = op0 + blockIdx.y;
    const bool is_smp = which != 0;
    const size_t pair = blockIdx.z;
    const int tile = rcol_tile_of_block(blockIdx.x, logT);
    if (tile >= P.ntiles) return; // grid.x is rounded up
    const int M2 = P.M2, c0 = tile * T;
    const float *in = is_smp ? smp + pair * smp_stride : src + pair * src_stride;
    const int data_m = is_smp ? M1 / 2 : M1; // packed rows that are not zero padding
    float2 *out = (is_smp ? cy : cx) + RWS_PAIR(pair) * pair_pitch;
    float4 *lds4 = reinterpret_cast<float4 *>(asx_lds_r);
    const LdsLayout Lc = col_layout(T, logT, NT);
    const TwPre pre = tw_prefetch_first<S1, false, true>(Lc, P.tw1);

    // Work items (m, h): rows 2m and 2m+1, real columns c0 + 4h .. 4h+3 -> slots (m, 2h) and (m, 2h+1).  The Q4 lanes h of a lane
    // group take RPQ CONSECUTIVE row pairs m = RPQ * group + i (each a 64-byte piece of two rows: the addresses a wave asks for
    // are 16 pieces apart whichever way the pairs are dealt).  That makes a lane group the owner of one BAND of 2 RPQ rows x T
    // columns, whose sum and sum of squares -- what the spectral Pearson form (pearson_spectral.hip) builds its window sums
    // from -- are RPQ register additions and two DPP steps away from the loads this pass makes anyway.  (Dealing the pairs
    // round-robin, 16 lanes of a wave per band of eight rows: five 16-lane reductions per thread, k_fwd_cols_r +3 %,
    // profiles/r5_experiments/04_*.)
    constexpr int QN = NT / Q4, RPQ = rcol_rows_per_group(M1, NT, T);
    static_assert(Q4 == 4, "sixteen real columns: four lanes per row pair (the quad reductions below)");
    static_assert(M1 % RPQ == 0 && (M1 / 2) % RPQ == 0 && RPQ <= ASX_RCOL_LOADS && RPQ * QN >= M1, "whole bands in both tracks");
    const int grp = threadIdx.x >> logQ4, h = threadIdx.x & (Q4 - 1), m0 = grp * RPQ;
    float ss = 0.f, q1 = 0.f;
    {
        float4 a[RPQ], b[RPQ];
        float sq[RPQ]; // a row pair's eight squares: one chain of eight roundings; the pairs are then added as a tree (below)
        static_for<0, RPQ>([&](auto I) __attribute__((always_inline)) {
            const int m = m0 + decltype(I)::value;
            a[I] = b[I] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < data_m) { // also false past the end of the tile (m >= M1 >= data_m)
                const float *p = in + (size_t)(2 * m) * M2 + c0 + 4 * h;
                a[I] = *reinterpret_cast<const float4 *>(p);
                b[I] = *reinterpret_cast<const float4 *>(p + M2);
            }
        });
        static_for<0, RPQ>([&](auto I) __attribute__((always_inline)) {
            const int m = m0 + decltype(I)::value;
            if (m < M1) {
                float4 *o = lds4 + (m << logH) + 2 * h;
                o[0] = make_float4(a[I].x, b[I].x, a[I].y, b[I].y);
                o[1] = make_float4(a[I].z, b[I].z, a[I].w, b[I].w);
            }
            // (row pairs past the end of the tile or in the sample's zero half hold zeros)
            sq[I] = fmaf(a[I].x, a[I].x, fmaf(a[I].y, a[I].y, fmaf(a[I].z, a[I].z, a[I].w * a[I].w)));
            sq[I] = fmaf(b[I].x, b[I].x, fmaf(b[I].y, b[I].y, fmaf(b[I].z, b[I].z, fmaf(b[I].w, b[I].w, sq[I]))));
            if (band) q1 += ((a[I].x + a[I].y) + (a[I].z + a[I].w)) + ((b[I].x + b[I].y) + (b[I].z + b[I].w)); // kernel-uniform
        });
        // The band's sum of squares feeds the spectral Pearson form's error bound (asx_spec_pick, xcorr_dev.h: <= 16 u relative): eight
        // roundings per row pair, ceil(log2 RPQ) <= 3 down this tree, two in the quad sum = 13 u.  (Round 5 ran ONE chain through all
        // RPQ pairs: 8 RPQ + 2 = 42 roundings, which that bound did not cover -- ADVICE r5.)
        ss = tree_sum<RPQ>(sq);
    }
    if (band) {
        const float r1 = quad_sum(q1), r2 = quad_sum(ss);
        // tile-major: a block's band sums are one contiguous run (row-major -- adjacent tiles 8 bytes apart, sixteen blocks of
        // eight XCDs writing into every 128-byte line: k_fwd_cols_r +2 % at 600 x 2400, +7 % at 400 x 1200, profiles/r5_experiments/04_*)
        if (h == 0 && m0 < data_m)
            band[(((size_t)pair * 2 + which) * (size_t)P.ntiles + tile) * (size_t)(M1 / RPQ) + grp] = make_float2(r1, r2);
    }
    // |source|^2 and |sample|^2 (the scale of the float32 error bound of the peak search) from the pass that reads
    // the inputs anyway
    ss = wave_sum_f32(ss);
    if ((threadIdx.x & 63) == 0) nrm_red[threadIdx.x >> 6] = ss;
    __syncthreads();
    (void)lds_fft_static_head<S1, false, true>(lds4, Lc, P.tw1, pre); // every stage but the innermost one
    // A thread that has no work item in the store phase below (rcol_item_of_thread).  (Thread 0's wave waited for this store before its first butterfly
    // of that phase, at the end of the block's life where nothing hides it: 0.997 -> 0.979 ms, profiles/r5_experiments/20_*.)
    if (threadIdx.x == NT - H - 1) {
        float t = nrm_red[0];
        for (int w = 1; w < NT / 64; w++) t += nrm_red[w];
        nrm_part[(pair * 2 + which) * (size_t)P.ntiles + tile] = t;
    }
    // ---- the innermost stage (radix RL, RL consecutive slots per butterfly, no twiddles), untangling and the stores, all
    // from registers.  Butterfly b of a column pair yields the frequencies u_b + MB t (t < RL, MB = M1 / RL, u_b = digit
    // swap of b); their untangling partners M1 - u_b - MB t are element RL-1-t of butterfly b' (u_b' = MB - u_b).  A work
    // item runs BOTH butterflies and stores the 2 RL rows
    //     2 C[u] = S + w (-i D),  2 C[M1-u] = conj(S - w (-i D)),  S = Z[u] + conj Z[M1-u], D = Z[u] - conj Z[M1-u], w = w_{2 M1}^u
    // (w = w_{2 M1}^u_b times the compile-time root w_{2 RL}^t): no LDS pass for the result, no index table.  The two
    // butterflies that pair with themselves (u_b = 0, whose partners are its own elements RL - t and which also yields
    // row M1; u_b = MB/2) share the work item v = 0.
    static_assert(S1::nstages == 3, "three-stage column schedules");
    constexpr int RL = S1::stage(2).R, R0c = S1::stage(0).R, R1c = S1::stage(1).R, MB = M1 / RL;
    static_assert(S1::stage(2).q == 1 && MB == R0c * R1c && MB % 2 == 0, "innermost stage of consecutive slots");
    constexpr int NBPAIRS = (MB / 2) * H;
    static_assert(NBPAIRS <= NT - 1, "one work item per thread at most, none for thread NT - H - 1 (the block's norm)");
    if (const int e = rcol_item_of_thread<NBPAIRS, H, NT>(threadIdx.x); e >= 0) {
        const int g = e & (H - 1), v = e >> logH;  // v = u_b in [0, MB/2)
        const int ub = v, ubp = v == 0 ? MB / 2 : MB - v;
        const int d1 = ub / R0c, d0 = ub - d1 * R0c, e1 = ubp / R0c, e0 = ubp - e1 * R0c;
        const float4 *pa = lds4 + (((d0 * R1c + d1) * RL) << logH) + g, *pb = lds4 + (((e0 * R1c + e1) * RL) << logH) + g;
        Cx2 za[RL], zb[RL];
        static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
            za[TT] = lds_get(pa + (decltype(TT)::value << logH));
            zb[TT] = lds_get(pb + (decltype(TT)::value << logH));
        });
        Bfly<RL, false>::run(za);
        Bfly<RL, false>::run(zb);
        const int cg = 2 * g;
        auto row = [&](int u, Cx2 c, bool conj) __attribute__((always_inline)) {
            st_f4(out + (size_t)u * M2 + c0 + cg, conj ? make_float4(c.re.x, -c.im.x, c.re.y, -c.im.y)
                                                       : make_float4(c.re.x, c.im.x, c.re.y, c.im.y), NTS && (ASX_RNT & 2));
        };
        if (v != 0) {
            const float2 wu = tw_F(P, (uint32_t)ub * (uint32_t)M2); // w_{2 M1}^u_b = w_F^(u_b M2)
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 a = za[t], bq = zb[RL - 1 - t];
                const Cx2 S = Cx2{ a.re + bq.re, a.im - bq.im };
                const Cx2 Dm = Cx2{ a.im + bq.im, bq.re - a.re }; // -i D
                const Cx2 wd = mul_root<2 * RL, t, false>(mulw(Dm, wu));
                row(ub + MB * t, S + wd, false);
                row(ubp + MB * (RL - 1 - t), S - wd, true);
            });
        } else {
            // u_b = 0: Z[MB t] pairs with Z[MB (RL - t)] (t = 0 with itself: rows 0 and M1); w = w_{2 RL}^t
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 a = za[t], bq = za[(RL - t) % RL];
                const Cx2 S = Cx2{ a.re + bq.re, a.im - bq.im };
                const Cx2 Dm = Cx2{ a.im + bq.im, bq.re - a.re };
                const Cx2 wd = mul_root<2 * RL, t, false>(Dm);
                row(MB * t, S + wd, false);
                if constexpr (t == 0) row(M1, S - wd, true);
            });
            // u_b = MB/2: Z[MB/2 + MB t] pairs with Z[MB/2 + MB (RL-1-t)]; w = w_{4 RL}^(2t + 1)
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 a = zb[t], bq = zb[RL - 1 - t];
                const Cx2 S = Cx2{ a.re + bq.re, a.im - bq.im };
                const Cx2 Dm = Cx2{ a.im + bq.im, bq.re - a.re };
                const Cx2 wd = mul_root<4 * RL, 2 * t + 1, false>(Dm);
                row(MB / 2 + MB * t, S + wd, false);
            });
        }
    }
}

// grid (ceil(per / 256), npairs): pool calls.  Pair i of the group (the call's pair A.first + i) as {source a, sample b}: from the caller's
// row, or a = (first + i) / nsmp, b = (first + i) % nsmp.  An index outside its pool gives slot 0 and ASX_POOL_INVALID, so that no
// kernel reads outside the pools.  Block x = 0 writes the record; every block copies its share of the two slots' norm partials and
// band sums into pair i's places (k_bcast_aux's copy with a slot per pair).  per = ntiles, or ntiles * nbands with band sums.
__global__ __launch_bounds__(256) void k_pool_resolve(AsxPoolArgs A, AsxPoolPair *__restrict__ out, float *__restrict__ nrm,
                                                       float2 *__restrict__ band, int ntiles, int nbands)
{
    const size_t pair = blockIdx.y;
    const uint64_t k = A.first + pair;
    int64_t a, b;
    if (A.rows) { a = A.rows[2 * k]; b = A.rows[2 * k + 1]; }
    else { a = (int64_t)(k / A.nsmp); b = (int64_t)(k - (uint64_t)a * A.nsmp); }
    const bool ok = a >= 0 && (uint64_t)a < A.nsrc && b >= 0 && (uint64_t)b < A.nsmp;
    if (!ok) a = b = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        AsxPoolPair r;
        r.sx = (uint32_t)a; r.sy = (uint32_t)b;
        r.flags = ok ? 0u : ASX_POOL_INVALID; r.pad = 0u;
        r.src_off = (uint64_t)a * A.src_stride;
        r.smp_off = (uint64_t)b * A.smp_stride;
        out[pair] = r;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ntiles) {
        nrm[(pair * 2 + 0) * (size_t)ntiles + i] = A.nrm[((size_t)a * 2 + 0) * ntiles + i];
        nrm[(pair * 2 + 1) * (size_t)ntiles + i] = A.nrm[((size_t)b * 2 + 1) * ntiles + i];
    }
    const int nb = ntiles * nbands;
    if (band && i < nb) {
        band[(pair * 2 + 0) * (size_t)nb + i] = A.band[((size_t)a * 2 + 0) * nb + i];
        band[(pair * 2 + 1) * (size_t)nb + i] = A.band[((size_t)b * 2 + 1) * nb + i];
    }
}

// grid (ceil(per / 256), npairs): the broadcast operand's norm partials and band sums (the slot's pair 0, operand `which`) into
// every pair's place in the group's workspaces, where k_rows_r and the spectral Pearson form read them.  per = ntiles (norms)
// + ntiles * nbands (band sums, when band != null).
__global__ __launch_bounds__(256) void k_bcast_aux(const float *__restrict__ snrm, const float2 *__restrict__ sband,
                                                    float *__restrict__ nrm, float2 *__restrict__ band, int ntiles, int nbands,
                                                    unsigned which)
{
    const size_t pair = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ntiles) nrm[(pair * 2 + which) * (size_t)ntiles + i] = snrm[(size_t)which * ntiles + i];
    const int nb = ntiles * nbands;
    if (band && i < nb) band[(pair * 2 + which) * (size_t)nb + i] = sband[(size_t)which * nb + i];
}

// k_inv_cols_r's r_out: the argument, or null where the instance has none (constexpr: the compiler then drops the dumping code as it
// reads it, as it did for the pruned kernels' literal null; dropped later, the same kernels came out with other registers)
__device__ __forceinline__ constexpr float *rcol_r_out() { return nullptr; }
__device__ __forceinline__ constexpr float *rcol_r_out(float *p) { return p; }

// ---------------------------------------------------------------------------
// k_inv_cols_r: grid (npairs, tiles).  c2r column transforms of length 2 M1 from the rows k1 = 0 .. M1 of Q: tangling
// between rows u and M1 - u into the slots of the M1-point inverse transform, whose outputs are the packed rows
// z[m] = r[2m] + i r[2m+1] of the tile's T real columns; the last stage is consumed from registers (r reaches
// neither HBM nor LDS): |.|-argmax with the reference's tie / sign / NaN rules (src/cross_correlation.c:52-67),
// lags inside the float32 error window appended to the pair's candidate list, as in k_inv_cols.
// Lag of component h of slot (m, g): h = 0 re0, 1 im0, 2 re1, 3 im1 -> (2m + (h & 1)) * M2 + c0 + 2g + (h >> 1).
// ---------------------------------------------------------------------------
// Sel (asx_internal.h) says which lags compete.  Sel::masks: only the lags of Z = sel.window_of(pair) compete, and Z.seed is the one
// whose key is signed; out-of-window values become NaN in the fast scan (a NaN never wins there and is never a candidate) and are
// skipped everywhere else; r_out still receives every lag.  One instance per selection, so that the full window runs the
// <AsxSelAll> instance untouched: AsxWin the plan's window (asx_plan_set_lag_window); AsxWinRows the pair's row in device memory,
// read once per block in front of the tile loads (an invalid row holds no lag, asx_win_row); AsxSelTopk<ZC> the pass's window, seed
// and the zones around the pair's earlier entries from its record (passes 2..k of asx_xcorr_topk_f32_dev), left out of every scan,
// candidate list and tile peak of the pass; AsxSelPrune<FIRST> the pruned pass below, which also names the block's tile.
// Out: float, r_out -- or nothing: the pruned pass has no such argument.
// The body is written here and nowhere else, and in the __global__ itself rather than in a function it calls: a call boundary
// changes the instruction stream (see rows_r_body), and the <AsxSelAll> instance has to stay the kernel it was.
template <class S1, int TC, int NT, class Sel, class... Out>
__global__ __launch_bounds__(NT, 4) void k_inv_cols_r(const RArgs P, const float2 *__restrict__ qi, size_t pair_pitch,
                                                       AsxPeakWs W, Out *__restrict__... r_arg, unsigned first_gen, Sel sel)
{
    static_assert(sizeof...(Out) <= 1, "r_out or nothing");
    if (!asx_sel_takes(sel, rcol_tile_of_block(blockIdx.y, asx_ilog2(TC)), P.M2, TC)) return; // (the pruned pass: before anything else is asked)
    constexpr bool WIN = Sel::masks;
    const auto Z = sel.window_of(blockIdx.x, P.N);
    float *const r_out = rcol_r_out(r_arg...);
    constexpr int M1 = S1::n, T = TC, logT = asx_ilog2(TC), H = T / 2, logH = logT - 1;
    __shared__ asx_peak_t red[NT / 64];
    __shared__ asx_peak_t s_run0;
    __shared__ float s_b2;
    // TILE-major launch order, grid (npairs, tiles): the tiles of one pair are spread over the life of the launch, so the running
    // maximum a block fetches at its start (`run0`) already holds the maximum of the tiles before it, and a tile that cannot hold
    // the peak -- nearly all of them -- never enters the candidate path with its returning atomic.  Pair-major (the 150 tiles of a
    // pair resident together, run0 == 0 for all of them): 0.405 against 0.367 ms at 600 rows, 0.423 against 0.299 ms per 1024 pairs
    // at 300 rows (profiles/r5_experiments/02_*).
    const size_t pair = blockIdx.x;
    const int tile = asx_sel_tile(sel, rcol_tile_of_block(blockIdx.y, logT)); // its place in the grid, or the tile the pruned pass names
    if (tile * T >= P.M2) return; // the tile count is rounded up; the tile width is this kernel's own (it reads only)
    {
        // Stagger: the blocks that share a CU run the same program -- a load phase (the tile's rows), then compute phases of about
        // the same length -- and, started together, stay in step: both wait for memory, then both compute.  The blocks of the FIRST
        // generation start half a block's life apart, by the parity of their position in the launch order (the split that measured
        // best); later generations inherit the offset.  0.370 -> 0.349 ms at 600 rows, -3 .. -6 % at 400 (rows and
        // forward columns: nothing, profiles/r5_experiments/05_*).  Speed only.  (What it staggers is not the two blocks of a CU -- those are
        // 256 apart in launch order, same parity -- but HALF THE CHIP against the other half: a read-only kernel whose blocks all take the
        // same time otherwise loads in step and computes in step chip-wide, and the memory system idles between the bursts.  On the round's
        // final kernel: 0.373 ms without, 0.301 with; more phases or other lengths: the same, profiles/r5_experiments/25_*.)
        // The first generation = the blocks resident at once: two per CU for 600- and 400-row tiles, four for 300-row tiles.  (Round 5 had
        // left the 300-row instance alone -- with the FIRST 512 of its 1024 resident blocks treated that way it was 1.5 % slower; with the
        // whole first generation: 0.310 -> 0.278 ms per 1024 pairs of N = 144 000, profiles/r5_experiments/25_*.)
        // first_gen comes from the launcher (occupancy of this kernel x the device's CUs: nothing here assumes 256 CUs).
        const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
        if (gridDim.x * gridDim.y > first_gen && lin < first_gen && (lin & 1u)) // (a launch of one generation has nobody to inherit the offset)
            for (unsigned i = 0; i < (unsigned)(M1 * 27 / 64 / 2); i += 16) __builtin_amdgcn_s_sleep(16); // half a block's life; 64 cycles per unit
    }
    const double shift = W.shift ? W.shift[pair] : 0.0; // non-zero only in the second look (asx_api.hip)
    const int M2 = P.M2, c0 = tile * T;
    const float2 *in = qi + RWS_PAIR(pair) * pair_pitch;
    float4 *lds4 = reinterpret_cast<float4 *>(asx_lds_r);
    const LdsLayout Lc = col_layout(T, logT, NT);
    // the pair's running maximum so far and the width of the near-maximum window: fetched now, used behind the barriers
    const float b2_early = W.bound2[pair];
    // (thread 0 asks for the running maximum here and leaves it in LDS BEHIND the tile loads: stored at once, its wave sat out a memory
    // round trip before it issued its share of the tile's loads, and the block's first barrier waited for that wave: 0.3195 -> 0.3145 ms
    // at 600 rows, -1 % at 400; every thread asking instead: +3 % at 600 rows, profiles/r5_experiments/20_*)
    asx_peak_t run0_early = 0;
    if (threadIdx.x == 0) run0_early = W.pairmax[pair];
    // ---- first stage to run (the innermost, radix RL = R_last, RL consecutive slots per butterfly), fed from HBM --------
    // Butterfly b of a column pair holds the frequencies u_b + MB t (t < RL, MB = M1 / RL, u_b = digit swap of b); their
    // tangling partners M1 - u_b - MB t are element RL-1-t of butterfly b' (u_b' = MB - u_b).  A work item takes BOTH
    // butterflies: 2 RL rows of 16 bytes straight from HBM, the tangling in registers
    //     Z'[u] = S + i conj(w) D,  Z'[M1-u] = conj(S - i conj(w) D),  S = Q[u] + conj Q[M1-u], D = Q[u] - conj Q[M1-u], w = w_{2 M1}^u
    // (w = w_{2 M1}^u_b times the compile-time root w_{2 RL}^t), the two inverse butterflies, 2 RL slots written: no fill
    // phase, no index table, no barrier before the first stage.  u_b = 0 (rows 0, MB, ..., M1: the extra row is its own
    // partner row set) and u_b = MB/2 pair with themselves: one butterfly.
    static_assert(S1::nstages == 3, "three-stage column schedules");
    constexpr StageK KL = S1::stage(2), KM = S1::stage(1);
    constexpr int RL = KL.R, R0c = S1::stage(0).R, R1c = KM.R, MB = M1 / RL;
    static_assert(KL.q == 1 && MB == R0c * R1c && MB % 2 == 0, "innermost stage of consecutive slots");
    constexpr int NITEMS = (MB / 2) * H; // v = 0 takes both butterflies that pair with themselves (u_b = 0 and MB/2)
    const size_t sblock = pair * (size_t)(P.M2 / T) + tile; (void)sblock;
    RSTAMP(2, sblock, 0);
    const TwPre pre_mid = tw_prefetch_exec<S1, 1, true, true, true>(Lc, P.tw1);
    static_assert(NITEMS <= NT, "one work item per thread at most");
    if (const int e = rcol_item_of_thread<NITEMS, H, NT>(threadIdx.x); e >= 0) {
        const int g = e & (H - 1), v = e >> logH;  // v = u_b in [0, MB/2)
        const int ub = v, ubp = v == 0 ? MB / 2 : MB - v; // first rows of the two butterflies' row sets
        const float2 *ca = in + (size_t)ub * M2 + c0 + 2 * g, *cb = in + (size_t)ubp * M2 + c0 + 2 * g;
        // The tangling twiddle w_{2 M1}^u_b = w_F^(u_b M2).  WU_FRONT: asked for IN FRONT of the rows (vmcnt completes in order) and used by
        // both branches below (u_b = 0: exactly 1), which keeps the compiler from sinking the look-up into the one branch that needs it,
        // behind the rows, where its second table value was only issued when the rows had arrived: 0.317 -> 0.3055 ms at 600 rows.  The
        // 400- and 300-row instances lose 1 - 1.6 % with it (profiles/r5_experiments/23_*) and keep the look-up where it was.
        constexpr bool WU_FRONT = ASX_INV_WU && M1 == 600;
        float2 wu_all = make_float2(1.f, 0.f);
        if constexpr (WU_FRONT) wu_all = tw_F(P, (uint32_t)ub * (uint32_t)M2);
        Cx2 A[RL], B[RL];
        static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
            constexpr int t = decltype(TT)::value;
            const float4 x = ld_f4(ca + (size_t)(t * MB) * M2, ASX_RNT & 1);
            const float4 y = ld_f4(cb + (size_t)(t * MB) * M2, ASX_RNT & 1);
            A[t] = Cx2{ v2f{ x.x, x.z }, v2f{ x.y, x.w } };
            B[t] = Cx2{ v2f{ y.x, y.z }, v2f{ y.y, y.w } };
        });
        Cx2 za[RL], zb[RL];
        if (v != 0) {
            const float2 wu = WU_FRONT ? wu_all : tw_F(P, (uint32_t)ub * (uint32_t)M2);
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 b = B[RL - 1 - t];
                const Cx2 S = Cx2{ A[t].re + b.re, A[t].im - b.im };
                const Cx2 D = Cx2{ A[t].re - b.re, A[t].im + b.im };
                const Cx2 tt = mul_pos_i(mul_root<2 * RL, t, true>(mulwc(D, wu))); // i conj(w) D, w = wu * w_{2 RL}^t
                za[t] = S + tt;
                const Cx2 m = S - tt;
                zb[RL - 1 - t] = Cx2{ m.re, -m.im };
            });
        } else {
            // u_b = 0: Q[MB t] pairs with Q[MB (RL - t)], t = 0 with the extra row M1; u_b = MB/2: within the butterfly
            const float4 xm = ld_f4(in + (size_t)M1 * M2 + c0 + 2 * g, ASX_RNT & 1);
            const Cx2 QM = Cx2{ v2f{ xm.x, xm.z }, v2f{ xm.y, xm.w } };
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                Cx2 b = QM;
                if constexpr (t != 0) b = A[RL - t];
                const Cx2 S = Cx2{ A[t].re + b.re, A[t].im - b.im };
                const Cx2 D = Cx2{ A[t].re - b.re, A[t].im + b.im };
                if constexpr (WU_FRONT) za[t] = S + mul_pos_i(mul_root<2 * RL, t, true>(mulwc(D, wu_all))); // wu_all = w_F^0 = 1 here
                else za[t] = S + mul_pos_i(mul_root<2 * RL, t, true>(D));
            });
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 b = B[RL - 1 - t];
                const Cx2 S = Cx2{ B[t].re + b.re, B[t].im - b.im };
                const Cx2 D = Cx2{ B[t].re - b.re, B[t].im + b.im };
                zb[t] = S + mul_pos_i(mul_root<4 * RL, 2 * t + 1, true>(D));
            });
        }
        // slots: butterfly b = d0 * R1 + d1 for u_b = d0 + R0 * d1
        const int d1 = ub / R0c, d0 = ub - d1 * R0c, e1 = ubp / R0c, e0 = ubp - e1 * R0c;
        float4 *pa = lds4 + (((d0 * R1c + d1) * RL) << logH) + g, *pb = lds4 + (((e0 * R1c + e1) * RL) << logH) + g;
        Bfly<RL, true>::run(za);
        Bfly<RL, true>::run(zb);
        static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
            lds_put(pa + (decltype(TT)::value << logH), za[TT]);
            lds_put(pb + (decltype(TT)::value << logH), zb[TT]);
        });
    }
    if (threadIdx.x == 0) {
        s_run0 = run0_early;
        s_b2 = b2_early;
    }
    RSTAMP(2, sblock, 1);
    // A digitally silent track (zero norm: r is exactly zero everywhere): the running maximum stays zero, which k_finalize
    // reads as index 0, the reference's answer (see k_inv_cols).  Checked HERE, behind the tile loads: in front of them the
    // block waited a memory latency for this one float before it issued anything.  Block-uniform.
    if (b2_early == 0.f && r_out == nullptr) return;
    __syncthreads();
    const TwPre pre_last = lds_fft_static_steps<S1, true, true, S1::nstages - 1, true, 1>(lds4, Lc, P.tw1, pre_mid);
    RSTAMP(2, sblock, 2);
    const asx_peak_t run0 = s_run0;
    const float b2 = s_b2;
    auto last_stage = [&](auto &&sink) __attribute__((always_inline)) {
        lds_last_stage_static<S1, true, true>(lds4, Lc, P.tw1, pre_last, sink);
    };
    const uint32_t uM2 = (uint32_t)M2;
    // the seed's tile takes the general form (lag 0's tile without a window)
    const uint32_t seed = WIN ? Z.seed : 0u;
    const bool fast = (WIN ? (uint32_t)tile != (seed % uM2) / (uint32_t)T : tile != 0) && (r_out == nullptr) && shift == 0.0;
    auto inw = [&](uint32_t idx) __attribute__((always_inline)) { return !WIN || asx_win_has(Z, idx); };
    auto examine_again = [&](float thr) __attribute__((always_inline)) {
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + (uint32_t)(h & 1) * uM2 + (uint32_t)(h >> 1);
                    const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                    if (inw(idx) && key >= thr) cand_append(W, pair, idx, key);
                }
            });
        });
    };
    float thr_again = 0.f;
    bool again = false;
    if (fast) {
        // The scan keeps ONE number per thread: the largest |r| of its 4 R lags (NaNs drop out of fmaxf).  Which lag it was is
        // looked up again only by a tile that can matter (below): with the tile-major launch order nearly every tile finds its
        // maximum under the window of the running maximum it fetched at its start and is done behind one barrier -- no index,
        // no second maximum, no atomic.  (Tracking index, slot and runner-up in the scan: 17 instead of 3 instructions per slot,
        // k_inv_cols_r 0.353 against 0.332 ms at 600 rows, 1.15 against 1.08 ms per 1024 pairs at 400, equal at 600 x 480,
        // 0.31 against 0.32 at 300 rows; profiles/r5_experiments/06_*.)
        float best_m = -INFINITY;
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                if constexpr (WIN) {
                    const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
                    const float a0 = inw(i0) ? fabsf(v[t].re.x) : NAN, a1 = inw(i0 + uM2) ? fabsf(v[t].im.x) : NAN;
                    const float a2 = inw(i0 + 1) ? fabsf(v[t].re.y) : NAN, a3 = inw(i0 + uM2 + 1) ? fabsf(v[t].im.y) : NAN;
                    best_m = fmaxf(fmaxf(best_m, fmaxf(a0, a1)), fmaxf(a2, a3));
                } else {
                    best_m = fmaxf(fmaxf(best_m, fmaxf(fabsf(v[t].re.x), fabsf(v[t].im.x))), fmaxf(fabsf(v[t].re.y), fabsf(v[t].im.y)));
                }
            });
        });
        RSTAMP(2, sblock, 4);
        const float wmax = wave_max_nonneg(fmaxf(best_m, 0.f));
        float *redf = reinterpret_cast<float *>(red);
        if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = wmax;
        __syncthreads();
        float bm = redf[0];
        for (int w = 1; w < NT / 64; w++) bm = fmaxf(bm, redf[w]);
        // the final maximum is >= run0: below run0's window nothing of this tile can be the peak or near it (run0 == 0, nothing
        // seen yet, gives a NaN threshold: no exit)
        if (bm < near_max_threshold(peak_key(run0), b2)) return; // block-uniform
        RSTAMP(2, sblock, 5);
        // ---- a tile that can matter (the first generation of blocks, record setters, the peak's tile): the last stage again for
        // the threads that hold its maximum or a near-maximum -- smallest lag and signed value of the maximum, candidates.
        // (The holders publishing for themselves, without the fold and its two barriers: the same time, and 8 bytes of scratch.)
        const float thr = near_max_threshold(fmaxf(bm, peak_key(run0)), b2); // key(run0) is NaN when nothing was seen: fmaxf drops it
        uint32_t my_idx = 0xFFFFFFFFu;
        float my_val = 0.f;
        if (best_m >= thr || best_m == bm) {
            last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
                static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                    constexpr int t = decltype(TT)::value;
                    const float val[4] = { v[t].re.x, v[t].re.y, v[t].im.x, v[t].im.y }; // in lag order: i0, i0 + 1, i0 + M2, i0 + M2 + 1
                    const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const uint32_t idx = i0 + (uint32_t)(h >> 1) * uM2 + (uint32_t)(h & 1);
                        const float a = inw(idx) ? fabsf(val[h]) : NAN;
                        if (a == bm && idx < my_idx) { my_idx = idx; my_val = val[h]; }
                        if (a >= thr) cand_append(W, pair, idx, a);
                    }
                });
            });
        }
        __syncthreads(); // redf is read by every thread above
        const asx_peak_t mine = my_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(bm, my_idx);
        const asx_peak_t tb = block_peak_max(mine, red);
        if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], tb); red[0] = tb; }
        __syncthreads();
        // the one thread that holds the tile's best lag: its SIGNED value (the key is |r|) for the spectral Pearson form
        if (W.tile_peak && mine != 0 && mine == red[0]) W.tile_peak[pair * (size_t)(P.M2 / T) + tile] = my_val;
    } else {
        // general form: first tile (lag 0 competes signed), r dumped for tests, shifted keys of the second look
        float best_key = -INFINITY, best_val = 0.f;
        uint32_t best_idx = 0xFFFFFFFFu;
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + (uint32_t)(h & 1) * uM2 + (uint32_t)(h >> 1);
                    const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                    if (inw(idx) && (key > best_key || (key == best_key && idx < best_idx) || best_idx == 0xFFFFFFFFu)) { best_key = key; best_idx = idx; best_val = val[h]; }
                    if (r_out) r_out[pair * (size_t)P.nout + idx] = val[h];
                }
            });
        });
        const asx_peak_t mine = best_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(best_key, best_idx);
        asx_peak_t best = block_peak_max(mine, red);
        if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], best); red[0] = best; }
        __syncthreads();
        if (W.tile_peak && mine != 0 && mine == red[0]) W.tile_peak[pair * (size_t)(P.M2 / T) + tile] = best_val; // one thread: indices are unique
        const float thr = near_max_threshold(peak_key(peak_max(red[0], run0)), b2);
        again = best_key >= thr;
        thr_again = thr;
    }
    if (again) examine_again(thr_again);
    RSTAMP(2, sblock, 3);
}

// ---------------------------------------------------------------------------
// The pruned inverse pass (asx_launch_inv_cols_r with an AsxPrune; every lag competes, no r_out, no second look): k_tile_bounds,
// k_inv_cols_r<..., AsxSelPrune<true>> on two tiles per pair, k_prune_select, k_inv_cols_r<..., AsxSelPrune<false>> on the tiles that are left.
//
// The bound.  Column j2 of r is the c2r transform of column j2 of Q: with the tangling Z'[u] = S + i conj(w) D, S = Q[u] + conj Q[M1-u],
// D = Q[u] - conj Q[M1-u], |Z'[u]|^2 + |Z'[M1-u]|^2 = 2 |S|^2 + 2 |D|^2 = 4 (|Q[u]|^2 + |Q[M1-u]|^2) (u = M1/2: |Z'|^2 = 4 |Q|^2), and
// for u = 0, with Q[0] = a + ib and Q[M1] = c + id, |Z'[0]|^2 = 2 (a - d)^2 + 2 (c - b)^2 <= 4 (|Q[0]|^2 + |Q[M1]|^2).  The M1-point
// inverse transform is unnormalised, sum_m |z[m]|^2 = M1 sum_u |Z'[u]|^2, and r[2m] + i r[2m+1] = z[m], so for ANY complex rows
//     sum_j1 r[j1][j2]^2 <= 4 M1 sum_{k1 = 0 .. M1} |Q[k1][j2]|^2
// with equality but for rows 0 and M1, which count twice here: in exact arithmetic they are real and Parseval gives them the weight
// 1 (h(0) = h(M1) = 1, h = 2 elsewhere), but the float32 rows carry an imaginary residue that the tangling mixes in (a - d, c - b),
// and the weight 2 covers every value of it -- two rows of M1 + 1, a bound larger by 1 / M1 at most.  No element of a tile exceeds
// the tile's Frobenius norm:
//     |r[j1][j2]| <= sqrt(4 M1 E),  E = sum over the tile's sixteen columns and all rows of |Q|^2 = the sum over k1 of eng.
// delta (ASX_PRUNE_DELTA, asx_internal.h) covers the float32 roundings on both sides of that; a tile whose energy sum lies under
// ASX_PRUNE_FLOOR_PER_TERM times its number of terms gets the bound +infinity (the squares of a very quiet pair underflow in
// float32 although r itself does not): it is never skipped.
// ---------------------------------------------------------------------------
// grid (npairs, nsl), tp threads in whole waves, tp = the tiles rounded up to 32 and nsl = 1024 / tp: ub[pair][tile] and the pair's largest-bound tile
// from eng[pair][k1][tile].  The rows are dealt to the nsl slices, k1 = s mod nsl to block (pair, s), which sums its rows in float64 in
// increasing k1, a tile per thread, and leaves part[pair][s][tile].  The block of a pair that draws the pair's last ticket adds the
// slices in slice order and states the bounds: the same eng gives the same bits, whichever block that is.  It puts the ticket back
// to zero for the next launch on this stream (U.ticket is zeroed once, when the plan is made).
//
// The hand-over inside the launch RESTS ON THE CODE GENERATED FOR THE gfx942 FAMILY (gfx950 included), NOT ON THE LANGUAGE'S MEMORY
// MODEL.  The model asks for a release in front of the ticket; at agent scope that is a write-back of the XCD's whole L2
// (buffer_wbl2 sc1), 744 of them per launch, and the kernel takes 25 us with it instead of 16 (EXPERIMENTS.md round 8).  What stands
// here instead, every access to part an atomic one so that none of it is a data race:
//   - a slice's sums leave as relaxed agent-scope atomic stores: global_store_dwordx2 ... sc1, written through to memory;
//   - every wave waits for its stores' acknowledgement (s_waitcnt vmcnt(0)) in front of the barrier, so all of the block's sums are in
//     memory before its one lane draws the ticket, an agent-scope atomic add (relaxed: NO release);
//   - the last arriver's agent-scope acquire fence (buffer_inv sc1) stands behind its ticket and in front of the barrier behind which
//     its threads load the sums, as relaxed agent-scope atomic loads (sc1).
// Relaxed atomics alone order nothing between the stores and the ticket; the explicit wait does, on this hardware.
// tests/test_rows_energy_isa.py pins each instruction of that sequence in the built library: a compiler that lowers any of it
// differently fails there.  That test knows one compiler (ROCm 7.2, tests/test_kernel_isa_order.py: PINNED_ROCM) and skips elsewhere,
// so any other compiler gets the release the model asks for on the ticket, and with it the slower, portable kernel, until the
// sequence has been read and stated for that compiler too.
#if defined(HIP_VERSION_MAJOR) && HIP_VERSION_MAJOR == 7 && HIP_VERSION_MINOR == 2
constexpr int BOUNDS_TICKET_ORDER = __ATOMIC_RELAXED;
#else
constexpr int BOUNDS_TICKET_ORDER = __ATOMIC_RELEASE;
#endif
constexpr int BOUNDS_ROWS_IN_FLIGHT = 16, BOUNDS_SLICES_IN_FLIGHT = 8;

// load(i), i = 0 .. n-1, added in float64 in increasing i with DEPTH loads in flight; past the last term a thread loads that term
// again and adds +0.0 in its place, which leaves a sum of non-negative terms (or a NaN) as it is
template <int DEPTH, class Load>
__device__ __forceinline__ double sum_in_order(int n, Load load)
{
    double sum = 0.0;
    for (int i0 = 0; i0 < n; i0 += DEPTH) {
        double v[DEPTH];
#pragma unroll
        for (int i = 0; i < DEPTH; i++) v[i] = load(i0 + i < n ? i0 + i : n - 1);
#pragma unroll
        for (int i = 0; i < DEPTH; i++) sum += i0 + i < n ? v[i] : 0.0;
    }
    return sum;
}

__global__ __launch_bounds__(1024) void k_tile_bounds(const float *__restrict__ eng, float *__restrict__ ub, int *__restrict__ best,
                                                       double *part, unsigned *__restrict__ ticket, int nrows, int ntiles,
                                                       double scale, double floor)
{
    __shared__ unsigned long long tops[16];
    __shared__ int last;
    const size_t pair = blockIdx.x;
    const int tile = threadIdx.x, tp = (ntiles + 31) & ~31, sl = blockIdx.y, nsl = gridDim.y; // (whole waves: blockDim.x may exceed tp)
    unsigned long long *pp = reinterpret_cast<unsigned long long *>(part + pair * 1024);
    if (tile < ntiles) {
        const float *e = eng + pair * (size_t)nrows * ntiles + (size_t)sl * ntiles + tile;
        const size_t step = (size_t)nsl * ntiles;
        const double sum = sum_in_order<BOUNDS_ROWS_IN_FLIGHT>((nrows - sl + nsl - 1) / nsl, // rows of the slice
                                                               [=](int i) { return (double)e[(size_t)i * step]; });
        __hip_atomic_store(pp + sl * tp + tile, (unsigned long long)__double_as_longlong(sum), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned drawn = __hip_atomic_fetch_add(ticket + pair, 1u, BOUNDS_TICKET_ORDER, __HIP_MEMORY_SCOPE_AGENT);
        last = drawn == (unsigned)nsl - 1u;
        if (last) {
            __hip_atomic_store(ticket + pair, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    // bounds are >= 0 or NaN: their bits order them; a NaN bound (NaN in Q) is never the largest, and never below a threshold either
    unsigned long long top = 0;
    if (tile < ntiles) {
        const double s = sum_in_order<BOUNDS_SLICES_IN_FLIGHT>(nsl, [=](int i) { // in slice order
            return __longlong_as_double((long long)__hip_atomic_load(pp + i * tp + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        });
        // under the floor the float32 squares may have underflowed (asx_internal.h): no bound, the tile is transformed
        const float b = s < floor ? INFINITY : __double2float_ru(sqrt(scale * s) * (1.0 + (double)ASX_PRUNE_DELTA));
        ub[pair * ntiles + tile] = b;
        top = b == b ? ((unsigned long long)__float_as_uint(b) << 32) | (0xFFFFFFFFu - (unsigned)tile) : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(top >> 32), off, 64), lo = __shfl_xor((unsigned)top, off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0) tops[threadIdx.x >> 6] = top;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < (int)blockDim.x / 64; w++) top = tops[w] > top ? tops[w] : top;
    best[pair] = top ? (int)(0xFFFFFFFFu - (unsigned)top) : 0; // (ties: the smallest tile; every bound NaN: tile 0)
}

// grid (npairs), 256 threads, behind the first launch: skip[pair][tile] = 1 for the tiles the second launch leaves out -- the two the
// first launch took, and every tile whose bound lies under the window of the pair's running maximum: |r^| <= ub < key(max so far) - b2
// <= final maximum - b2, the exit k_inv_cols_r takes behind its scan, taken before the tile is loaded.  An empty running maximum
// (a silent pair: the blocks left at the zero bound) and a NaN bound make the comparison false: nothing but the two is skipped.
__global__ __launch_bounds__(256) void k_prune_select(const float *__restrict__ ub, const int *__restrict__ best,
                                                       unsigned char *__restrict__ skip, AsxPeakWs W, int ntiles,
                                                       unsigned long long *__restrict__ stats, const unsigned long long *__restrict__ list,
                                                       unsigned char *__restrict__ redo, uint32_t pair_base)
{
    __shared__ unsigned kept, short_of;
    const size_t pair = blockIdx.x;
    if (threadIdx.x == 0) { kept = 0; short_of = 0; }
    __syncthreads();
    const asx_peak_t pm = W.pairmax[pair];
    const float thr = near_max_threshold(peak_key(pm), W.bound2[pair]); // NaN when pm == 0
    const int bt = best[pair];
    const unsigned long long w = list ? list[pair] : ASX_Q_ALL;
    unsigned n = 0, miss = asx_q_stored(w, bt) ? 0u : 1u;
    for (int t = threadIdx.x; t < ntiles; t += 256) {
        const bool sk = t == bt || t == 0 || (pm != 0 && ub[pair * ntiles + t] < thr);
        skip[pair * ntiles + t] = sk ? 1 : 0;
        n += sk ? 0u : 1u;
        miss |= (!sk && !asx_q_stored(w, t)) ? 1u : 0u;
    }
    if (n) atomicAdd(&kept, n);
    if (miss) atomicOr(&short_of, 1u);
    __syncthreads();
    // Partial storing: the exact check of the prediction.  The pair is complete when the largest-bound tile and every tile left to
    // the second launch are stored (tile 0 always is).  Otherwise nothing of this pass may stand: every tile is skipped, and the
    // running maximum and the candidate count are emptied, so that the tail treats the pair as a silent one -- it can neither list
    // nor mark it -- and the pair goes on the overflow list with ASX_QSTORE_REDO, counted for the host as k_finalize counts an
    // overflowed pair (but not in W.overflows: the pair has not overflowed).  redo is written for every pair of such a group.
    const bool again = short_of != 0; // block-uniform
    if (again)
        for (int t = threadIdx.x; t < ntiles; t += 256) skip[pair * ntiles + t] = 1;
    if (threadIdx.x == 0) {
        const unsigned first = 1u + ((bt != 0 && asx_q_stored(w, bt)) ? 1u : 0u);
        atomicAdd(&stats[0], (unsigned long long)((again ? 0u : kept) + first));
        atomicAdd(&stats[1], (unsigned long long)ntiles);
        if (list) redo[pair] = again ? 1 : 0;
        if (again) {
            W.pairmax[pair] = 0;
            W.cand_n[pair] = 0;
            if (W.over_list) {
                const uint32_t slot = atomicAdd(W.over_n, 1u);
                if (slot < W.over_cap) W.over_list[slot] = (pair_base + (uint32_t)pair) | ASX_QSTORE_REDO;
                if (W.over_host) (void)__hip_atomic_fetch_add(W.over_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Partial storing, the prediction.  grid (npairs), 256 threads, a tile per thread (ntiles <= 256), behind launch A of the row pass:
// p[t] = the float64 sum of eng[k1][t] over the predictor rows in increasing k1; list[pair] = tile 0 plus the up-to-three tiles
// t != 0 of largest p[t] that exceed c medians of p (ties: the smaller tile; the median: the element of rank ntiles / 2), or
// ASX_Q_ALL when no tile, tile 0 included, does -- unrelated tracks, where every tile will be needed.  A NaN makes every comparison false: ASX_Q_ALL.
// Only the time depends on what this writes (k_prune_select).
__global__ __launch_bounds__(256) void k_q_predict(const float *__restrict__ eng, int nrows, int ntiles, int row_a, int r0, double c,
                                                    unsigned long long *__restrict__ list, unsigned long long *__restrict__ qstats)
{
    __shared__ double p[256];
    __shared__ double med;
    __shared__ unsigned pick[3];
    const size_t pair = blockIdx.x;
    const int t = threadIdx.x;
    double mine = 0.0;
    if (t < ntiles) {
        const float *e = eng + (pair * (size_t)nrows + (size_t)row_a) * ntiles + t;
        for (int i = 0; i < r0; i++) mine += (double)e[(size_t)i * ntiles];
        p[t] = mine;
    }
    if (t == 0) med = (double)NAN;
    if (t < 3) pick[t] = 0xFFFFu;
    __syncthreads();
    int below = 0, above = 0; // tiles in front of this one in ascending order; tiles t' != 0 in front of it in descending order
    if (t < ntiles)
        for (int o = 0; o < ntiles; o++) {
            const double v = p[o];
            below += (v < mine || (v == mine && o < t)) ? 1 : 0;
            above += (o != 0 && (v > mine || (v == mine && o < t))) ? 1 : 0;
        }
    if (t < ntiles && below == ntiles / 2) med = mine;
    __syncthreads();
    if (t > 0 && t < ntiles && above < 3 && mine > c * med) pick[above] = (unsigned)t;
    __syncthreads();
    if (t != 0) return;
    // (the picks are the largest: a pick at place 1 or 2 implies the places in front of it)
    // (tile 0 standing out alone -- a peak at a lag that is a small multiple of M2 away from 0 -- is a list of tile 0)
    unsigned long long w = ASX_Q_ALL;
    unsigned stored = (unsigned)ntiles;
    if (pick[0] != 0xFFFFu || mine > c * med) {
        w = 0ull | ((unsigned long long)pick[0] << 16) | ((unsigned long long)pick[1] << 32) | ((unsigned long long)pick[2] << 48);
        stored = 1u + (pick[0] != 0xFFFFu ? 1u : 0u) + (pick[1] != 0xFFFFu ? 1u : 0u) + (pick[2] != 0xFFFFu ? 1u : 0u);
    }
    list[pair] = w;
    atomicAdd(&qstats[w == ASX_Q_ALL ? 1 : 0], 1ull);
    atomicAdd(&qstats[3], (unsigned long long)stored);
}

// Partial storing, behind the Pearson kernels of the group: the spectral form has counted the mode of every pair's pass
// (k_pearson_final_spec: hdr[3]); a discarded pass (redo) is taken back, the pair's second run counts its own.
__global__ __launch_bounds__(256) void k_qstore_takeback(const unsigned char *__restrict__ redo, const double *__restrict__ hdr,
                                                          unsigned long long *__restrict__ mode_count, int npairs)
{
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= npairs || !redo[pair]) return;
    const int mode = (int)hdr[(size_t)pair * ASX_SPEC_HDR + 3];
    if (mode >= 0 && mode < ASX_PM_NMODES) atomicAdd(&mode_count[mode], ~0ull); // minus one
}

// ---------------------------------------------------------------------------
// k_phat_finalize: grid (npairs / 256), a thread per pair.  The tail of a PHAT group behind k_inv_cols_r: the float32 running maximum IS
// the answer -- the reference's rule (src/cross_correlation.c:52-67: the seed signed, then fabs and a strict '>') applied to the
// float32 values of r_phat, the smallest index among equal ones, which is what pairmax encodes.  No candidate is read, no pair is
// listed, counted or marked: seg (flags 0; the seed when nothing was seen -- a silent track -- found as k_finalize finds it),
// refine_n = 0, and peak = |r_phat[lag]| / F.  A pair whose row is not a window gets a NaN peak (k_invalid_rows writes the rest).
// ---------------------------------------------------------------------------
template <class Sel>
__global__ __launch_bounds__(256) void k_phat_finalize(AsxPeakWs W, AsxSeg *__restrict__ seg, double *__restrict__ peak, uint32_t N,
                                                        double f, int npairs, Sel sel)
{
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= npairs) return;
    const asx_peak_t best = W.pairmax[pair];
    seg[pair] = make_seg(best ? peak_index(best) : sel.seed_of((size_t)pair, N), N);
    W.refine_n[pair] = 0u;
    if (!peak) return;
    // the key is |r| everywhere but at the seed, which competes signed; an empty maximum (a silent track) stands for r = 0; a NaN seed
    // was packed as -infinity (peak_pack_key)
    const float key = best ? peak_key(best) : 0.f;
    double v = key == -INFINITY ? (double)NAN : fabs((double)key) / f;
    if constexpr (std::is_same<Sel, AsxWinRows>::value) {
        AsxWin z;
        if (!asx_win_row(sel, (size_t)pair, N, z)) v = (double)NAN;
    }
    peak[pair] = v;
}

// Its AsxSelTopkSeed form, under a name of its own as k_pearson_prep_x has one (the two k_phat_finalize instances stay the kernels they
// were): the tail of passes 2..k of a PHAT top-k group (asx_xcorr_phat_topk_f32_dev), whose seed is the pair's record's.  It writes no
// peak: k_topk_peak forms each entry's height from pairmax, which this kernel leaves as it found it.
__global__ __launch_bounds__(256) void k_phat_finalize_x(AsxPeakWs W, AsxSeg *__restrict__ seg, uint32_t N, int npairs, AsxSelTopkSeed sel)
{
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= npairs) return;
    const asx_peak_t best = W.pairmax[pair];
    seg[pair] = make_seg(best ? peak_index(best) : sel.seed_of((size_t)pair, N), N);
    W.refine_n[pair] = 0u;
}

// ---------------------------------------------------------------------------
// k_phat_near: grid (npairs), a block per pair.  Behind k_phat_finalize in the tail of a PHAT group whose call asked for it
// (asx_xcorr_phat_sub_f32_dev): r_phat at the 2h + 1 indices around the pair's settled peak p = seg[pair].peak, straight from the
// group's float32 Q', which is whole (a PHAT group is never pruned) -- rows u = 0 .. M1 at q + pair * pair_pitch + u * M2, columns in
// natural order, as k_rows_rp wrote and k_inv_cols_r read them.  One lag idx = j1 * M2 + j2 is a sum down ONE column:
//     r[idx] = Re Q[0][j2] + (-1)^j1 Re Q[M1][j2] + 2 sum_{0 < u < M1} Re( Q[u][j2] exp(+i pi u j1 / M1) )
// (the c2r column step of k_inv_cols_r written out), and the neighbours in INDEX space, circularly over F = 2N, are the neighbouring
// columns of the same rows; a step across a row end moves j1 by one (2 M1 - 1 -> 0 at index F - 1 -> 0).  2h + 1 <= M2 (the launcher's
// callers check it), so the indices hold at most two values of j1 and a thread needs at most two twiddles per row, each from the
// reduced integer (u * j1) mod 2 M1: sincospi of that over M1 is good to the last bits whatever M1 is.  Threads stride over the rows
// and accumulate in float64; the block's sum is a fixed tree (lanes, then waves), so a pair's values do not depend on the batch.
//   near[pair * (2h + 1) + e] = r[(p - h + e) mod F] / v, signed (near may be null); frac[pair] = the vertex of the parabola through
// the three centre values, in float64 in the order the header states.  The window plays no part.  A pair whose row is not a window
// (rows) or whose indices lie outside their pools (pl) gets NaN in all of them.  The kernel only reads what the group left.
// ---------------------------------------------------------------------------
#define ASX_NEAR_N (2 * ASX_NEAR_MAX + 1)
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__global__ __launch_bounds__(256) void k_phat_near(const float2 *__restrict__ q, size_t pair_pitch, const AsxSeg *__restrict__ seg,
                                                    uint32_t N, int M1, int M2, double v, int h, const int64_t *__restrict__ rows,
                                                    size_t rows_step, const AsxPoolPair *__restrict__ pl, double *__restrict__ frac,
                                                    double *__restrict__ near)
{
    const size_t pair = blockIdx.x;
    const int tid = threadIdx.x, n = 2 * h + 1;
    __shared__ double red[4][ASX_NEAR_N];
    __shared__ double y[ASX_NEAR_N];
    bool valid = true;
    if (rows) {
        AsxWin z;
        valid = asx_win_row(AsxWinRows{ rows, rows_step }, pair, N, z);
    }
    if (pl && (pl[pair].flags & ASX_POOL_INVALID)) valid = false;
    if (!valid) { // (block-uniform: nobody is left at a barrier)
        if (near && tid < n) near[pair * (size_t)n + tid] = (double)NAN;
        if (tid == 0) frac[pair] = (double)NAN;
        return;
    }
    const uint32_t F = 2u * N;
    const uint32_t first = (seg[pair].peak % F + F - (uint32_t)h) % F; // index of entry 0
    const uint32_t j1a = first / (uint32_t)M2, j2a = first - j1a * (uint32_t)M2;
    const uint32_t j1b = j1a + 1u == 2u * (uint32_t)M1 ? 0u : j1a + 1u;  // behind the row end
    const bool two = j2a + (uint32_t)n > (uint32_t)M2;
    const float2 *in = q + RWS_PAIR(pair) * pair_pitch;
    double acc[ASX_NEAR_N];
#pragma unroll
    for (int e = 0; e < ASX_NEAR_N; e++) acc[e] = 0.0;
    for (int u = tid; u <= M1; u += 256) {
        // the weights of Re Q and Im Q of row u at j1a and at j1b
        double ca = 1.0, sa = 0.0, cb = 1.0, sb = 0.0;
        if (u == M1) {
            ca = (j1a & 1u) ? -1.0 : 1.0;
            cb = (j1b & 1u) ? -1.0 : 1.0;
        } else if (u != 0) {
            sincospi((double)(((uint32_t)u * j1a) % (2u * (uint32_t)M1)) / (double)M1, &sa, &ca);
            ca *= 2.0; sa *= 2.0;
            if (two) {
                sincospi((double)(((uint32_t)u * j1b) % (2u * (uint32_t)M1)) / (double)M1, &sb, &cb);
                cb *= 2.0; sb *= 2.0;
            }
        }
        const float2 *row = in + (size_t)u * (size_t)M2;
#pragma unroll
        for (int e = 0; e < ASX_NEAR_N; e++) {
            if (e < n) {
                const uint32_t c = j2a + (uint32_t)e;
                const bool wrapped = c >= (uint32_t)M2;
                const float2 x = row[wrapped ? c - (uint32_t)M2 : c];
                acc[e] += (wrapped ? cb : ca) * (double)x.x - (wrapped ? sb : sa) * (double)x.y;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < ASX_NEAR_N; e++) {
        if (e < n) {
            const double s = wave_sum_f64(acc[e]);
            if ((tid & 63) == 0) red[tid >> 6][e] = s;
        }
    }
    __syncthreads();
    if (tid < n) {
        const double r = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / v;
        y[tid] = r;
        if (near) near[pair * (size_t)n + tid] = r;
    }
    __syncthreads();
    if (tid == 0) frac[pair] = asx_parabola_frac(y[h - 1], y[h], y[h + 1]);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// one flavour of k_rows_r, with the flavour's extra argument (none: k_rows_r itself)
template <class K, class... X>
static void launch_rows_r(K kernel, const AsxDev &P, int nt, const AsxSpectra &C, float2 *q, const AsxPeakWs &W, int npairs,
                          hipStream_t s, X... extra)
{
    const int nrows = P.M1 + 1;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nrows * (unsigned)npairs), dim3(nt), (size_t)P.M2 * sizeof(float4), s, rargs_of(P),
                       (const float2 *)C.cx, (const float2 *)C.cy, q, nrows, (size_t)nrows * (size_t)P.M2, W, extra...);
}

// The row pass of a group whose spectra are C, in the flavour its form names (asx_group_form; never ASX_ROWS_PACKED here): k_rows_re
// (plus the tile energies U->eng) for the pruned pass, k_rows_rl (C_x / C_y at the pairs' bank slots) in a pool group, else k_rows_r in
// the broadcast form C.bc -- or, weighted, k_rows_rp in that form, or k_rows_rb with fband when only a band votes, and in a pool group
// their listed forms, k_rows_rlp and k_rows_rlb.  The operands that are not broadcast and q have the group workspace's pair pitch.
void asx_launch_rows_r(const AsxDev &P, const AsxSpectra &C, AsxRowFlavour rows, AsxWeight weight, const AsxBand &fband, const AsxPrune *U,
                       float2 *q, const AsxPeakWs &W, int npairs, hipStream_t s)
{
    asx_with_entry(AsxRRows{}, P.krows, [&](auto e) {
        using S = typename decltype(e)::sched;
        constexpr int NT = e.nt, nt = e.two ? 2 * NT : NT;
        constexpr bool TWO = e.two;
        switch (rows) {
        case ASX_ROWS_ENERGY:
            if (!U->q_rows) launch_rows_r(k_rows_re<S, NT, TWO>, P, nt, C, q, W, npairs, s, U->eng);
            // partial storing (run_group asked asx_qstore_rows): launch A, the predictor rows, stores everything and leaves their
            // energies; k_q_predict states each pair's list; launch B, the other rows, stores the listed tiles
            else if constexpr (TWO) {
                const int nrows = P.M1 + 1, r0 = U->q_rows, a = U->q_row_a;
                auto part = [&](AsxRowRun run, const unsigned long long *list) {
                    hipLaunchKernelGGL((k_rows_rm<S, NT, TWO>), dim3((unsigned)run.count * (unsigned)npairs), dim3(nt),
                                       (size_t)P.M2 * sizeof(float4), s, rargs_of(P), (const float2 *)C.cx, (const float2 *)C.cy, q, nrows,
                                       (size_t)nrows * (size_t)P.M2, W, U->eng, run, list);
                };
                part(AsxRowRun{ 0, r0, a }, nullptr);
                hipLaunchKernelGGL(k_q_predict, dim3(npairs), dim3(256), 0, s, U->eng, nrows, P.ntiles, a, r0, (double)ASX_QSTORE_C, U->list,
                                   U->qstats);
                part(AsxRowRun{ a, nrows - r0, r0 }, U->list);
            }
            break;
        case ASX_ROWS_LISTED:
            if (weight == ASX_W_PHAT_BAND) launch_rows_r(k_rows_rlb<S, NT, TWO>, P, nt, C, q, W, npairs, s, C.pl, fband);
            else if (weight == ASX_W_PHAT) launch_rows_r(k_rows_rlp<S, NT, TWO>, P, nt, C, q, W, npairs, s, C.pl);
            else launch_rows_r(k_rows_rl<S, NT, TWO>, P, nt, C, q, W, npairs, s, C.pl);
            break;
        default:
            if (weight == ASX_W_PHAT_BAND)
                switch (C.bc) {
                case 0: launch_rows_r(k_rows_rb<S, NT, TWO, 0>, P, nt, C, q, W, npairs, s, fband); break;
                case 1: launch_rows_r(k_rows_rb<S, NT, TWO, 1>, P, nt, C, q, W, npairs, s, fband); break;
                case 2: launch_rows_r(k_rows_rb<S, NT, TWO, 2>, P, nt, C, q, W, npairs, s, fband); break;
                default: launch_rows_r(k_rows_rb<S, NT, TWO, 3>, P, nt, C, q, W, npairs, s, fband); break;
                }
            else if (weight == ASX_W_PHAT)
                switch (C.bc) {
                case 0: launch_rows_r(k_rows_rp<S, NT, TWO, 0>, P, nt, C, q, W, npairs, s); break;
                case 1: launch_rows_r(k_rows_rp<S, NT, TWO, 1>, P, nt, C, q, W, npairs, s); break;
                case 2: launch_rows_r(k_rows_rp<S, NT, TWO, 2>, P, nt, C, q, W, npairs, s); break;
                default: launch_rows_r(k_rows_rp<S, NT, TWO, 3>, P, nt, C, q, W, npairs, s); break;
                }
            else
                switch (C.bc) {
                case 0: launch_rows_r(k_rows_r<S, NT, TWO, 0>, P, nt, C, q, W, npairs, s); break;
                case 1: launch_rows_r(k_rows_r<S, NT, TWO, 1>, P, nt, C, q, W, npairs, s); break;
                case 2: launch_rows_r(k_rows_r<S, NT, TWO, 2>, P, nt, C, q, W, npairs, s); break;
                default: launch_rows_r(k_rows_r<S, NT, TWO, 3>, P, nt, C, q, W, npairs, s); break;
                }
        }
    });
}

void asx_launch_phat_finalize(const AsxDev &P, const AsxPeakWs &W, AsxSeg *seg, double *peak, double f, int npairs, hipStream_t s,
                              const AsxSearch &q)
{
    asx_with_selection(q, [&](auto sel) {
        const dim3 grid((unsigned)(npairs + 255) / 256), block(256);
        if constexpr (std::is_same<decltype(sel), AsxSelTopkSeed>::value) // (a top-k pass: the step's k_topk_peak writes the peak)
            hipLaunchKernelGGL(k_phat_finalize_x, grid, block, 0, s, W, seg, P.N, npairs, sel);
        else
            hipLaunchKernelGGL(k_phat_finalize<decltype(sel)>, grid, block, 0, s, W, seg, peak, P.N, f, npairs, sel);
    });
}

void asx_launch_phat_near(const AsxDev &P, const float2 *q, const AsxSeg *seg, double f, int h, const AsxSearch &find,
                          const AsxPoolPair *pl, double *frac, double *near, int npairs, hipStream_t s)
{
    const bool rows = find.kind == AsxSearch::ROWS;
    hipLaunchKernelGGL(k_phat_near, dim3((unsigned)npairs), dim3(256), 0, s, q, asx_spectrum_len(P), seg, P.N, P.M1, P.M2, f, h,
                       rows ? find.rows.rows : nullptr, rows ? find.rows.step : (size_t)0, pl, frac, near);
}

// Blocks of `fn` the current device holds at once (k_inv_cols_r's first generation, the one its stagger delays half of): occupancy
// x CUs, asked once per kernel and device.  ADVICE r5: the kernel used to hard-code 512 / 1024 = this part's 256 CUs.
static unsigned resident_blocks(const void *fn, int nthreads, size_t lds)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, unsigned> known;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find({ fn, dev });
    if (it != known.end()) return it->second;
    int per_cu = 0, cus = 0;
    unsigned n = 512;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, nthreads, lds) == hipSuccess && per_cu > 0 && cus > 0)
        n = (unsigned)per_cu * (unsigned)cus;
    known[{ fn, dev }] = n;
    return n;
}

// Partial storing: the predictor rows R0 of a pruned group of npairs pairs, 0 = the group keeps k_rows_re.  The plan's row schedule
// must have a k_rows_rm instance (the two-half form) and at most 256 tiles (k_q_predict).  R0 = the kernel's resident blocks / npairs,
// clamped to [8, 32], so that launch A is about one generation of blocks: rows that had to be computed anyway, and enough of them that
// the tile sums of unrelated tracks stay under ASX_QSTORE_C medians.  mode 1 (auto): only a group of at least ASX_QSTORE_MIN_GENS
// generations of blocks -- the split costs the row pass about one generation's tail and two launches, which has to be small against
// what a third less store traffic returns (about 8 % of the pass: measured, EXPERIMENTS.md); single pairs and small groups launch
// exactly what they launched before.  mode 2: any group, R0 = 8 (tests).
constexpr int ASX_QSTORE_MIN_GENS = 8;
int asx_qstore_rows(const AsxDev &P, int npairs, int mode)
{
    int r0 = 0;
    if (mode <= 0 || npairs <= 0 || P.ntiles > 256 || P.M1 + 1 < 64) return 0;
    asx_with_entry(AsxRRows{}, P.krows, [&](auto e) {
        using S = typename decltype(e)::sched;
        constexpr int NT = e.nt;
        if constexpr (e.two) {
            if (mode >= 2) { r0 = 8; return; }
            const unsigned res = resident_blocks((const void *)k_rows_rm<S, NT, true>, 2 * NT, (size_t)P.M2 * sizeof(float4));
            if ((size_t)(P.M1 + 1) * (size_t)npairs < (size_t)ASX_QSTORE_MIN_GENS * res) return;
            r0 = std::min(32, std::max(8, (int)(res / (unsigned)npairs)));
        }
    });
    return r0;
}

void asx_launch_qstore_takeback(const AsxPrune &U, const AsxSpecWs &S, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_qstore_takeback, dim3((unsigned)(npairs + 255) / 256), dim3(256), 0, s, U.redo, S.hdr, S.mode_count, npairs);
}

// Forward columns of tracks first .. first + count - 1 of src and / or smp (null: not that operand), src_stride / smp_stride floats
// apart (0 = one track), into the same tracks of dst: C at pitch (M1 + 1) M2, norm partials and band sums in the AsxPeakWs layouts.
// temporal: C stored with ordinary stores (the broadcast slot, the bank).  The kernel reads and writes only the operands it is
// launched for (op0 + blockIdx.y), so an absent operand's pointers are never used.
void asx_launch_fwd_cols_r(const AsxDev &P, const float *src, size_t src_stride, const float *smp, size_t smp_stride, size_t first,
                           int count, const AsxSpectra &dst, bool temporal, hipStream_t s)
{
    const unsigned op0 = src ? 0 : 1, nops = (src ? 1 : 0) + (smp ? 1 : 0);
    if (nops == 0) return;
    const size_t pitch = asx_spectrum_len(P), lds = (size_t)P.M1 * P.T * sizeof(float2);
    const size_t per = 2 * (size_t)P.ntiles; // norm partials per track slot; band sums: nbands times as many
    if (src) src += first * src_stride;
    if (smp) smp += first * smp_stride;
    float2 *cx = dst.cx + first * pitch, *cy = dst.cy + first * pitch;
    float2 *band = dst.band ? dst.band + first * per * (size_t)P.nbands : nullptr;
    float *nrm = dst.nrm + first * per;
    const dim3 grid(rcol_grid_x(P.ntiles, P.logT), nops, count);
    auto launch = [&](auto kernel, int nt) {
        allow_big_lds((const void *)kernel, lds);
        hipLaunchKernelGGL(kernel, grid, dim3(nt), lds, s, rargs_of(P), src, smp, src_stride, smp_stride, cx, cy, nrm, pitch, band, op0);
    };
    asx_with_entry(AsxRCols{}, P.kcols, [&](auto e) {
        using S = typename decltype(e)::sched;
        if (temporal) launch(k_fwd_cols_r<S, e.t, e.nt, false>, e.nt);
        else launch(k_fwd_cols_r<S, e.t, e.nt, true>, e.nt);
    });
}

void asx_launch_pool_resolve(const AsxDev &P, const AsxPoolArgs &A, AsxPoolPair *out, float *nrm, float2 *band, int npairs,
                             hipStream_t s)
{
    const int per = std::max(P.ntiles, band ? P.ntiles * P.nbands : 0);
    hipLaunchKernelGGL(k_pool_resolve, dim3((unsigned)(per + 255) / 256, (unsigned)npairs), dim3(256), 0, s, A, out, nrm, band, P.ntiles,
                       P.nbands);
}

void asx_launch_bcast_aux(const AsxDev &P, const float *snrm, const float2 *sband, float *nrm, float2 *band, int npairs,
                          unsigned which, hipStream_t s)
{
    const int per = std::max(P.ntiles, band ? P.ntiles * P.nbands : 0);
    hipLaunchKernelGGL(k_bcast_aux, dim3((unsigned)(per + 255) / 256, (unsigned)npairs), dim3(256), 0, s, snrm, sband, nrm, band,
                       P.ntiles, P.nbands, which);
}

// one instance of k_inv_cols_r with its selection
template <class K, class Sel>
static void launch_inv_r(K kernel, const AsxDev &P, dim3 grid, int nt, size_t lds, hipStream_t s, const float2 *q, const AsxPeakWs &W,
                         float *r_out, Sel sel)
{
    const void *fn = (const void *)kernel;
    allow_big_lds(fn, lds);
    hipLaunchKernelGGL(kernel, grid, dim3(nt), lds, s, rargs_of(P), q, asx_spectrum_len(P), W, r_out,
                       resident_blocks(fn, nt, lds), sel);
}

// The pruned inverse pass over the Q and the tile energies k_rows_re left: bounds, the two likely tiles, the flags, the rest.
template <class S1, int TC, int NT>
static void launch_inv_rq(const AsxDev &P, const float2 *q, const AsxPeakWs &W, const AsxPrune &U, int npairs, hipStream_t s)
{
    const size_t pitch = asx_spectrum_len(P), lds = (size_t)S1::n * TC * sizeof(float2);
    auto k1 = k_inv_cols_r<S1, TC, NT, AsxSelPrune<true>>;
    auto k2 = k_inv_cols_r<S1, TC, NT, AsxSelPrune<false>>;
    allow_big_lds((const void *)k1, lds);
    allow_big_lds((const void *)k2, lds);
    const int tp = (P.ntiles + 31) & ~31; // AsxKernelChoice::prunable: at most 1024
    hipLaunchKernelGGL(k_tile_bounds, dim3(npairs, 1024 / tp), dim3((tp + 63) & ~63), 0, s, U.eng, U.ub, U.best, U.part, U.ticket, P.M1 + 1, P.ntiles,
                       4.0 * (double)P.M1, ASX_PRUNE_FLOOR_PER_TERM * (double)ASX_PRUNE_T * (double)(P.M1 + 1));
    hipLaunchKernelGGL(k1, dim3(npairs, 2), dim3(NT), lds, s, rargs_of(P), q, pitch, W, resident_blocks((const void *)k1, NT, lds),
                       AsxSelPrune<true>{ U.best, U.skip, U.list });
    hipLaunchKernelGGL(k_prune_select, dim3(npairs), dim3(256), 0, s, U.ub, U.best, U.skip, W, P.ntiles, U.stats, U.list, U.redo, U.pair_base);
    hipLaunchKernelGGL(k2, dim3(npairs, rcol_grid_x(P.ntiles, asx_ilog2(TC))), dim3(NT), lds, s, rargs_of(P), q, pitch, W,
                       resident_blocks((const void *)k2, NT, lds), AsxSelPrune<false>{ U.best, U.skip, U.list });
}

// The inverse column pass of a group: U null, the flavour the search asks for; U the AsxPrune of a pruned group (every lag competes,
// no r_out, and the row pass has left U->eng), the pruned pass.
void asx_launch_inv_cols_r(const AsxDev &P, const float2 *q, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                           const AsxSearch &search, const AsxPrune *U)
{
    asx_with_entry(AsxRCols{}, P.kcols, [&](auto e) {
        using S = typename decltype(e)::sched;
        constexpr int T = e.t, NT = e.nt;
        const size_t lds = (size_t)S::n * T * sizeof(float2);
        const dim3 grid(npairs, rcol_grid_x(P.M2 / T, asx_ilog2(T)));
        if (U)
            launch_inv_rq<S, T, NT>(P, q, W, *U, npairs, s);
        else
            asx_with_selection<1, 3, ASX_TOPK_MAX - 1>(search, [&](auto sel) {
                launch_inv_r(k_inv_cols_r<S, T, NT, decltype(sel), float>, P, grid, NT, lds, s, q, W, r_out, sel);
            });
    });
}
