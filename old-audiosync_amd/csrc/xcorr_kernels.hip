// csrc/xcorr_kernels.hip — the gfx950 kernels of the cross-correlation path.
//
// Pipeline for one pair (reference: src/cross_correlation.c:133-307):
//
//   k_fwd_cols   packs source / zero-padded sample as complex (z[j] = x[2j] + i x[2j+1]),
//                column transforms of length M1 in LDS, four-step twiddle      (:159-166, :34-39)
//   k_rows       row transforms of length M2 of BOTH spectra, real-FFT untangling,
//                X * conj(Y), inverse real-FFT tangling, inverse row transforms,
//                inverse four-step twiddle -- all inside LDS                    (:232-233, :237-239)
//   k_inv_cols   inverse column transforms, |.|-argmax with the reference's exact
//                tie/sign/NaN rules, r never written to HBM                     (:52-67, :242)
//   k_finalize   per-pair reduction of the tile partials, lag wrap, segments   (:256-271)
//   k_pearson_*  five float64 sums over the compared segments, coefficient,
//                NaN gate                                                       (:74-116, :272-276)
//
// The transforms are memory-bound (about 6 flop/byte); nothing here uses MFMA.
#include "asx_internal.h"
#include "lds_fft.h"
#include "xcorr_dev.h"
#include "kernel_table.h"
#include "closure_dev.h"

#include <algorithm>
#include <math.h>
#include <type_traits>
#include <stdlib.h>

// The file is compiled in parts so that a build uses all the cores (Makefile: one object per part):
//   -DASX_PART=<bit mask>; no ASX_PART = everything in one translation unit.
//   1 k_fwd_cols, compile-time schedules    2 k_fwd_cols, run-time schedules
//   4 k_rows, compile-time schedules        8 k_rows, run-time schedules
//   16 k_inv_cols, compile-time schedules   32 k_inv_cols, run-time schedules
//   64 everything else (peak finalisation, refinement, Pearson, helpers, the launch dispatchers)
#ifndef ASX_PART
#define ASX_PART 127
#endif
#define ASX_HAS_PART(bit) ((ASX_PART & (bit)) != 0)

// Diagnostic phase clocks (never in a shipped build; -DASX_STAMPS): lane 0 of every k_rows block
// records s_memtime at phase boundaries into a buffer nothing else reads.
#ifdef ASX_STAMPS
#define ASX_STAMP_AT(kernel, block, slot)                                                            \
    do {                                                                                             \
        if (P.stamps && P.stamp_kernel == (kernel) && threadIdx.x == 0)                              \
            P.stamps[(size_t)(block) * 8 + (slot)] = clock64();                                      \
    } while (0)
#else
#define ASX_STAMP_AT(kernel, block, slot) do {} while (0)
#endif
#define ASX_STAMP(slot) ASX_STAMP_AT(0, task, slot)

// ASX_NT bits (non-temporal accesses): 1 row loads of k_rows, 2 its row stores, 4 loads of the Pearson pass,
// 8 tile stores of k_fwd_cols, 16 tile loads of k_inv_cols
#ifndef ASX_NT
#define ASX_NT 4 // Pearson reads its inputs once: non-temporal loads, 0.213 -> 0.201 ms; the row kernel got slower with them
#endif
typedef float asx_f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 asx_ld16(const float2 *p, bool nt)
{
    if (nt) { const asx_f4v v = __builtin_nontemporal_load(reinterpret_cast<const asx_f4v *>(p)); return make_float4(v.x, v.y, v.z, v.w); }
    return *reinterpret_cast<const float4 *>(p);
}
__device__ __forceinline__ void asx_st16(float2 *p, float4 v, bool nt)
{
    if (nt) { asx_f4v w = { v.x, v.y, v.z, v.w }; __builtin_nontemporal_store(w, reinterpret_cast<asx_f4v *>(p)); }
    else *reinterpret_cast<float4 *>(p) = v;
}
#ifndef ASX_ROWS_MIN_WAVES
#define ASX_ROWS_MIN_WAVES 4   // k_rows fits 128 VGPRs (92-119 by variant): four blocks per CU, which is also what its LDS allows
#endif

extern __shared__ __attribute__((aligned(16))) float2 asx_lds[];

// ---------------------------------------------------------------------------
// Column tiles.  A tile is T columns (T even, a power of two) of the [M1][M2] matrix,
// held in LDS as [M1][T/2] float4 slots; a slot is two adjacent columns as they lie in HBM,
// {re0, im0, re1, im1} (lds_fft.h), so one thread transforms two columns with shared
// twiddles and b128 LDS accesses, and tiles move in and out without a shuffle.
// ---------------------------------------------------------------------------
// k_fwd_cols: grid (ntiles, 2, npairs).  blockIdx.y: 0 = source, 1 = sample.
// Packs real samples as complex (z[j] = x[2j] + i x[2j+1]); zero padding and the periodic
// extension of the source (embedded lengths) happen in the loads, never in HBM.
// S1 = void: column schedule, tile width and block size from the plan at run time (any length);
// S1 = Sched<M1, radices...>, TC = tile width, NT = block size: compiled in (production lengths,
// see the launchers).
template <int MAXR, class S1 = void, int TC = 0, int NT = 0>
__global__ __launch_bounds__(ASX_FFT_THREADS_MAX, 4) void k_fwd_cols(const AsxDev *__restrict__ Pp,
                                                                      const float *__restrict__ src,
                                                                      const float *__restrict__ smp,
                                                                      float2 *__restrict__ zxa,
                                                                      float2 *__restrict__ zya,
                                                                      float *__restrict__ nrm_part)
{
    const AsxDev &PD = *Pp; // the plan lives in device memory: uniform scalar loads, taken once
    const AsxKP P = asx_kp(PD);
    __shared__ float nrm_red[ASX_FFT_THREADS_MAX / 64];
    const bool is_smp = blockIdx.y != 0;
    const size_t pair = blockIdx.z;
    constexpr bool STATIC = !std::is_void<S1>::value;
    int T = P.T, logT = P.logT, M1 = P.M1;
    int nthreads = blockDim.x;
    if constexpr (STATIC) { T = TC; logT = asx_ilog2(TC); M1 = S1::n; nthreads = NT; }
    const int tile = col_tile_of_block(blockIdx.x, logT);
    if (tile >= P.ntiles) return; // grid.x is rounded up (col_grid_x)
    const int logH = logT - 1, H = T >> 1, M2 = P.M2;
    const int c0 = tile * T;

    const float *in = is_smp ? smp + pair * (size_t)P.N : src + pair * (size_t)P.src_period;
    const uint32_t valid = is_smp ? P.N : P.src_valid;      // real samples that are not zero padding
    const uint32_t period = is_smp ? P.N : P.src_period;    // source may be periodically extended
    float2 *out = (is_smp ? zya : zxa) + pair * (size_t)P.M;
    const bool even = (M2 & 1) == 0;
    const bool vec_in = even && ((reinterpret_cast<uintptr_t>(in) & 15u) == 0);
    float4 *lds4 = reinterpret_cast<float4 *>(asx_lds);

    const int nelem4 = M1 << logH;
    const LdsLayout Lc = col_layout(T, logT, nthreads);
    const size_t stamp_block = (pair * 2 + blockIdx.y) * P.ntiles + tile;
    (void)stamp_block;
    ASX_STAMP_AT(1, stamp_block, 0);
    TwPre pre;
    if constexpr (STATIC) pre = tw_prefetch_first<S1, false, true>(Lc, P.tw1);
    else pre = tw_prefetch<true>(PD.st1, 0, Lc, P.tw1);
    // all of a thread's tile loads are issued before the first is consumed (ASX_COL_LOADS per
    // round): a rolled loop would pay the HBM latency once per iteration
    // Fast path (block-uniform): full tile, 16-byte aligned rows, no periodic extension, and the
    // zero padding starts on a row boundary -> a row is either all data or all zeros.
    const uint32_t row_reals = 2u * (uint32_t)M2;                 // real samples per matrix row
    const bool fast = vec_in && (c0 + T <= M2) && (valid <= period) && (valid % row_reals == 0u);
    const int data_rows = fast ? (int)(valid / row_reals) : 0;     // rows below this are all data
    // sum of squares of everything this block loads: |source|^2 and |sample|^2 (the scale of the
    // float32 error bound of the peak search) come out of the pass that reads the inputs anyway
    float ss = 0.f;
    for (int e0 = threadIdx.x; e0 < nelem4; e0 += ASX_COL_LOADS * nthreads) {
        float4 v[ASX_COL_LOADS];
        if (fast) {
            static_for<0, ASX_COL_LOADS>([&](auto I) __attribute__((always_inline)) {
                const int e = e0 + decltype(I)::value * nthreads;
                const int cg = e & (H - 1), j1 = e >> logH;
                v[I] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j1 < data_rows) // also false for e >= nelem4 (j1 >= M1 >= data_rows)
                    v[I] = *reinterpret_cast<const float4 *>(in + 2 * ((size_t)j1 * M2 + c0 + 2 * cg));
            });
        } else {
        static_for<0, ASX_COL_LOADS>([&](auto I) __attribute__((always_inline)) {
            const int e = e0 + decltype(I)::value * nthreads;
            const int cg = e & (H - 1), j1 = e >> logH;
            const int j2 = c0 + 2 * cg;
            v[I] = make_float4(0.f, 0.f, 0.f, 0.f); // (re0, im0, re1, im1) as it lies in memory
            if (e < nelem4 && j2 < M2) {
                const uint32_t i0 = 2u * ((uint32_t)j1 * (uint32_t)M2 + (uint32_t)j2);
                if (vec_in && i0 + 3u < valid && i0 + 3u < period) {
                    v[I] = *reinterpret_cast<const float4 *>(in + i0);
                } else {
                    float r[4] = { 0.f, 0.f, 0.f, 0.f };
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const uint32_t idx = i0 + h;
                        if (j2 + (h >> 1) < M2 && idx < valid) r[h] = in[idx < period ? idx : idx - period];
                    }
                    v[I] = make_float4(r[0], r[1], r[2], r[3]);
                }
            }
        });
        }
        static_for<0, ASX_COL_LOADS>([&](auto I) __attribute__((always_inline)) {
            const int e = e0 + decltype(I)::value * nthreads;
            if (e < nelem4) {
                lds4[e] = v[I];
                ss = fmaf(v[I].x, v[I].x, fmaf(v[I].y, v[I].y, fmaf(v[I].z, v[I].z, fmaf(v[I].w, v[I].w, ss))));
            }
        });
    }
    ss = wave_sum_f32(ss);
    if ((threadIdx.x & 63) == 0) nrm_red[threadIdx.x >> 6] = ss;
    __syncthreads();
    ASX_STAMP_AT(1, stamp_block, 1);
    // (the first stage fed straight from HBM, as in k_inv_cols, was measured 2 % slower here: this kernel is bound by its
    // HBM access pattern, not by its LDS passes -- DESIGN.md 5.1, tools/experiments/kernel_switches.patch)
    if constexpr (STATIC) lds_fft_static<S1, false, true>(lds4, Lc, P.tw1, pre);
    else lds_fft<MAXR, false, true>(lds4, PD.st1, Lc, P.tw1, pre);
    ASX_STAMP_AT(1, stamp_block, 2);
    if (threadIdx.x == 0) {
        float t = nrm_red[0];
        for (int w = 1; w < (nthreads + 63) >> 6; w++) t += nrm_red[w];
        nrm_part[(pair * 2 + blockIdx.y) * (size_t)P.ntiles + tile] = t;
    }

    // slot p1 holds frequency k1 = k1_of_pos1[p1] and stays in that slot in HBM; the
    // four-step twiddle w_M^(k1*j2) is applied by k_rows, where k1 is block-uniform.
    const bool full = even && (c0 + T <= M2);
    for (int e = threadIdx.x; e < nelem4; e += nthreads) {
        const int cg = e & (H - 1), p1 = e >> logH;
        const int j2 = c0 + 2 * cg;
        if (full) {
            const float4 v = lds4[e];
            asx_st16(out + (size_t)p1 * M2 + j2, v, ASX_NT & 8);
        } else if (j2 < M2) {
            const float4 v = lds4[e];
            float2 *o = out + (size_t)p1 * M2 + j2;
            if (even) {
                *reinterpret_cast<float4 *>(o) = v;
            } else {
                o[0] = make_float2(v.x, v.y);
                if (j2 + 1 < M2) o[1] = make_float2(v.z, v.w);
            }
        }
    }
    ASX_STAMP_AT(1, stamp_block, 3);
}

// ---------------------------------------------------------------------------
// k_rows: grid (M1/2 + 1, npairs).  Block k1 handles spectrum rows k1 and m1 = M1 - k1
// (the rows that hold each other's k <-> M-k partners).  LDS: A[M2], B[M2] float4 slots,
// pairing the two SPECTRA: A[e] = {X[e], Y[e]} of row k1, B of row m1.
// After the spectral combine the same storage holds C[e] = {Ga[e], Gb[e]},
// the two rows of G, which the inverse transforms as one pair.  Self-paired rows
// (k1 = 0, M1/2) use A only and carry zeros in the second member of C.
// ---------------------------------------------------------------------------
// Row loads of one task, all issued before the first is consumed.  (Issuing them one task
// AHEAD in a persistent block was tried: +50 live VGPRs pushed k_rows to 221 registers = two
// waves per SIMD, and the kernel got 1.6x slower; see DESIGN.md "what did not work".)
struct RowRegs {
    float2 xa[ASX_ROW_STEPS], ya[ASX_ROW_STEPS], xb[ASX_ROW_STEPS], yb[ASX_ROW_STEPS];
};
#define ASX_ROW_WSTEPS ((ASX_ROW_STEPS + 1) / 2) // steps of the 16-byte form: two elements per lane and step
struct RowRegsWide {
    float4 xa[ASX_ROW_WSTEPS], ya[ASX_ROW_WSTEPS], xb[ASX_ROW_WSTEPS], yb[ASX_ROW_WSTEPS];
};

// S2 = void: schedule of the row transforms read from the plan at run time (any length);
// S2 = Sched<M2, radices...>: compiled in (the production lengths, see asx_launch_rows).
template <int MAXR, class S2 = void, int NT = 0>
__global__ __launch_bounds__(ASX_FFT_THREADS_MAX, ASX_ROWS_MIN_WAVES) void k_rows(const AsxDev *__restrict__ Pp,
                                                                  const float2 *__restrict__ zxa,
                                                                  const float2 *__restrict__ zya,
                                                                  float2 *__restrict__ ga,
                                                                  const int4 *__restrict__ row_tasks,
                                                                  int M1, int M2_arg, uint32_t M, AsxPeakWs W)
{
    constexpr bool STATIC = !std::is_void<S2>::value;
    int M2 = M2_arg, nthreads = blockDim.x;
    if constexpr (STATIC) { M2 = S2::n; nthreads = NT; }
    // The start of a block is a chain of dependent memory accesses (plan struct -> index table ->
    // rows); M1/M2/M and the task table come as kernel arguments so that ONE 16-byte load
    // (slots and row numbers) separates the block from its row loads.
    const AsxDev &PD = *Pp; // the plan lives in device memory: uniform scalar loads, taken once
    const AsxKP P = asx_kp(PD);
    const int nrows = M1 / 2 + 1;
    float4 *A4 = reinterpret_cast<float4 *>(asx_lds), *B4 = A4 + M2;
    __shared__ float2 tw_step[2][ASX_ROW_STEPS];

    // one task per block.  (Resident blocks that pull tasks from a ticket counter were measured: no gain, block start-up
    // is not what this kernel waits for -- DESIGN.md 5.1, tools/experiments/kernel_switches.patch.)
    const int task = blockIdx.x;
    {
        const int pair = task / nrows;
        const int4 rt = row_tasks[task - pair * nrows];
        const int pa = rt.x, pb = rt.y;
        const int k1 = rt.z, m1 = rt.w;
        const bool self = (k1 == m1);
        ASX_STAMP(0);
        if (k1 == 0 && threadIdx.x < 64) {
            // Row 0 of a pair also prepares the pair's peak search (k_inv_cols runs after this kernel):
            // the float32 error bound from the norms k_fwd_cols left, and the running maximum and the
            // candidate count back to zero.
            const float *np = W.nrm_part + (size_t)pair * 2 * P.ntiles;
            float sx = 0.f, sy = 0.f;
            for (int t = threadIdx.x; t < P.ntiles; t += 64) { sx += np[t]; sy += np[P.ntiles + t]; }
            sx = wave_sum_f32(sx); sy = wave_sum_f32(sy);
            if (threadIdx.x == 0) {
                W.bound2[pair] = PD.bound_scale * sqrtf(sx) * sqrtf(sy);
                W.pairmax[pair] = 0;
                W.cand_n[pair] = 0;
            }
        }
        LdsLayout Lf;
        Lf.ngroups = self ? 1 : 2; Lf.log_ngroups = 0;
        const int tid = threadIdx.x;
        Lf.elem_stride = 1; Lf.group_stride = M2; Lf.nthreads = nthreads; Lf.tid = tid;
        LdsLayout Li;
        Li.ngroups = 1; Li.log_ngroups = 0;
        Li.elem_stride = 1; Li.group_stride = 0; Li.nthreads = nthreads; Li.tid = tid;
        // Every row load of the thread is issued first; the twiddle lookups below overlap them.
        // Rows of even length move as 16 bytes per lane (two complex values): a block's burst of
        // 8-byte loads takes 2-3x as long to come back (tools/micro/rowload_latency.hip: 21 k cycles
        // against 8-12 k for the same four rows).
        const bool wide = (M2 & 1) == 0;
        const int half = M2 >> 1; // wide: a thread owns the element pairs q = t + nthreads*i, j2 = 2q, 2q+1
        RowRegs L;
        RowRegsWide LW;
        {
            const float2 *gx = zxa + (size_t)pair * M, *gy = zya + (size_t)pair * M;
            if (wide) {
                static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                    const int q = tid + decltype(I)::value * nthreads;
                    // (no zero fill of the registers a thread does not load: every use below is under the same
                    //  conditions, and the fill was 100 v_mov per wave, 5 % of the kernel's VALU instructions)
                    if (q < half) {
                        LW.xa[I] = asx_ld16(gx + (size_t)pa * M2 + 2 * q, ASX_NT & 1);
                        LW.ya[I] = asx_ld16(gy + (size_t)pa * M2 + 2 * q, ASX_NT & 1);
                        if (!self) {
                            LW.xb[I] = asx_ld16(gx + (size_t)pb * M2 + 2 * q, ASX_NT & 1);
                            LW.yb[I] = asx_ld16(gy + (size_t)pb * M2 + 2 * q, ASX_NT & 1);
                        }
                    }
                });
            } else {
                static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
                    const int j2 = tid + decltype(I)::value * nthreads;
                    L.xa[I] = L.ya[I] = L.xb[I] = L.yb[I] = make_float2(0.f, 0.f);
                    if (j2 < M2) {
                        L.xa[I] = gx[(size_t)pa * M2 + j2];
                        L.ya[I] = gy[(size_t)pa * M2 + j2];
                        if (!self) {
                            L.xb[I] = gx[(size_t)pb * M2 + j2];
                            L.yb[I] = gy[(size_t)pb * M2 + j2];
                        }
                    }
                });
            }
        }
        TwPre pre_f;
        if constexpr (STATIC) pre_f = tw_prefetch_first<S2, false, false>(Lf, P.tw2);
        else pre_f = tw_prefetch<false>(PD.st2, 0, Lf, P.tw2);

        // Four-step twiddle of row k1: w_M^(k1*j2).  With j2 = c*(t + nthreads*i) + h (c = 2, h = 0/1
        // for the wide form; c = 1, h = 0 otherwise) it factors into w_M^(k1*c*t) (one two-level
        // lookup per thread), w_M^(k1*c*nthreads*i) (a handful per block) and w_M^(k1*h) (block-uniform).
        const int cw = wide ? 2 : 1;
        const int nsteps = wide ? (half + nthreads - 1) / nthreads : (M2 + nthreads - 1) / nthreads; // <= ASX_ROW_STEPS (launcher)
        if (tid < 2 * nsteps) {
            const int which = tid >= nsteps;
            const int i = tid - which * nsteps;
            const uint32_t row = which ? (uint32_t)m1 : (uint32_t)k1;
            tw_step[which][i] = tw_F(P, 2u * row * (uint32_t)(cw * i * nthreads));
        }
        const uint32_t tcol = (uint32_t)cw * tid < (unsigned)M2 ? (uint32_t)cw * tid : 0u;
        const float2 twa = tw_F(P, 2u * (uint32_t)k1 * tcol);
        const float2 twb = tw_F(P, 2u * (uint32_t)m1 * tcol);
        const float2 wk1 = tw_F(P, 2u * (uint32_t)k1), wm1 = tw_F(P, 2u * (uint32_t)m1); // w_M^k1, w_M^m1
        // (The first row stage fed straight from HBM, as in k_inv_cols, made no difference here: 1.18-1.20 ms with and
        // without, +8 VGPRs -- DESIGN.md 5.1, tools/experiments/kernel_switches.patch.)
        {
            __syncthreads();
            if (wide) {
                static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                    constexpr int i = decltype(I)::value;
                    const int q = tid + i * nthreads;
                    if (q < half) {
                        const float2 wa0 = cmul(twa, tw_step[0][i]), wa1 = cmul(wa0, wk1);
                        lds_put(A4 + 2 * q, mulw(Cx2{ v2f{ LW.xa[I].x, LW.ya[I].x }, v2f{ LW.xa[I].y, LW.ya[I].y } }, wa0));
                        lds_put(A4 + 2 * q + 1, mulw(Cx2{ v2f{ LW.xa[I].z, LW.ya[I].z }, v2f{ LW.xa[I].w, LW.ya[I].w } }, wa1));
                        if (!self) {
                            const float2 wb0 = cmul(twb, tw_step[1][i]), wb1 = cmul(wb0, wm1);
                            lds_put(B4 + 2 * q, mulw(Cx2{ v2f{ LW.xb[I].x, LW.yb[I].x }, v2f{ LW.xb[I].y, LW.yb[I].y } }, wb0));
                            lds_put(B4 + 2 * q + 1, mulw(Cx2{ v2f{ LW.xb[I].z, LW.yb[I].z }, v2f{ LW.xb[I].w, LW.yb[I].w } }, wb1));
                        }
                    }
                });
            } else {
                static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
                    constexpr int i = decltype(I)::value;
                    const int j2 = tid + i * nthreads;
                    if (j2 < M2) {
                        lds_put(A4 + j2, mulw(Cx2{ v2f{ L.xa[I].x, L.ya[I].x }, v2f{ L.xa[I].y, L.ya[I].y } },
                                              cmul(twa, tw_step[0][i])));
                        if (!self)
                            lds_put(B4 + j2, mulw(Cx2{ v2f{ L.xb[I].x, L.yb[I].x }, v2f{ L.xb[I].y, L.yb[I].y } },
                                                  cmul(twb, tw_step[1][i])));
                    }
                });
            }
        __syncthreads();
        ASX_STAMP(1);
        if constexpr (STATIC) lds_fft_static<S2, false, false>(A4, Lf, P.tw2, pre_f);
        else lds_fft<MAXR, false, false>(A4, PD.st2, Lf, P.tw2, pre_f);
        }
        ASX_STAMP(2);

        // ---- spectral combine: the same storage then holds C[e] = {Ga[e], Gb[e]}, the two rows of G.
        const float2 wA = wk1; // w_M^k1, block-uniform; w_M^(k1 + M1*k2) = wA * w_M2^k2
        TwPre pre_i;
        if (!self) {
            // The common case.  A thread walks SLOT PAIRS (s, s' = M2-1-s), s = t + i*nthreads < M2/2, not bins:
            // digit reversal complements every digit, so the partner bin M2-1-k2 of the bin at slot s sits at
            // slot s'.  Bin(s) of row k1 pairs with bin(s') of row m1 and bin(s') of row k1 with bin(s) of row
            // m1: the thread reads A[s], B[s'], A[s'], B[s] and writes C[s] = {G_k1[s], G_m1[s]} and C[s'] --
            // nobody else touches these four slots, so there is NO barrier between the reads and the writes,
            // the writes are whole 16-byte slots, consecutive lanes walk consecutive slots (forwards in s,
            // backwards in s'): no bank conflicts, no index table (the twiddle table is kept in slot order).
            // Sweeps: table reads of all steps in flight, then the LDS reads, then the arithmetic.
            const int npairs2 = (M2 + 1) >> 1;
            float2 w2a[ASX_ROW_WSTEPS], w2b[ASX_ROW_WSTEPS];
            int sl[ASX_ROW_WSTEPS];
            static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int sx = tid + i * nthreads;
                sl[i] = sx < npairs2 ? sx : 0; // clamped: the loads are unconditional
                w2a[i] = P.tw2s[sl[i]];
                w2b[i] = P.tw2s[M2 - 1 - sl[i]];
            });
            if constexpr (STATIC) pre_i = tw_prefetch_first<S2, true, false>(Li, P.tw2);
            else pre_i = tw_prefetch<false>(PD.st2, PD.st2.nstages - 1, Li, P.tw2);
            Cx2 za[ASX_ROW_WSTEPS], zb[ASX_ROW_WSTEPS], zc[ASX_ROW_WSTEPS], zd[ASX_ROW_WSTEPS];
            static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                za[i] = lds_get(A4 + sl[i]);
                zb[i] = lds_get(B4 + (M2 - 1 - sl[i]));
                zc[i] = lds_get(A4 + (M2 - 1 - sl[i]));
                zd[i] = lds_get(B4 + sl[i]);
            });
            static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int sx = tid + i * nthreads;
                float2 gk0, gm0, gk1, gm1;
                combine_pair(za[i], zb[i], cmul(wA, w2a[i]), gk0, gm0); // bin(s) of k1 with bin(s') of m1
                combine_pair(zc[i], zd[i], cmul(wA, w2b[i]), gk1, gm1); // bin(s') of k1 with bin(s) of m1
                if (sx < npairs2) {
                    const int sp = M2 - 1 - sx;
                    if (sp != sx) {
                        A4[sx] = make_float4(gk0.x, gk0.y, gm1.x, gm1.y);
                        A4[sp] = make_float4(gk1.x, gk1.y, gm0.x, gm0.y);
                    } else { // odd M2: the middle slot is its own partner
                        A4[sx] = make_float4(gk0.x, gk0.y, gm0.x, gm0.y);
                    }
                }
            });
        } else {
        // Self-paired rows (k1 = 0, M1/2; two blocks per pair): bins pair up inside the row through the
        // index table.  Every thread first computes its G values into registers (it reads slots other
        // threads will overwrite), then, after a barrier, writes them.
        float2 gk[ASX_ROW_STEPS], gm[ASX_ROW_STEPS];
        int sa[ASX_ROW_STEPS], sb[ASX_ROW_STEPS]; // -1: nothing to write
        static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            const int k2 = tid + i * nthreads;
            sa[i] = -1; sb[i] = -1;
            gk[i] = make_float2(0.f, 0.f); gm[i] = make_float2(0.f, 0.f);
            if (k1 == 0) {
                if (k2 == 0) {
                    // DC and Nyquist bins are real: X[0] = Re Z0 + Im Z0, X[M] = Re Z0 - Im Z0
                    const Cx2 z = lds_get(A4);
                    const float P0 = (z.re.x + z.im.x) * (z.re.y + z.im.y);
                    const float PM = (z.re.x - z.im.x) * (z.re.y - z.im.y);
                    sa[i] = 0;
                    gk[i] = make_float2(P0 + PM, P0 - PM);
                } else if (k2 <= M2 / 2) {
                    const int m2 = M2 - k2;
                    sa[i] = P.pos2_of_k2[k2];
                    const int s2 = P.pos2_of_k2[m2];
                    combine_pair(lds_get(A4 + sa[i]), lds_get(A4 + s2), P.tw2[k2], gk[i], gm[i]);
                    if (m2 != k2) sb[i] = s2;
                }
            } else { // k1 == M1/2, M1 even
                if (k2 < (M2 + 1) / 2) {
                    const int m2 = M2 - 1 - k2;
                    sa[i] = P.pos2_of_k2[k2];
                    const int s2 = P.pos2_of_k2[m2];
                    combine_pair(lds_get(A4 + sa[i]), lds_get(A4 + s2), cmul(wA, P.tw2[k2]), gk[i], gm[i]);
                    if (m2 != k2) sb[i] = s2;
                }
            }
        });
        if constexpr (STATIC) pre_i = tw_prefetch_first<S2, true, false>(Li, P.tw2);
        else pre_i = tw_prefetch<false>(PD.st2, PD.st2.nstages - 1, Li, P.tw2);
        __syncthreads();
        static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            if (sa[i] >= 0) A4[sa[i]] = make_float4(gk[i].x, gk[i].y, 0.f, 0.f);
            if (sb[i] >= 0) A4[sb[i]] = make_float4(gm[i].x, gm[i].y, 0.f, 0.f);
        });
        }
        __syncthreads();

        ASX_STAMP(3);
        // inverse row transforms of the G pair, digit-reversed in -> natural j2 out
        if constexpr (STATIC) lds_fft_static<S2, true, false>(A4, Li, P.tw2, pre_i);
        else lds_fft<MAXR, true, false>(A4, PD.st2, Li, P.tw2, pre_i);
        ASX_STAMP(4);

        // inverse four-step twiddle conj(w_M^(k1*j2)) / conj(w_M^(m1*j2)), one per member; unrolled so
        // that the LDS reads of all steps are in flight together (a rolled loop pays the LDS latency
        // once per step).  twa / twb ride in registers from the load phase.  Even rows leave as 16
        // bytes per lane, like they came.
        float2 *go = ga + (size_t)pair * M;
        if (wide) {
            Cx2 g0[ASX_ROW_WSTEPS], g1[ASX_ROW_WSTEPS];
            static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int q = tid + i * nthreads;
                const int qq = q < half ? q : 0;
                g0[i] = lds_get(A4 + 2 * qq);
                g1[i] = lds_get(A4 + 2 * qq + 1);
            });
            static_for<0, ASX_ROW_WSTEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int q = tid + i * nthreads;
                if (q < half) {
                    const float2 wa0 = cmul(twa, tw_step[0][i]), wb0 = cmul(twb, tw_step[1][i]);
                    const float2 wa1 = cmul(wa0, wk1), wb1 = cmul(wb0, wm1);
                    const Cx2 h0 = mul2c(g0[i], Cx2{ v2f{ wa0.x, wb0.x }, v2f{ wa0.y, wb0.y } });
                    const Cx2 h1 = mul2c(g1[i], Cx2{ v2f{ wa1.x, wb1.x }, v2f{ wa1.y, wb1.y } });
                    asx_st16(go + (size_t)pa * M2 + 2 * q, make_float4(h0.re.x, h0.im.x, h1.re.x, h1.im.x), ASX_NT & 2);
                    if (!self)
                        asx_st16(go + (size_t)pb * M2 + 2 * q, make_float4(h0.re.y, h0.im.y, h1.re.y, h1.im.y), ASX_NT & 2);
                }
            });
        } else {
            Cx2 gout[ASX_ROW_STEPS];
            static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int j2 = tid + i * nthreads;
                gout[i] = lds_get(A4 + (j2 < M2 ? j2 : 0));
            });
            static_for<0, ASX_ROW_STEPS>([&](auto I) __attribute__((always_inline)) {
                constexpr int i = decltype(I)::value;
                const int j2 = tid + i * nthreads;
                if (j2 < M2) {
                    const float2 wa = cmul(twa, tw_step[0][i]), wb = cmul(twb, tw_step[1][i]);
                    const Cx2 g = mul2c(gout[i], Cx2{ v2f{ wa.x, wb.x }, v2f{ wa.y, wb.y } });
                    go[(size_t)pa * M2 + j2] = make_float2(g.re.x, g.im.x);
                    if (!self) go[(size_t)pb * M2 + j2] = make_float2(g.re.y, g.im.y);
                }
            });
        }
        ASX_STAMP(5);
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------------------
// k_inv_cols: grid (ntiles, npairs).  Inverse column transforms; the time-domain
// correlation r[2j] = Re g[j], r[2j+1] = Im g[j] only lives in LDS/registers.
// ---------------------------------------------------------------------------
// Sel (asx_internal.h) says which lags compete.  Sel::masks: only the lags of Z = sel.window_of(pair) compete and Z.seed is the one
// whose key is signed (the generalisation of the idx < nout test); the fast scans see out-of-window values as NaN (never a maximum
// there, never a candidate), the general scans skip them; r_out still receives every lag.  One instance per selection, so that the
// full window runs the <AsxSelAll> instance untouched: AsxWin the plan's window (asx_plan_set_lag_window); AsxWinRows the pair's row
// in device memory (asx_xcorr_windowed_f32_dev), read once per block in front of the tile loads (an invalid row holds no lag,
// asx_win_row); AsxSelTopk<ASX_TOPK_MAX - 1> the pass's window, seed and the zones around the pair's earlier entries from its record
// (passes 2..k of asx_xcorr_topk_f32_dev; one zone capacity: the packed kernels are off the hot path).
// The body is written here and nowhere else, and in the __global__ itself: a call boundary changes the instruction stream.
template <int MAXR, class S1, int TC, int NT, class Sel>
__global__ __launch_bounds__(ASX_FFT_THREADS_MAX, 4) void k_inv_cols(const AsxDev *__restrict__ Pp, const float2 *__restrict__ ga,
                                                                   AsxPeakWs W, float *__restrict__ r_out, Sel sel)
{
    constexpr bool WIN = Sel::masks;
    const auto Z = sel.window_of(blockIdx.y, Pp->N);
    const AsxDev &PD = *Pp; // the plan lives in device memory: uniform scalar loads, taken once
    const AsxKP P = asx_kp(PD);
    __shared__ asx_peak_t red[ASX_FFT_THREADS_MAX / 64];
    const size_t pair = blockIdx.y;
    constexpr bool STATIC = !std::is_void<S1>::value;
    int T = P.T, logT = P.logT, M1 = P.M1;
    int nthreads = blockDim.x;
    if constexpr (STATIC) { T = TC; logT = asx_ilog2(TC); M1 = S1::n; nthreads = NT; }
    const int tile = col_tile_of_block(blockIdx.x, logT);
    if (tile >= P.ntiles) return; // grid.x is rounded up (col_grid_x)
    // A digitally silent track (a zero norm, e.g. the zero-filled tail of a short capture): r is exactly zero
    // everywhere, the reference's scan returns index 0 (src/cross_correlation.c:52-67), which is what a running
    // maximum left at zero means to k_finalize.  Without this every one of the 2N lags would be a near-tie of the
    // maximum 0 inside a window of width 0, the lists would overflow and the synchronous entry points would
    // re-evaluate all of them exactly (seconds at N = 1 440 000).  Block-uniform; r_out (tests) still wants zeros.
    if (W.bound2[pair] == 0.f && r_out == nullptr) return;
    const double shift = W.shift ? W.shift[pair] : 0.0; // block-uniform; non-zero only in the second look (second_look, asx_api.hip)
    const int logH = logT - 1, H = T >> 1, M2 = P.M2;
    const int c0 = tile * T;
    const float2 *in = ga + pair * (size_t)P.M;
    const bool even = (M2 & 1) == 0;
    float4 *lds4 = reinterpret_cast<float4 *>(asx_lds);

    const int nelem4 = M1 << logH;
    const LdsLayout Lc = col_layout(T, logT, nthreads);
    const size_t stamp_block = pair * P.ntiles + tile;
    (void)stamp_block;
    ASX_STAMP_AT(2, stamp_block, 0);
    // The pair's running maximum so far (other tiles publish theirs with atomicMax below) and the width
    // of the near-maximum window are consumed after the first pass of the scan, at the very end.  Loaded where
    // they are used, the block waits 2 700 cycles for an L2 round trip there (phase stamps).  Thread 0 fetches
    // them now and parks them in LDS: its wave waits for them together with its tile loads, and everybody reads
    // them behind the barriers of the transform.
    __shared__ asx_peak_t s_run0;
    __shared__ float s_b2;
    if (threadIdx.x == 0) {
        s_run0 = W.pairmax[pair];
        s_b2 = W.bound2[pair];
    }
    TwPre pre;
    if constexpr (STATIC) pre = tw_prefetch_first<S1, true, true, true>(Lc, P.tw1);
    else pre = tw_prefetch<true>(PD.st1, PD.st1.nstages - 1, Lc, P.tw1);
#ifndef ASX_INV_FED
#define ASX_INV_FED 1 // first inverse stage fed straight from HBM (compile-time schedules, full tiles)
#endif
    TwPre pre_last;
    bool filled = false;
    if constexpr (STATIC && ASX_INV_FED) {
        if (even && (c0 + T <= M2)) { // block-uniform: full tile
            // No fill phase: the first stage to run (innermost, 10 consecutive rows per butterfly) takes its
            // inputs from HBM -- the thread's loads are all in flight together, as in the fill loop -- and writes
            // its outputs to LDS: one LDS write + read pass and one barrier less per tile.
            ASX_STAMP_AT(2, stamp_block, 1);
            pre_last = lds_fft_static_head_fed<S1, true, true>(lds4, Lc, P.tw1, pre,
                [&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
                    const float2 *col = in + (size_t)pos0 * M2 + c0 + 2 * g;
                    static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                        constexpr int t = decltype(TT)::value;
                        const float4 x = asx_ld16(col + (size_t)(t * q) * M2, ASX_NT & 16);
                        v[t] = Cx2{ v2f{ x.x, x.z }, v2f{ x.y, x.w } };
                    });
                });
            filled = true;
        }
    }
    if (!filled) {
    for (int e0 = threadIdx.x; e0 < nelem4; e0 += ASX_COL_LOADS * nthreads) {
        float4 v[ASX_COL_LOADS];
        static_for<0, ASX_COL_LOADS>([&](auto I) __attribute__((always_inline)) {
            const int e = e0 + decltype(I)::value * nthreads;
            const int cg = e & (H - 1), p1 = e >> logH;
            const int j2 = c0 + 2 * cg;
            v[I] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (even && (c0 + T <= M2)) { // block-uniform: full tile
                if (e < nelem4) v[I] = *reinterpret_cast<const float4 *>(in + (size_t)p1 * M2 + j2);
            } else if (e < nelem4 && j2 < M2) {
                const float2 *g = in + (size_t)p1 * M2 + j2;
                if (even) {
                    v[I] = *reinterpret_cast<const float4 *>(g);
                } else {
                    const float2 a = g[0];
                    const float2 b = (j2 + 1 < M2) ? g[1] : make_float2(0.f, 0.f);
                    v[I] = make_float4(a.x, a.y, b.x, b.y);
                }
            }
        });
        static_for<0, ASX_COL_LOADS>([&](auto I) __attribute__((always_inline)) {
            const int e = e0 + decltype(I)::value * nthreads;
            if (e < nelem4) lds4[e] = v[I];
        });
    }
    __syncthreads();
    ASX_STAMP_AT(2, stamp_block, 1);
    // every inverse stage but the last: the last one's outputs are consumed from registers below
    // (r reaches neither HBM nor LDS; LDS keeps that stage's input, so the stage can be run again)
    if constexpr (STATIC) pre_last = lds_fft_static_head<S1, true, true>(lds4, Lc, P.tw1, pre);
    else lds_fft<MAXR, true, true>(lds4, PD.st1, Lc, P.tw1, pre); // run-time schedule: the whole transform, r into LDS
    }
    ASX_STAMP_AT(2, stamp_block, 2);

    // ANY earlier value of the running maximum is a lower bound of the final one, so a stale read merely admits
    // more candidates (k_finalize filters them against the final maximum).
    const asx_peak_t run0 = s_run0;
    const float b2 = s_b2;
    const uint32_t seed = WIN ? Z.seed : 0u;
    // the seed's tile (lag 0's without a window) takes the general form: idx >> 1 = j1 M2 + column
    auto seed_tile = [&]() __attribute__((always_inline)) { return (int)(((seed >> 1) % (uint32_t)M2) / (uint32_t)T); };
    auto inw = [&](uint32_t idx) __attribute__((always_inline)) { return !WIN || asx_win_has(Z, idx); };
    // fast scans: out-of-window lags as NaN (a slot is four consecutive lags from i0)
    auto mask4 = [&](float4 g, uint32_t i0) __attribute__((always_inline)) {
        if constexpr (WIN) {
            if (!inw(i0)) g.x = NAN;
            if (!inw(i0 + 1)) g.y = NAN;
            if (!inw(i0 + 2)) g.z = NAN;
            if (!inw(i0 + 3)) g.w = NAN;
        }
        return g;
    };
    if constexpr (!STATIC) {
        // Run-time schedules (lengths outside the reference's six): r lies in LDS and is scanned there.  The
        // scan from the last stage's registers below, instantiated inside the switch over eleven radix bodies,
        // pushed these kernels into scratch (k_inv_cols 0.77 ms against 0.43 ms for the compiled-in schedule).
        const bool fastg = even && (c0 + T <= M2) && (P.nout == P.F) && (WIN ? tile != seed_tile() : tile != 0) && (r_out == nullptr) && shift == 0.0;
        auto examine_slot = [&](int e, float4 g, float thr) {
            const int cg = e & (H - 1), j1 = e >> logH;
            const int j2 = c0 + 2 * cg;
            if (j2 >= M2) return;
            const uint32_t i0 = 2u * ((uint32_t)j1 * (uint32_t)M2 + (uint32_t)j2);
            const float val[4] = { g.x, g.y, g.z, g.w }; // slot = {re0, im0, re1, im1}: four consecutive lags
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const uint32_t idx = i0 + h;
                if ((WIN ? asx_win_has(Z, idx) : idx < P.nout) && j2 + (h >> 1) < M2) {
                    const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                    if (key >= thr) cand_append(W, pair, idx, key);
                }
            }
        };
        if (fastg) {
            // pass 1: per thread the largest and second largest slot maximum; a thread meets its slots in
            // increasing lag order, so a strict '>' keeps the earliest of equal maxima
            float best_m = -INFINITY, second_m = -INFINITY;
            int best_e = threadIdx.x;
            // (the slot's first lag, for the window's mask)
            auto slot_i0 = [&](int e) { return 2u * ((uint32_t)(e >> logH) * (uint32_t)M2 + (uint32_t)(c0 + 2 * (e & (H - 1)))); };
            for (int e = threadIdx.x; e < nelem4; e += nthreads) {
                const float4 g = mask4(lds4[e], WIN ? slot_i0(e) : 0u);
                const float m = fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fmaxf(fabsf(g.z), fabsf(g.w))); // NaNs drop out
                if (m > best_m) { second_m = best_m; best_m = m; best_e = e; }
                else if (m > second_m) second_m = m;
            }
            const float4 gb = mask4(lds4[best_e], WIN ? slot_i0(best_e) : 0u);
            uint32_t my_idx;
            {
                const int cg = best_e & (H - 1), j1 = best_e >> logH;
                const uint32_t i0 = 2u * ((uint32_t)j1 * (uint32_t)M2 + (uint32_t)(c0 + 2 * cg));
                const uint32_t h = fabsf(gb.x) == best_m ? 0u : fabsf(gb.y) == best_m ? 1u : fabsf(gb.z) == best_m ? 2u : 3u;
                my_idx = i0 + h;
            }
            const float wmax = wave_max_nonneg(fmaxf(best_m, 0.f));
            unsigned long long holders = __ballot(best_m == wmax);
            uint32_t widx = 0xFFFFFFFFu;
            while (holders) {
                const int l = __ffsll((long long)holders) - 1;
                const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)my_idx, l);
                widx = li < widx ? li : widx;
                holders &= holders - 1;
            }
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = widx == 0xFFFFFFFFu ? 0 : peak_pack_key(wmax, widx);
            __syncthreads();
            asx_peak_t tb = red[0];
            for (int w = 1; w < (int)((nthreads + 63) >> 6); w++) tb = peak_max(tb, red[w]);
            if (threadIdx.x == 0) atomicMax(&W.pairmax[pair], tb);
            const float thr = near_max_threshold(peak_key(peak_max(tb, run0)), b2);
            if (best_m >= thr) {
                if (second_m >= thr) {
                    for (int e = threadIdx.x; e < nelem4; e += nthreads) {
                        const float4 g = mask4(lds4[e], WIN ? slot_i0(e) : 0u);
                        const float m = fmaxf(fmaxf(fabsf(g.x), fabsf(g.y)), fmaxf(fabsf(g.z), fabsf(g.w)));
                        if (m >= thr) examine_slot(e, g, thr);
                    }
                } else {
                    examine_slot(best_e, gb, thr);
                }
            }
        } else {
            float best_key = -INFINITY;
            uint32_t best_idx = 0xFFFFFFFFu;
            for (int e = threadIdx.x; e < nelem4; e += nthreads) {
                const int cg = e & (H - 1), j1 = e >> logH;
                const int j2 = c0 + 2 * cg;
                if (j2 < M2) {
                    const uint32_t i0 = 2u * ((uint32_t)j1 * (uint32_t)M2 + (uint32_t)j2);
                    const float4 g = lds4[e];
                    const float val[4] = { g.x, g.y, g.z, g.w };
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const uint32_t idx = i0 + h;
                        if (idx < P.nout && j2 + (h >> 1) < M2) {
                            const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                            if (inw(idx) && (key > best_key || (key == best_key && idx < best_idx) || best_idx == 0xFFFFFFFFu)) { best_key = key; best_idx = idx; }
                            if (r_out) r_out[pair * (size_t)P.nout + idx] = val[h];
                        }
                    }
                }
            }
            asx_peak_t best = best_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(best_key, best_idx);
            best = block_peak_max(best, red);
            if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], best); red[0] = best; }
            __syncthreads();
            const float thr = near_max_threshold(peak_key(peak_max(red[0], run0)), b2);
            for (int e = threadIdx.x; e < nelem4; e += nthreads) examine_slot(e, lds4[e], thr);
        }
        ASX_STAMP_AT(2, stamp_block, 3);
    } else {
    auto last_stage = [&](auto &&sink) __attribute__((always_inline)) {
        lds_last_stage_static<S1, true, true>(lds4, Lc, P.tw1, pre_last, sink);
    };

    // Output T of a butterfly is row j1 = pos0 + T*q of column pair g: four consecutive lags
    // {re0, im0, re1, im1} from i0 = 2*(j1*M2 + c0 + 2g).
    // Peak search (src/cross_correlation.c:52-67): largest key, smallest lag among equal keys.
    // Fast path (block-uniform): the tile is full, every lag counts, lag 0 (the signed one) is
    // not in it and r is not being dumped -> one packed maximum per slot, indices resolved at the end.
    const bool fast = even && (c0 + T <= M2) && (P.nout == P.F) && (WIN ? tile != seed_tile() : tile != 0) && (r_out == nullptr) && shift == 0.0;
    // second look (rare, one instantiation for both paths): the thread runs its last stage again and
    // appends every valid lag whose key is inside the window
    auto examine_again = [&](float thr) __attribute__((always_inline)) {
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            const int j2 = c0 + 2 * g;
            if (j2 >= M2) return;
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = 2u * ((uint32_t)(pos0 + t * q) * (uint32_t)M2 + (uint32_t)j2);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + h;
                    if ((WIN ? asx_win_has(Z, idx) : idx < P.nout) && j2 + (h >> 1) < M2) {
                        const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                        if (key >= thr) cand_append(W, pair, idx, key);
                    }
                }
            });
        });
    };
    float thr_again = 0.f;
    bool again = false;
    if (fast) {
        // pass 1: per thread the largest and second largest slot maximum
        float best_m = -INFINITY, second_m = -INFINITY;
        uint32_t best_i0 = 0xFFFFFFFFu;
        float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float4 s4 = mask4(make_float4(v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y),
                                        WIN ? 2u * ((uint32_t)(pos0 + t * q) * (uint32_t)M2 + (uint32_t)(c0 + 2 * g)) : 0u);
                const float m = fmaxf(fmaxf(fabsf(s4.x), fabsf(s4.y)), fmaxf(fabsf(s4.z), fabsf(s4.w))); // NaNs drop out
                const uint32_t i0 = 2u * ((uint32_t)(pos0 + t * q) * (uint32_t)M2 + (uint32_t)(c0 + 2 * g));
                if (m > best_m || (m == best_m && i0 < best_i0)) { second_m = best_m; best_m = m; gb = s4; best_i0 = i0; }
                else if (m > second_m) second_m = m;
            });
        });
        // lag order inside a slot = its memory order {re0, im0, re1, im1}
        const uint32_t hh = fabsf(gb.x) == best_m ? 0u : fabsf(gb.y) == best_m ? 1u : fabsf(gb.z) == best_m ? 2u : 3u;
        const uint32_t my_idx = best_i0 + hh;
        // wave maximum in registers, smallest lag among the lanes that hold it, one entry per wave
        ASX_STAMP_AT(2, stamp_block, 4);
        const float wmax = wave_max_nonneg(fmaxf(best_m, 0.f));
        unsigned long long holders = __ballot(best_m == wmax);
        uint32_t widx = 0xFFFFFFFFu;
        while (holders) {
            const int l = __ffsll((long long)holders) - 1;
            const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)my_idx, l);
            widx = li < widx ? li : widx;
            holders &= holders - 1;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = widx == 0xFFFFFFFFu ? 0 : peak_pack_key(wmax, widx);
        __syncthreads();
        // every thread folds the wave entries itself: no second barrier to broadcast the result
        asx_peak_t tb = red[0];
        for (int w = 1; w < (int)((nthreads + 63) >> 6); w++) tb = peak_max(tb, red[w]);
        if (threadIdx.x == 0) atomicMax(&W.pairmax[pair], tb);
        // Second look: lags within the float32 error window of the largest key known so far.  Almost every
        // thread is below the threshold; the one that holds the maximum usually has no second slot near
        // it and examines just that slot; a thread with more runs its last stage again.
        ASX_STAMP_AT(2, stamp_block, 5);
        const float thr = near_max_threshold(peak_key(peak_max(tb, run0)), b2);
        thr_again = thr;
        if (best_m >= thr) {
            if (second_m >= thr) {
                again = true;
            } else {
                const float val[4] = { gb.x, gb.y, gb.z, gb.w };
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (fabsf(val[h]) >= thr) cand_append(W, pair, best_i0 + h, fabsf(val[h]));
            }
        }
    } else {
        // general form: first tile (lag 0 competes signed), ragged or embedded tiles, r dumped for tests
        float best_key = -INFINITY;
        uint32_t best_idx = 0xFFFFFFFFu;
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            const int j2 = c0 + 2 * g;
            if (j2 >= M2) return;
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = 2u * ((uint32_t)(pos0 + t * q) * (uint32_t)M2 + (uint32_t)j2);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + h;
                    if (idx < P.nout && j2 + (h >> 1) < M2) {
                        const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                        if (inw(idx) && (key > best_key || (key == best_key && idx < best_idx) || best_idx == 0xFFFFFFFFu)) { best_key = key; best_idx = idx; }
                        if (r_out) r_out[pair * (size_t)P.nout + idx] = val[h];
                    }
                }
            });
        });
        asx_peak_t best = best_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(best_key, best_idx);
        best = block_peak_max(best, red);
        if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], best); red[0] = best; }
        __syncthreads();
        const float thr = near_max_threshold(peak_key(peak_max(red[0], run0)), b2);
        again = best_key >= thr;
        thr_again = thr;
    }
    if (again) examine_again(thr_again);
    ASX_STAMP_AT(2, stamp_block, 3);
    } // compiled-in schedules
}

#if ASX_HAS_PART(64)
// ---------------------------------------------------------------------------
// k_finalize: grid (npairs).  Reduce tile partials, wrap the lag, pick segments.
// ---------------------------------------------------------------------------
// sel.seed_of(pair): the index a running maximum that nothing reached stands for -- AsxSelSeed: the lag window's first index (0
// without a window); AsxWinRows (asx_xcorr_windowed_f32_dev): the pair's own, from its row (0 for an invalid row, which lists nothing:
// it never overflows, and k_invalid_rows overwrites its results); AsxSelTopkSeed (top-k passes 2..k): the pass's, from the pair's record.
// Sink: nothing -- or, in the top-k form, unsigned long long: a pair that already overflowed in an earlier pass of the call was
// counted and listed then, its later overflows go to `sink` (asx_plan_peak_overflows counts a pair once per call).
template <class Sel, class... Sink>
__global__ __launch_bounds__(ASX_THREADS) void k_finalize(const AsxDev *__restrict__ Pp, AsxPeakWs W0, AsxSeg *__restrict__ seg,
                                                           uint32_t pair_base, Sel sel, Sink *__restrict__... sink)
{
    static_assert(sizeof...(Sink) <= 1, "the sink or nothing");
    const uint32_t seed = sel.seed_of(blockIdx.x, Pp->N);
    AsxPeakWs W = W0;
    if constexpr (sizeof...(Sink) == 1) {
        if (sel.X[blockIdx.x].flags & ASX_TK_INEXACT) {
            W.overflows = (sink, ...);
            W.over_list = nullptr;
        }
    }
    const uint32_t N = Pp->N;
    __shared__ uint32_t nsel;
    const size_t pair = blockIdx.x;
    const asx_peak_t best = W.pairmax[pair];        // float32 maximum, smallest lag among equal keys
    const uint32_t ntot = W.cand_n[pair];
    const uint32_t n = ntot < W.cap ? ntot : W.cap;
    // the tiles collected against the running maximum; keep what is near the FINAL maximum
    const float thr = near_max_threshold(peak_key(best), W.bound2[pair]);
    if (threadIdx.x == 0) nsel = 0;
    __syncthreads();
    const AsxCand *c = W.cand + pair * (size_t)W.cap;
    uint32_t *out = W.refine_idx + pair * (size_t)W.cap;
    for (uint32_t i = threadIdx.x; i < n; i += ASX_THREADS) {
        const AsxCand e = c[i];
        if (e.key >= thr) out[atomicAdd(&nsel, 1u)] = e.idx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        AsxSeg sg = make_seg(best ? peak_index(best) : seed, N);
        // One candidate: the float32 argmax is unambiguous.  More than the list holds (a signal periodic in
        // more than `cap` lags, an offset of hundreds of deviations in both tracks): the float32 argmax is only a
        // placeholder.  The pair is MARKED (its ret becomes ASX_RET_INEXACT in k_pearson_final), counted
        // (asx_plan_peak_overflows) and put on the list the entry points read to take the second look
        // (asx_api.hip: resolve_overflows): the reference's scan has no candidate limit (src/cross_correlation.c:52-67).
        const bool over = ntot > W.cap;
        if (over) sg.flags = ASX_SEG_INEXACT;
        seg[pair] = sg;
        W.refine_n[pair] = (!over && nsel >= 2u) ? nsel : 0u;
        if (over) {
            atomicAdd(W.overflows, 1ull);
            if (W.over_list) {
                const uint32_t slot = atomicAdd(W.over_n, 1u);
                if (slot < W.over_cap) W.over_list[slot] = pair_base + (uint32_t)pair;
                if (W.over_host) (void)__hip_atomic_fetch_add(W.over_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// grid (npairs / ASX_THREADS): behind the Pearson kernels of pass j of a top-k group (asx_xcorr_topk_f32_dev).  Pass j's result of
// each pair (in the group's temporaries) becomes entry j of the caller's arrays (index pair * k + j): (0, NaN, -2) for an invalid
// row, (0, NaN, -3) once A_j is empty, ret = 1 from an overflowed pass on.  Then, unless j is the last pass, the zone around the
// entry's lag joins the pair's record, the next pass's seed is the smallest index left in the window (none: the record is marked
// empty and its window holds nothing), and the per-pair state of the peak search that k_rows zeroes is zeroed again.  j = 0 starts
// the record from the call's window: the plan's (win_lo, win_hi) or the pair's row.
__device__ inline int64_t tk_first_free(const AsxTopkPair *__restrict__ t, uint32_t nz, int64_t l, int64_t end)
{
    // the smallest lag >= l and <= end outside the record's first nz zones (end + 1: none); a zone once passed is never met again
    for (int it = 0; it < ASX_TOPK_MAX; it++) {
        bool moved = false;
        for (uint32_t i = 0; i < nz; i++) {
            const int64_t lo = t->lo[i], hi = lo + (int64_t)t->wd[i];
            if (lo <= l && l <= hi) { l = hi + 1; moved = true; }
        }
        if (!moved || l > end) break;
    }
    return l <= end ? l : end + 1;
}

__global__ __launch_bounds__(ASX_THREADS) void k_topk_step(AsxTopkWs T, const AsxSeg *__restrict__ seg, AsxPeakWs W, int64_t win_lo,
                                                            int64_t win_hi, AsxWinRows R, uint32_t N, int npairs, int j, int k,
                                                            int64_t sep, int64_t *__restrict__ lag, double *__restrict__ coef,
                                                            int32_t *__restrict__ ret)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs) return;
    const int64_t n = (int64_t)N;
    AsxTopkPair *t = T.pairs + pair; // (fields one by one: a whole record in registers, indexed by nz, went to scratch)
    uint32_t flags, nz;
    if (j == 0) {
        int64_t lo = win_lo, hi = win_hi;
        AsxWin z;
        flags = 0;
        if (R.rows) {
            const int64_t *row = R.rows + 2 * (size_t)pair * R.step;
            lo = row[0];
            hi = row[1];
            if (!asx_win_row(R, (size_t)pair, N, z)) flags = ASX_TK_INVALID;
        } else {
            z = asx_win_of(lo, hi, N);
        }
        t->z = z;
        t->wlo = (int32_t)lo;
        t->whi = (int32_t)hi;
        nz = 0;
    } else {
        flags = t->flags;
        nz = t->nz;
    }
    const AsxSeg sg = seg[pair];
    if (sg.flags & ASX_SEG_INEXACT) flags |= ASX_TK_INEXACT;
    int64_t l = T.lag[pair];
    double c = T.coef[pair];
    int32_t r = T.ret[pair];
    if (flags & ASX_TK_INVALID) { l = 0; c = (double)NAN; r = -2; }
    else if (flags & ASX_TK_EMPTY) { l = 0; c = (double)NAN; r = -3; }
    if ((flags & ASX_TK_INEXACT) && !(flags & ASX_TK_INVALID)) r = 1; // (the zones of the entries from here on came from a float32 argmax)
    const size_t e = (size_t)pair * (size_t)k + (size_t)j;
    if (lag) lag[e] = l;
    coef[e] = c;
    ret[e] = r;
    if (j + 1 >= k) return;
    if (!(flags & (ASX_TK_INVALID | ASX_TK_EMPTY))) {
        const int64_t d = sep < 2 * n ? sep : 2 * n;
        const int64_t zlo = sg.lag - d < -n ? -n : sg.lag - d, zhi = sg.lag + d > n - 1 ? n - 1 : sg.lag + d;
        t->lo[nz] = (int32_t)zlo;
        t->wd[nz] = (uint32_t)(zhi - zlo);
        nz++;
        // ascending index order: the lags max(lo, 0) .. hi, then lo .. min(hi, -1)
        const int64_t lo = t->wlo, hi = t->whi;
        int64_t seed = -1;
        if (hi >= 0) {
            const int64_t f = tk_first_free(t, nz, lo > 0 ? lo : 0, hi);
            if (f <= hi) seed = f;
        }
        if (seed < 0 && lo < 0) {
            const int64_t e1 = hi < -1 ? hi : -1, f = tk_first_free(t, nz, lo, e1);
            if (f <= e1) seed = 2 * n + f;
        }
        if (seed < 0) {
            flags |= ASX_TK_EMPTY;
            t->z.n = 0; // nothing competes: the running maximum stays empty and stands for index 0
            t->z.seed = 0;
        } else {
            t->z.seed = (uint32_t)seed;
        }
    }
    t->nz = nz;
    t->flags = flags;
    W.pairmax[pair] = 0;
    W.cand_n[pair] = 0;
}

// grid (npairs / ASX_THREADS): what the step of a PHAT top-k group (asx_xcorr_phat_topk_f32_dev) adds, launched IN FRONT of pass j's
// k_topk_step: entry j's peak height.  The pass's running maximum is still in pairmax (k_phat_finalize only read it; the step zeroes
// it), so peak[pair * k + j] is formed as k_phat_finalize forms the one-entry call's -- |key| / f, 0 for an empty maximum, NaN for a
// NaN seed -- and is NaN where the step is about to write -2 or -3: the record's flags say so from pass 1 on (an earlier step set
// them), the pair's row in pass 0.  k_topk_step needs no PHAT form of its own: no pass of a PHAT group marks its segment, so ret is
// never 1, and bound2 stays what row 0 of the PHAT row kernel set (FLT_MIN, or 0 for a silent track).
__global__ __launch_bounds__(ASX_THREADS) void k_topk_peak(const AsxTopkPair *__restrict__ X, const asx_peak_t *__restrict__ pairmax,
                                                            AsxWinRows R, uint32_t N, int npairs, int j, int k, double f,
                                                            double *__restrict__ peak)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs) return;
    bool entry;
    if (j == 0) {
        AsxWin z;
        entry = !R.rows || asx_win_row(R, (size_t)pair, N, z);
    } else {
        entry = !(X[pair].flags & (ASX_TK_INVALID | ASX_TK_EMPTY));
    }
    const asx_peak_t best = pairmax[pair];
    const float key = best ? peak_key(best) : 0.f;
    peak[(size_t)pair * (size_t)k + (size_t)j] = (!entry || key == -INFINITY) ? (double)NAN : fabs((double)key) / f;
}

// grid (npairs / ASX_THREADS): behind k_pearson_final / k_pearson_final_spec of a group with per-pair windows, the pairs whose row is
// invalid (asx_win_row) get lag 0, a NaN coefficient and ret -2; the others are not touched
__global__ __launch_bounds__(ASX_THREADS) void k_invalid_rows(AsxWinRows R, uint32_t N, int npairs, int64_t *__restrict__ lag,
                                                               double *__restrict__ coef, int32_t *__restrict__ ret)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs) return;
    AsxWin Z;
    if (asx_win_row(R, (size_t)pair, N, Z)) return;
    if (lag) lag[pair] = 0;
    coef[pair] = (double)NAN;
    ret[pair] = -2;
}

// grid (npairs / ASX_THREADS): behind the Pearson kernels (and k_invalid_rows) of a pool group, the pairs with an index outside its pool
// (ASX_POOL_INVALID) get lag 0, a NaN coefficient and ret -4; the others are not touched.  peak: null, or the peak heights of a PHAT
// pool group (asx_xcorr_pool_phat_f32_dev), where such a pair gets NaN over the 0 that k_phat_finalize wrote for its empty maximum.
__global__ __launch_bounds__(ASX_THREADS) void k_invalid_pairs(const AsxPoolPair *__restrict__ PL, int npairs, int64_t *__restrict__ lag,
                                                                double *__restrict__ coef, int32_t *__restrict__ ret,
                                                                double *__restrict__ peak)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs || !(PL[pair].flags & ASX_POOL_INVALID)) return;
    if (lag) lag[pair] = 0;
    coef[pair] = (double)NAN;
    ret[pair] = -4;
    if (peak) peak[pair] = (double)NAN;
}

// the k-entry form (asx_xcorr_pool_topk_f32_dev): behind the LAST k_topk_step of a pool group, all k entries (index pair * k + j) of
// such a pair, over whatever the steps wrote there (-2 and -3 included)
__global__ __launch_bounds__(ASX_THREADS) void k_invalid_pairs_k(const AsxPoolPair *__restrict__ PL, int npairs, int k,
                                                                  int64_t *__restrict__ lag, double *__restrict__ coef,
                                                                  int32_t *__restrict__ ret)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs || !(PL[pair].flags & ASX_POOL_INVALID)) return;
    for (int j = 0; j < k; j++) {
        const size_t e = (size_t)pair * (size_t)k + (size_t)j;
        if (lag) lag[e] = 0;
        coef[e] = (double)NAN;
        ret[e] = -4;
    }
}

// ... of a PHAT pool group whose call asked for the peak heights (asx_xcorr_pool_phat_topk_f32_dev): a NaN peak in all k entries as well
__global__ __launch_bounds__(ASX_THREADS) void k_invalid_pairs_kp(const AsxPoolPair *__restrict__ PL, int npairs, int k,
                                                                   int64_t *__restrict__ lag, double *__restrict__ coef,
                                                                   int32_t *__restrict__ ret, double *__restrict__ peak)
{
    const int pair = blockIdx.x * ASX_THREADS + threadIdx.x;
    if (pair >= npairs || !(PL[pair].flags & ASX_POOL_INVALID)) return;
    for (int j = 0; j < k; j++) {
        const size_t e = (size_t)pair * (size_t)k + (size_t)j;
        if (lag) lag[e] = 0;
        coef[e] = (double)NAN;
        ret[e] = -4;
        peak[e] = (double)NAN;
    }
}

// ---------------------------------------------------------------------------
// Exact re-evaluation of near-tied lags: r[k] = sum_{n<N} source[(n+k) mod 2N] * sample[n]
// (the identity behind src/cross_correlation.c:232-239), accumulated as an
// unevaluated sum of two doubles (error ~1e-30 relative: the products of float32 inputs are exact
// in float64, those of float64 inputs carry their rounding error along via fma).
// grid (ASX_DOT_BLOCKS, npairs): block x of a pair takes candidates x, x + gridDim.x, ...
// ---------------------------------------------------------------------------
struct dd_t {
    double hi, lo;
};
__device__ __forceinline__ dd_t dd_add(dd_t a, dd_t b)
{
    const double s = a.hi + b.hi;
    const double bb = s - a.hi;
    double e = (a.hi - (s - bb)) + (b.hi - bb);
    e += a.lo + b.lo;
    dd_t r;
    r.hi = s + e;
    r.lo = e - (r.hi - s);
    return r;
}

// at: where pair i's inputs start, in elements from src / smp -- AsxAtPitch, or AsxAtList (asx_xcorr_pool_f32_dev, float inputs)
template <typename TIn, class Where>
__global__ __launch_bounds__(ASX_THREADS) void k_refine_dots(const AsxDev *__restrict__ Pp, const TIn *__restrict__ src,
                                                              const TIn *__restrict__ smp, Where at, AsxPeakWs W)
{
    __shared__ double red[2][ASX_THREADS / 64];
    const size_t pair = blockIdx.y;
    const uint32_t ncand = W.refine_n[pair];
    if (blockIdx.x >= ncand) return;
    const uint32_t N = Pp->N, L = 2u * N;
    const TIn *x = src + at.src_off(pair);
    const TIn *y = smp + at.smp_off(pair);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < ncand; c += gridDim.x) {
        const uint32_t k = W.refine_idx[pair * (size_t)W.cap + c];
        double hi = 0.0, lo = 0.0;
        for (uint32_t n = threadIdx.x; n < N; n += ASX_THREADS) {
            uint32_t i = n + k;
            if (i >= L) i -= L;
            const double a = (double)x[i], b = (double)y[n];
            const double p = a * b;
            double pe = 0.0;
            if (sizeof(TIn) == sizeof(double)) pe = fma(a, b, -p);
            const double s = hi + p;
            const double bb = s - hi;
            lo += ((hi - (s - bb)) + (p - bb)) + pe;
            hi = s;
        }
        dd_t acc;
        acc.hi = hi; acc.lo = lo;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            dd_t o;
            o.hi = __shfl_xor(acc.hi, off, 64);
            o.lo = __shfl_xor(acc.lo, off, 64);
            acc = dd_add(acc, o);
        }
        if (lane == 0) { red[0][wave] = acc.hi; red[1][wave] = acc.lo; }
        __syncthreads();
        if (threadIdx.x == 0) {
            dd_t t;
            t.hi = red[0][0]; t.lo = red[1][0];
            for (int w = 1; w < ASX_THREADS / 64; w++) {
                dd_t o;
                o.hi = red[0][w]; o.lo = red[1][w];
                t = dd_add(t, o);
            }
            W.refine_val[pair * (size_t)W.cap + c] = t.hi + t.lo;
        }
        __syncthreads();
    }
}

// grid (npairs): the reference's max_abs_index rule (src/cross_correlation.c:52-67) on the exact values:
// key(seed) = r[seed] signed, key(i) = |r[i]|, largest key, smallest lag among equal keys; a NaN key never
// wins unless it sits at the seed (index 0, or the first index of a lag window: AsxWin).
// sel.seed_of(pair): the plan's (AsxSelSeed), the pair's own from its row (AsxWinRows) or the pass's from the pair's top-k record
// (AsxSelTopkSeed).
template <class Sel>
__global__ __launch_bounds__(ASX_THREADS) void k_refine_pick(const AsxDev *__restrict__ Pp, AsxPeakWs W, AsxSeg *__restrict__ seg,
                                                              Sel sel)
{
    const uint32_t seed = sel.seed_of(blockIdx.x, Pp->N);
    __shared__ double rkey[ASX_THREADS / 64];
    __shared__ uint32_t ridx[ASX_THREADS / 64];
    const size_t pair = blockIdx.x;
    const uint32_t n = W.refine_n[pair];
    if (n < 2u) return;
    double bk = -INFINITY;
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < n; i += ASX_THREADS) {
        const uint32_t idx = W.refine_idx[pair * (size_t)W.cap + i];
        const double v = W.refine_val[pair * (size_t)W.cap + i];
        double key;
        if (idx == seed) key = (v != v) ? (double)INFINITY : v + 0.0;
        else { key = fabs(v); if (key != key) key = -(double)INFINITY; }
        if (key > bk || (key == bk && idx < bi)) { bk = key; bi = idx; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ok = __shfl_xor(bk, off, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off, 64);
        if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { rkey[wave] = bk; ridx[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ASX_THREADS / 64; w++)
            if (rkey[w] > bk || (rkey[w] == bk && ridx[w] < bi)) { bk = rkey[w]; bi = ridx[w]; }
        if (bi != 0xFFFFFFFFu) seg[pair] = make_seg(bi, Pp->N);
    }
}

// ---------------------------------------------------------------------------
// Pearson coefficient (src/cross_correlation.c:74-116).  The reference makes two passes (means, then
// the centred sums); here ONE streaming pass gives the same numbers: every thread accumulates its
// elements relative to a pivot (its own first element), turns the five sums into
// (count, mean, centred second moments) and the partitions are merged pairwise with the exact update
// formulas (Chan et al.): no large-offset cancellation anywhere (offset 1e6, amplitude 0.1 is fine).
// The merge tree is fixed, and x and y go through the same operations, so identical segments give
// bit-identical Mxx, Myy, Cxy and therefore exactly +-1.0 (tests/test_cross_correlation.c:29).
// ---------------------------------------------------------------------------
// (PStat, pstat_merge, pstat_wave_merge: xcorr_dev.h -- shared with pearson_spectral.hip)
// steps of k_pearson_partial's loop whose loads are in flight together (0 = one step at a time, as it was): the direct form 0.200 -> 0.190 ms
// per 124 pairs of N = 1 440 000, the spectral form's remainder 0.090 -> 0.087 (profiles/r5_experiments/24_*); the same additions in the same order
#ifndef ASX_PEARSON_DEEP
#define ASX_PEARSON_DEEP 4
#endif
// Where (asx_internal.h, Inputs): pair i's inputs at src + at.src_off(i), smp + at.smp_off(i) -- AsxAtPitch, or AsxAtList in a pool
// call (asx_xcorr_pool_f32_dev, float inputs only)
template <typename TIn, bool SPEC, class Where>
__global__ __launch_bounds__(ASX_THREADS) void k_pearson_partial(const TIn *__restrict__ src, const TIn *__restrict__ smp, Where at,
                                                                  uint32_t basis_len, const AsxSeg *__restrict__ seg,
                                                                  double *__restrict__ psums, AsxSpecWs V)
{
    __shared__ double red[6][ASX_THREADS / 64];
    const size_t pair = blockIdx.y;
    AsxSeg s = seg[pair];
    // SPEC (the spectral Pearson form): what this pair still needs read -- nothing, its wrap-around part, or its segment -- follows from
    // the sums k_pearson_prep left; every block works that out for itself (pair-uniform: scalar loads and arithmetic)
    // Block 0 also RECORDS the mode (the spare header slot): k_pearson_final_spec, in another translation unit, reads it instead of
    // deciding again -- with -ffp-contract=fast two inlining contexts may round `bound <= tol` differently at the threshold, and a final
    // kernel that disagreed with the work list would read partial sums written for another mode.  One writer, a later
    // kernel reads: no fence.
    if constexpr (SPEC) {
        const AsxSpecPick d = asx_spec_pick(s, V.part + pair * (size_t)(V.nb * 4), V.nb, V.hdr + pair * ASX_SPEC_HDR, V.tol, V.N);
        s = d.work;
        if (blockIdx.x == 0 && threadIdx.x == 0) V.hdr[pair * ASX_SPEC_HDR + 3] = (double)d.mode;
    }
    // gridDim.x partial blocks per pair (asx_pearson_blocks: by the basis length alone); the final kernel merges
    // exactly gridDim.x entries
    const uint32_t chunk = (basis_len + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = (uint64_t)blockIdx.x * chunk;
    uint64_t hi = lo + chunk;
    if (hi > s.len) hi = s.len;
    if (lo >= s.len) {
        // nothing of the segment falls to this block (block-uniform): an empty record (pstat_merge skips n == 0) -- the whole
        // launch for a pair the spectral form has settled (pearson_spectral.hip), the tail of a short segment otherwise
        if (threadIdx.x == 0) psums[(pair * gridDim.x + blockIdx.x) * 6] = 0.0;
        return;
    }
    const TIn *x = src + at.src_off(pair) + s.src_off;
    const TIn *y = smp + at.smp_off(pair) + s.smp_off;
    uint64_t i = lo + 4u * threadIdx.x;
    double px = 0, py = 0; // pivots: the first element this thread meets
#if ASX_PEARSON_DEEP
    // (taken from the first 16-byte load below when the thread has one: a scalar load and the wait for it in front of the loop otherwise)
    if (i < hi && !(i + 3 < hi)) { px = (double)x[i]; py = (double)y[i]; }
#else
    if (i < hi) { px = (double)x[i]; py = (double)y[i]; }
#endif
    double sx = 0, sy = 0, sxy = 0, sxx = 0, syy = 0;
    uint32_t cnt = 0;
    auto add = [&](double a, double b) {
        const double da = a - px, db = b - py;
        sx += da;
        sy += db;
        sxy += da * db;
        sxx += da * da;
        syy += db * db;
        cnt++;
    };
    // four consecutive elements per lane and step: 16-byte loads (the segments start at any element,
    // so the vector type only promises element alignment), then the few elements that are left
    typedef TIn vec4u __attribute__((ext_vector_type(4), aligned(sizeof(TIn))));
    auto ld4 = [&](const TIn *p) __attribute__((always_inline)) {
        return (ASX_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const vec4u *>(p)) : *reinterpret_cast<const vec4u *>(p);
    };
#if ASX_PEARSON_DEEP
    // ASX_PEARSON_DEEP steps at a time: their 2 * ASX_PEARSON_DEEP loads in flight together, then the same additions in the same order (the
    // loop used to wait for each step's two loads before it issued the next step's: 16 memory round trips per block, one after the other)
    {
        bool first = i + 3 < hi;
        constexpr uint32_t STEP = 4u * ASX_THREADS;
        for (; i + 3 + (uint64_t)(ASX_PEARSON_DEEP - 1) * STEP < hi; i += (uint64_t)ASX_PEARSON_DEEP * STEP) {
            vec4u a[ASX_PEARSON_DEEP], b[ASX_PEARSON_DEEP];
#pragma unroll
            for (int u = 0; u < ASX_PEARSON_DEEP; u++) { a[u] = ld4(x + i + (uint64_t)u * STEP); b[u] = ld4(y + i + (uint64_t)u * STEP); }
            if (first) { px = (double)a[0].x; py = (double)b[0].x; first = false; }
#pragma unroll
            for (int u = 0; u < ASX_PEARSON_DEEP; u++) {
                add((double)a[u].x, (double)b[u].x);
                add((double)a[u].y, (double)b[u].y);
                add((double)a[u].z, (double)b[u].z);
                add((double)a[u].w, (double)b[u].w);
            }
        }
        if (first) { px = (double)x[i]; py = (double)y[i]; } // fewer than ASX_PEARSON_DEEP whole steps: the step loop below meets it first
    }
#endif
    for (; i + 3 < hi; i += 4u * ASX_THREADS) {
        const vec4u a = (ASX_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const vec4u *>(x + i)) : *reinterpret_cast<const vec4u *>(x + i);
        const vec4u b = (ASX_NT & 4) ? __builtin_nontemporal_load(reinterpret_cast<const vec4u *>(y + i)) : *reinterpret_cast<const vec4u *>(y + i);
        add((double)a.x, (double)b.x);
        add((double)a.y, (double)b.y);
        add((double)a.z, (double)b.z);
        add((double)a.w, (double)b.w);
    }
    for (; i < hi; i++) add((double)x[i], (double)y[i]); // only the lane that holds the ragged end
    PStat v;
    v.n = (double)cnt;
    v.mx = v.my = v.mxx = v.myy = v.cxy = 0.0;
    if (cnt) {
        v.mx = px + sx / v.n;
        v.my = py + sy / v.n;
        v.mxx = sxx - sx * sx / v.n;
        v.myy = syy - sy * sy / v.n;
        v.cxy = sxy - sx * sy / v.n;
    }
    v = pstat_wave_merge(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = v.n; red[1][wave] = v.mx; red[2][wave] = v.my;
        red[3][wave] = v.mxx; red[4][wave] = v.myy; red[5][wave] = v.cxy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ASX_THREADS / 64; w++) {
            PStat o;
            o.n = red[0][w]; o.mx = red[1][w]; o.my = red[2][w];
            o.mxx = red[3][w]; o.myy = red[4][w]; o.cxy = red[5][w];
            v = pstat_merge(v, o);
        }
        double *out = psums + (pair * gridDim.x + blockIdx.x) * 6;
        out[0] = v.n; out[1] = v.mx; out[2] = v.my; out[3] = v.mxx; out[4] = v.myy; out[5] = v.cxy;
    }
}

// grid (npairs), one wave per pair: lane b owns the partial blocks b, b + 64, ... (merged in that order: a fixed tree for a
// given block count, the same for x and y).
// (Pick, partial sums and this merge as ONE kernel -- the last block to arrive at a per-pair counter merges -- was
// measured: the release-acquire increment per block took the batch pass from 0.20 to 0.60 ms and the single pair
// gained nothing, its latency is the chain of dependent loads inside the kernels, not their number.)
__global__ __launch_bounds__(64) void k_pearson_final(const AsxSeg *__restrict__ seg,
                                                       const double *__restrict__ psums, uint32_t nb,
                                                       int64_t *__restrict__ lag,
                                                       double *__restrict__ coef,
                                                       int32_t *__restrict__ ret)
{
    const size_t pair = blockIdx.x;
    PStat v;
    v.n = v.mx = v.my = v.mxx = v.myy = v.cxy = 0.0;
    for (uint32_t b = threadIdx.x; b < nb; b += 64u) {
        const double *p = psums + (pair * nb + b) * 6;
        PStat o;
        o.n = p[0]; o.mx = p[1]; o.my = p[2]; o.mxx = p[3]; o.myy = p[4]; o.cxy = p[5];
        v = pstat_merge(v, o);
    }
    v = pstat_wave_merge(v);
    if (threadIdx.x == 0) {
        const AsxSeg s = seg[pair];
        // src/cross_correlation.c:115; an empty or constant segment gives 0/0 = NaN like the reference
        const double c = v.cxy / sqrt(v.mxx * v.myy);
        if (lag) lag[pair] = s.lag;
        coef[pair] = c;
        // src/cross_correlation.c:276: NaN coefficient -> return -1 (outputs already written)
        // ... unless the lag itself is still the float32 placeholder of an overflowed pair: 1 = "inexact, look again"
        // (only ever visible to callers of the asynchronous mode, include/audiosync/xcorr_hip.h)
        if (ret) ret[pair] = (s.flags & ASX_SEG_INEXACT) ? 1 : (c != c) ? -1 : 0;
    }
}

// ---------------------------------------------------------------------------
// result consumers: the acceptance threshold and frames -> milliseconds of
// src/audiosync.c:254-256 for a whole batch
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ASX_THREADS) void k_results_to_ms(const int64_t *__restrict__ lag,
                                                                const double *__restrict__ coef,
                                                                const int32_t *__restrict__ ret, size_t batch,
                                                                double min_confidence, double ms_per_frame,
                                                                int64_t *__restrict__ lag_ms,
                                                                int32_t *__restrict__ accept)
{
    const size_t i = (size_t)blockIdx.x * ASX_THREADS + threadIdx.x;
    if (i >= batch) return;
    lag_ms[i] = (int64_t)round((double)lag[i] * ms_per_frame);
    if (accept) accept[i] = (ret[i] == 0 && coef[i] >= min_confidence) ? 1 : 0;
}

// The entry a caller of the top-k calls keeps, one thread per pair: among the pair's k entries (index pair * k + j) with ret == 0 the
// largest SIGNED coefficient (the acceptance above is signed too), the smallest j among equals; none with ret == 0: entry 0 as it is.
// Its (lag, coef, ret) go to index pair -- the layout k_results_to_ms takes -- and j to best_entry.
__global__ __launch_bounds__(ASX_THREADS) void k_topk_best(const int64_t *__restrict__ lag, const double *__restrict__ coef,
                                                            const int32_t *__restrict__ ret, size_t batch, int k,
                                                            int64_t *__restrict__ best_lag, double *__restrict__ best_coef,
                                                            int32_t *__restrict__ best_ret, int32_t *__restrict__ best_entry)
{
    const size_t i = (size_t)blockIdx.x * ASX_THREADS + threadIdx.x;
    if (i >= batch) return;
    const size_t e0 = i * (size_t)k;
    int bj = -1;
    double bc = 0.0;
    for (int j = 0; j < k; j++) {
        if (ret[e0 + j] != 0) continue;
        const double c = coef[e0 + j];
        if (bj < 0 || c > bc) { bj = j; bc = c; }
    }
    const int j = bj < 0 ? 0 : bj;
    if (best_lag) best_lag[i] = lag[e0 + j];
    best_coef[i] = coef[e0 + j];
    best_ret[i] = ret[e0 + j];
    if (best_entry) best_entry[i] = j;
}

// ---------------------------------------------------------------------------
// Triangle closure over one clip pool (asx_pool_closure_dev): the tables are [C][C][k], pair (a, b) at a * C + b, and the lag of
// (a, b) estimates T_b - T_a, so lag_ac + lag_cb = lag_ab and lag_ab = -lag_ba.  Everything below is integer arithmetic (counts
// and int64 sums of lags within +-ASX_CLOSURE_LAG_LIMIT); only the pick compares coefficients.  C * C * k <= INT32_MAX: 32-bit indices.
// ---------------------------------------------------------------------------
#define ASX_CLOSURE_CH 256                          // clips of row (a, ., .) staged in LDS at a time
#define ASX_CLOSURE_BT 16                           // the b of one block: four per wave
#define ASX_CLOSURE_INV ((int64_t)1 << 60)          // a lag that is not valid: no sum that holds it is near a valid lag
#define ASX_CLOSURE_TINV (-((int64_t)1 << 62))      // ... and the target of an entry that is not valid: near no sum

// (closure_valid, closure_good, closure_usable, closure_block_sum and the rank-counting lower median: closure_dev.h, shared with place.hip)

// Vote and pick.  Block (x, y): clip a = y and the clips b = x * BT .. x * BT + BT - 1.  The row (a, c, p) goes through LDS once per
// block in chunks of CH clips c, as [p][c] so that the 64 lanes of a wave read 64 consecutive int64; a lag that is not valid is
// stored as INV.  Wave w takes b = w, w + 4, ...; its lanes run over c and read the column entry (c, b, .) -- k * 8 contiguous bytes
// per lane at a stride of C * k * 8 -- straight from global memory: the b of a block are neighbours, so the 16 * k * 8 contiguous
// bytes of (c, b0 .. b0 + 15, .) are the whole of the lines a lane touches, and the table (C * C * k * 12 bytes) is read by every
// a from L2.  The lane with c == b takes the reverse pair instead: P = {0}, Q = -lag(b, a, .).  |s - lag_j| <= tol is
// (uint64)(s - (lag_j - tol)) <= 2 tol; each lane forms its k x k sums and a mask of the j it supports, a ballot and a popcount per
// j count the clips, and the wave that owns b adds them to the block's counters.
__global__ __launch_bounds__(ASX_THREADS) void k_closure_votes(const int64_t *__restrict__ lag, const double *__restrict__ coef,
                                                                const int32_t *__restrict__ ret, uint32_t C, int k, int64_t tol,
                                                                int32_t *__restrict__ votes, int64_t *__restrict__ best_lag,
                                                                double *__restrict__ best_coef, int32_t *__restrict__ best_ret,
                                                                int32_t *__restrict__ best_entry)
{
    __shared__ int64_t rowP[ASX_TOPK_MAX * ASX_CLOSURE_CH];
    __shared__ int32_t cnt[ASX_CLOSURE_BT][ASX_TOPK_MAX];
    const uint32_t a = blockIdx.y, b0 = blockIdx.x * ASX_CLOSURE_BT;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t tol2 = 2u * (uint64_t)tol;
    if (threadIdx.x < ASX_CLOSURE_BT * ASX_TOPK_MAX) (&cnt[0][0])[threadIdx.x] = 0;
    for (uint32_t c0 = 0; c0 < C; c0 += ASX_CLOSURE_CH) {
        __syncthreads();                                        // the chunk before this one has been read
        const uint32_t nch = min((uint32_t)ASX_CLOSURE_CH, C - c0), row0 = (a * C + c0) * (uint32_t)k;
        for (uint32_t i = threadIdx.x; i < nch * (uint32_t)k; i += ASX_THREADS) {
            const uint32_t cl = i / (uint32_t)k, p = i - cl * (uint32_t)k;
            const int64_t v = lag[row0 + i];
            rowP[p * ASX_CLOSURE_CH + cl] = closure_valid(v, ret[row0 + i]) ? v : ASX_CLOSURE_INV;
        }
        __syncthreads();
        for (uint32_t bt = w; bt < ASX_CLOSURE_BT; bt += ASX_THREADS / 64) {
            const uint32_t b = b0 + bt;
            if (b >= C || b == a) continue;                     // (the same in every lane of the wave)
            int64_t T[ASX_TOPK_MAX];
#pragma unroll
            for (int j = 0; j < ASX_TOPK_MAX; j++) {
                T[j] = ASX_CLOSURE_TINV;
                if (j < k) {
                    const uint32_t e = (a * C + b) * (uint32_t)k + (uint32_t)j;
                    const int64_t v = lag[e];
                    if (closure_valid(v, ret[e])) T[j] = v - tol;
                }
            }
            int32_t wc[ASX_TOPK_MAX];
#pragma unroll
            for (int j = 0; j < ASX_TOPK_MAX; j++) wc[j] = 0;
            for (uint32_t ci = 0; ci < nch; ci += 64) {
                const uint32_t cl = ci + lane, c = c0 + cl;
                uint32_t mask = 0;                              // (a predicate per j instead, held as lane masks, measured 1.4 x slower)
                if (cl < nch && c != a) {
                    const bool rev = c == b;
                    const uint32_t q0 = (rev ? b * C + a : c * C + b) * (uint32_t)k;
                    int64_t Q[ASX_TOPK_MAX];
#pragma unroll
                    for (int q = 0; q < ASX_TOPK_MAX; q++) {
                        Q[q] = ASX_CLOSURE_INV;
                        if (q < k) {
                            const int64_t v = lag[q0 + (uint32_t)q];
                            if (closure_valid(v, ret[q0 + (uint32_t)q])) Q[q] = rev ? -v : v;
                        }
                    }
                    for (int p = 0; p < k; p++) {
                        int64_t P = rowP[p * ASX_CLOSURE_CH + cl];
                        if (rev) P = p == 0 ? 0 : ASX_CLOSURE_INV;
#pragma unroll
                        for (int q = 0; q < ASX_TOPK_MAX; q++) {
                            if (q < k) {
                                const int64_t s = P + Q[q];
#pragma unroll
                                for (int j = 0; j < ASX_TOPK_MAX; j++) mask |= ((uint64_t)(s - T[j]) <= tol2 ? 1u : 0u) << j;
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < ASX_TOPK_MAX; j++) wc[j] += (int32_t)__popcll(__ballot((mask >> j) & 1u));
            }
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < ASX_TOPK_MAX; j++) cnt[bt][j] += wc[j];
            }
        }
    }
    __syncthreads();
    // the pick, one thread per b: more votes, then the larger coefficient (strictly: a NaN never wins), then the smaller j
    const uint32_t b = b0 + threadIdx.x;
    if (threadIdx.x >= ASX_CLOSURE_BT || b >= C) return;
    const uint32_t pair = a * C + b, e0 = pair * (uint32_t)k;
    int bj = -1;
    int32_t bv = 0;
    double bc = 0.0;
    for (int j = 0; j < k; j++) {
        const int32_t v = cnt[threadIdx.x][j];                  // 0 on the diagonal and for an entry that is not valid
        if (votes) votes[e0 + (uint32_t)j] = v;
        if (!closure_valid(lag[e0 + (uint32_t)j], ret[e0 + (uint32_t)j])) continue;
        const double c = coef[e0 + (uint32_t)j];
        if (bj < 0 || v > bv || (v == bv && c > bc)) { bj = j; bv = v; bc = c; }
    }
    const uint32_t e = e0 + (uint32_t)(bj < 0 ? 0 : bj);
    best_lag[pair] = lag[e];
    reinterpret_cast<int64_t *>(best_coef)[pair] = reinterpret_cast<const int64_t *>(coef)[e];   // the bits, a NaN's payload too
    best_ret[pair] = ret[e];
    best_entry[pair] = bj < 0 ? 0 : bj;
}

// Confirm, one wave per pair (a, b), lanes over the third clip c: only the PICKED lags L vote.  The lane with c == b takes (b, a).
__global__ __launch_bounds__(ASX_THREADS) void k_closure_confirm(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                                  uint32_t C, int64_t tol, int32_t *__restrict__ confirm)
{
    const uint32_t pair = blockIdx.x * (ASX_THREADS / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pair >= C * C) return;
    const uint32_t a = pair / C, b = pair - a * C, lane = threadIdx.x & 63u;
    int32_t n = 0;
    if (closure_good(L, R, C, a, b)) {
        const int64_t lab = L[pair];
        for (uint32_t c0 = 0; c0 < C; c0 += 64) {
            const uint32_t c = c0 + lane;
            bool hit = false;
            if (c < C && c != a) {
                int64_t d = INT64_MAX;
                if (c == b) { if (closure_good(L, R, C, b, a)) d = lab + L[b * C + a]; }
                else if (closure_good(L, R, C, a, c) && closure_good(L, R, C, c, b)) d = L[a * C + c] + L[c * C + b] - lab;
                hit = d >= -tol && d <= tol;
            }
            n += (int32_t)__popcll(__ballot(hit));
        }
    }
    if (lane == 0) confirm[pair] = n;
}

// The root, one block: the given clip, or the one with the most usable pairs (a, .) and (., a), the smallest index among equals.
// Scores are counted a tile of ASX_THREADS clips at a time in LDS, in two passes that both read consecutive pairs: the rows (a, .)
// of the tile's clips, then per clip b the run (b, a0 .. a0 + tile - 1) of their columns.  Integer atomics: no order shows.
__global__ __launch_bounds__(ASX_THREADS) void k_closure_root(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                               const int32_t *__restrict__ F, uint32_t C, int min_confirm, int root,
                                                               int32_t *__restrict__ out)
{
    __shared__ int32_t score[ASX_THREADS];
    __shared__ int32_t red_s[ASX_THREADS / 64];
    __shared__ uint32_t red_a[ASX_THREADS / 64];
    if (root >= 0) {
        if (threadIdx.x == 0) out[0] = root;
        return;
    }
    int32_t best = -1;
    uint32_t best_a = 0;
    for (uint32_t a0 = 0; a0 < C; a0 += ASX_THREADS) {
        const uint32_t nt = min((uint32_t)ASX_THREADS, C - a0);
        __syncthreads();                                        // the tile before this one has been read
        score[threadIdx.x] = 0;
        __syncthreads();
        // (all three loads of a pair whatever they hold, so that the loads of several pairs are in flight at a time)
        auto usable = [&](uint32_t x, uint32_t y) {
            const uint32_t i = x * C + y;
            const int64_t l = L[i];
            const int32_t r = R[i], f = F[i];
            return x != y && closure_valid(l, r) && f >= min_confirm;
        };
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < nt * C; i += ASX_THREADS) {
            const uint32_t al = i / C, b = i - al * C;
            if (usable(a0 + al, b)) atomicAdd(&score[al], 1);
        }
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < nt * C; i += ASX_THREADS) {
            const uint32_t b = i / nt, al = i - b * nt;
            if (usable(b, a0 + al)) atomicAdd(&score[al], 1);
        }
        __syncthreads();
        int32_t s = threadIdx.x < nt ? score[threadIdx.x] : -1;
        uint32_t a = a0 + threadIdx.x;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int32_t s2 = __shfl_xor(s, o);
            const uint32_t a2 = __shfl_xor(a, o);
            if (s2 > s || (s2 == s && a2 < a)) { s = s2; a = a2; }
        }
        if ((threadIdx.x & 63u) == 0) { red_s[threadIdx.x >> 6] = s; red_a[threadIdx.x >> 6] = a; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ASX_THREADS / 64; i++)              // waves and tiles in ascending order of a: strictly more wins
            if (red_s[i] > best) { best = red_s[i]; best_a = red_a[i]; }
    }
    if (threadIdx.x == 0) out[0] = (int32_t)best_a;
}

// Clip b's estimates of T_b - T_root that hold clip c (the multiset E_b of the header), each handed to fn
template <typename Fn>
__device__ __forceinline__ void closure_estimates(const int64_t *L, const int32_t *R, const int32_t *F, uint32_t C, int min_confirm,
                                                  uint32_t r, uint32_t b, uint32_t c, Fn &&fn)
{
    if (c == b) {
        if (closure_usable(L, R, F, C, min_confirm, r, b)) fn(L[r * C + b]);
    } else if (c == r) {
        if (closure_usable(L, R, F, C, min_confirm, b, r)) fn(-L[b * C + r]);
    } else {
        if (closure_usable(L, R, F, C, min_confirm, r, c) && closure_usable(L, R, F, C, min_confirm, c, b)) fn(L[r * C + c] + L[c * C + b]);
        if (closure_usable(L, R, F, C, min_confirm, b, c) && closure_usable(L, R, F, C, min_confirm, c, r)) fn(-(L[b * C + c] + L[c * C + r]));
    }
}

// Offsets, one block per clip b: the lower median of E_b by rank counting (closure_lower_median) and the number of estimates within
// tol of it.  E_b is never stored: an estimate is two lags and their flags, read again (from L2) at every step, so any C fits; a
// pool whose usable pairs agree has its estimates a few frames apart and needs a few steps.
__global__ __launch_bounds__(ASX_THREADS) void k_closure_offsets(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                                  const int32_t *__restrict__ F, uint32_t C, int64_t tol,
                                                                  int min_confirm, const int32_t *__restrict__ root,
                                                                  int64_t *__restrict__ offset, int32_t *__restrict__ support,
                                                                  int32_t *__restrict__ placed)
{
    __shared__ ClosureLds sh;
    const uint32_t b = blockIdx.x, r = (uint32_t)root[0];
    if (b == r) {
        if (threadIdx.x == 0) { offset[b] = 0; support[b] = 0; placed[b] = 1; }
        return;
    }
    auto each = [&](auto &&fn) {
        for (uint32_t c = threadIdx.x; c < C; c += ASX_THREADS) closure_estimates(L, R, F, C, min_confirm, r, b, c, fn);
    };
    int turn = 1;
    int64_t med = 0;
    const int32_t total = closure_lower_median(each, sh, turn, med);
    const int32_t sup = total > 0 ? closure_count_near(each, med, tol, sh, turn) : 0;
    if (threadIdx.x == 0) { offset[b] = med; support[b] = sup; placed[b] = total > 0 ? 1 : 0; }
}

// ---------------------------------------------------------------------------
// The curve around given lags (asx_xcorr_curve_f32_dev, asx_xcorr_pool_curve_f32_dev): behind any call, on the lags it returned,
//     r[idx] = sum_{n<N} source[(n + idx) mod 2N] * sample[n]     at idx = (p + d) mod 2N, d = -h .. h,
// the sum of k_refine_dots, for all 2h + 1 indices in ONE pass over the entry's tracks: with i0 = (p - h) mod 2N, sample n meets
// source (n + i0 + j) mod 2N for j = 0 .. 2h, a window that slides with n.
// ---------------------------------------------------------------------------
// the ret of entry e as far as curve, track and warp share it: -4 for a row outside its pool (`outside`), over -2 for a centre
// outside [-N, N-1]; 0 for an entry to compute
__device__ __forceinline__ int32_t entry_ret(const AsxLagEntries &E, size_t e, bool outside)
{
    if (outside) return -4;
    const int64_t c = E.center[e], n = (int64_t)E.N;
    return (c < -n || c > n - 1) ? -2 : 0;
}
// ... behind k_curve_resolve (pl: the pool form's records, indexed by the entry's place in the slice le, or null)
__device__ __forceinline__ int32_t entry_ret(const AsxLagEntries &E, size_t e, size_t le, const AsxPoolPair *pl)
{
    return entry_ret(E, e, pl && (pl[le].flags & ASX_POOL_INVALID));
}
// where entry e's tracks are and what its ret is
__device__ __forceinline__ int32_t curve_locate(const AsxLagEntries &E, size_t e, uint64_t &src_off, uint64_t &smp_off)
{
    const size_t pair = e / (size_t)E.entries;
    int64_t a = (int64_t)pair, b = (int64_t)pair;
    bool in = true;
    if (E.nsrc) {
        if (E.rows) { a = E.rows[2 * pair]; b = E.rows[2 * pair + 1]; }
        else { a = (int64_t)(pair / E.nsmp); b = (int64_t)(pair % E.nsmp); }
        in = a >= 0 && (uint64_t)a < E.nsrc && b >= 0 && (uint64_t)b < E.nsmp;
    }
    src_off = in ? (uint64_t)a * E.src_stride : 0u;
    smp_off = in ? (uint64_t)b * E.smp_stride : 0u;
    return entry_ret(E, e, !in);
}
// index of the entry's first value, (p - h) mod 2N, p the index of the lag c in [-N, N-1]
__device__ __forceinline__ uint32_t curve_first(int64_t c, uint32_t N, int h)
{
    const uint32_t L = 2u * N;
    const uint32_t p = c >= 0 ? (uint32_t)c : (uint32_t)((int64_t)L + c);
    return (p + L - (uint32_t)h % L) % L;
}
// an entry's results from its 2h + 1 final values y (shared memory; not read when rv != 0): r, then frac, then ret
__device__ __forceinline__ void curve_write(const AsxCurve &A, size_t e, int32_t rv, const double *y, int tid)
{
    const int h = A.E.h, n = 2 * h + 1;
    if (tid < n) A.r[e * (size_t)n + tid] = rv ? (double)NAN : y[tid];
    if (tid == 0) {
        A.frac[e] = rv ? (double)NAN : asx_parabola_frac(y[h - 1], y[h], y[h + 1]);
        A.ret[e] = rv;
    }
}

// pool form: entries first .. first + count - 1 as listed input records (what k_pool_resolve makes of a pair, without the bank)
__global__ __launch_bounds__(ASX_THREADS) void k_curve_resolve(AsxLagEntries E, size_t first, int count, AsxPoolPair *__restrict__ out)
{
    const int le = (int)(blockIdx.x * ASX_THREADS + threadIdx.x);
    if (le >= count) return;
    AsxPoolPair rec;
    const int32_t rv = curve_locate(E, first + (size_t)le, rec.src_off, rec.smp_off);
    rec.sx = rec.sy = 0u;
    rec.flags = rv == -4 ? ASX_POOL_INVALID : 0u;
    rec.pad = 0u;
    out[le] = rec;
}

// The sweep that k_curve_dots, k_track_dots and k_warp_dots share.  A block takes a range of the sample's frames in sweeps of
// ASX_CURVE_SWEEP: the sweep's stretch of the source, a few values longer and taken modulo 2N, goes through LDS once, and a thread
// forms the products of each of its four consecutive samples from a window of values it reads from there -- one pass over both
// tracks for all the sums.  float64 throughout (the products of float32 values are exact); the order is fixed: a thread's samples
// ascending, the lanes of a wave (wave_sum), the waves, and, with more than one block, the blocks in order (from `part`): an entry's
// bits depend on neither the batch nor its place in it.
#define ASX_CURVE_SWEEP (4 * ASX_THREADS)
typedef float asx_f4u __attribute__((ext_vector_type(4), aligned(4))); // four floats at any float-aligned address
// the thread's four samples y[n0 + t4 ..+ 3] of the sweep of cnt frames from n0; past the sweep's end: zeros, which meet zeros of
// the stretch
__device__ __forceinline__ asx_f4v sweep_samples(const float *y, uint64_t n0, uint32_t t4, uint32_t cnt)
{
    asx_f4v yq = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (t4 + 3u < cnt) yq = *reinterpret_cast<const asx_f4u *>(y + n0 + t4);
    else {
        if (t4 < cnt) yq.x = y[n0 + t4];
        if (t4 + 1u < cnt) yq.y = y[n0 + t4 + 1u];
        if (t4 + 2u < cnt) yq.z = y[n0 + t4 + 2u];
    }
    return yq;
}
// the stretch: xs[t] = x[(g0 + t) mod L] for t < need, zero behind, up to the LDS length LEN; 16-byte loads where the four neither
// leave `need` nor straddle the wrap.  The thread stores xs[t4 + k ASX_CURVE_SWEEP ..+ 3]; the caller's barrier follows.
template <int LEN>
__device__ __forceinline__ void sweep_fill(float *xs, const float *x, uint32_t L, uint32_t g0, uint32_t need, uint32_t t4)
{
    static_assert(LEN % 4 == 0, "the stretch is stored in fours");
    auto wrapped = [&](uint32_t i) { if (i >= L) { i -= L; if (i >= L) i %= L; } return i; };
    for (uint32_t t = t4; t < (uint32_t)LEN; t += (uint32_t)ASX_CURVE_SWEEP) {
        asx_f4v v = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (t < need) {
            const uint32_t g = wrapped(g0 + t);
            if (t + 3u < need && g + 3u < L) v = *reinterpret_cast<const asx_f4u *>(x + g);
            else {
                v.x = x[g];
                if (t + 1u < need) v.y = x[wrapped(g0 + t + 1u)];
                if (t + 2u < need) v.z = x[wrapped(g0 + t + 2u)];
                if (t + 3u < need) v.w = x[wrapped(g0 + t + 3u)];
            }
        }
        *reinterpret_cast<asx_f4v *>(xs + t) = v;
    }
}
// the sweeps of a block at a constant lag: acc[j] = sum over the frames n of [lo, hi) of x[(n + i0 + j) mod L] y[n] for j < nt, nt <=
// ASX_CURVE_N (the sums past nt hold what nobody reads).  A thread forms the nt products of each of its four samples from a window
// of 3 + nt values.  xs: ASX_CURVE_SWEEP + 2 ASX_NEAR_MAX floats of LDS; every argument but tid is block-uniform (two barriers a sweep).
__device__ __forceinline__ void sweep_dots(float *xs, const float *x, const float *y, uint32_t L, uint32_t i0, uint64_t lo, uint64_t hi,
                                           int nt, int tid, double (&acc)[ASX_CURVE_N])
{
#pragma unroll
    for (int j = 0; j < ASX_CURVE_N; j++) acc[j] = 0.0;
    for (uint64_t n0 = lo; n0 < hi; n0 += ASX_CURVE_SWEEP) {
        const uint32_t cnt = hi - n0 < (uint64_t)ASX_CURVE_SWEEP ? (uint32_t)(hi - n0) : (uint32_t)ASX_CURVE_SWEEP;
        const uint32_t t4 = 4u * (uint32_t)tid;
        const asx_f4v yq = sweep_samples(y, n0, t4, cnt);
        // xs[t] = source[(n0 + i0 + t) mod 2N] for t < cnt + nt - 1, zero behind
        sweep_fill<ASX_CURVE_SWEEP + 2 * ASX_NEAR_MAX>(xs, x, L, (uint32_t)((n0 + i0) % L), cnt + (uint32_t)nt - 1u, t4);
        __syncthreads();
        double w[4 + 2 * ASX_NEAR_MAX];
#pragma unroll
        for (int q = 0; q < (4 + 2 * ASX_NEAR_MAX) / 4; q++) {
            asx_f4v v = { 0.0f, 0.0f, 0.0f, 0.0f };
            if (4 * q < 3 + nt) v = *reinterpret_cast<const asx_f4v *>(xs + t4 + 4u * (uint32_t)q);
            w[4 * q] = (double)v.x; w[4 * q + 1] = (double)v.y; w[4 * q + 2] = (double)v.z; w[4 * q + 3] = (double)v.w;
        }
        const double y0 = (double)yq.x, y1 = (double)yq.y, y2 = (double)yq.z, y3 = (double)yq.w;
#pragma unroll
        for (int j = 0; j < ASX_CURVE_N; j++) {
            if (j < nt) {
                double a = acc[j];
                a = fma(w[j], y0, a);
                a = fma(w[j + 1], y1, a);
                a = fma(w[j + 2], y2, a);
                a = fma(w[j + 3], y3, a);
                acc[j] = a;
            }
        }
        __syncthreads();
    }
}
// the block's sums from its threads': the lanes of each wave into red[wave][j] (the caller's barrier follows), then the four waves
template <int REC>
__device__ __forceinline__ void sweep_wave_sums(const double (&acc)[ASX_CURVE_N], int nt, int tid, double (&red)[ASX_THREADS / 64][REC])
{
#pragma unroll
    for (int j = 0; j < ASX_CURVE_N; j++) {
        if (j < nt) {
            const double s = wave_sum(acc[j]);
            if ((tid & 63) == 0) red[tid >> 6][j] = s;
        }
    }
}
template <int REC> __device__ __forceinline__ double sweep_block_sum(const double (&red)[ASX_THREADS / 64][REC], int j)
{
    static_assert(ASX_THREADS / 64 == 4, "the tree below adds four waves");
    return (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}
// an entry's nb partial sums p[0], p[stride], ... in block order
__device__ __forceinline__ double sweep_blocks_sum(const double *p, unsigned nb, int stride)
{
    double s = p[0];
    for (unsigned b = 1; b < nb; b++) s += p[(size_t)b * stride];
    return s;
}

// grid (blocks per entry, entries of the slice), entry e = first + blockIdx.y: the sweep over all 2h + 1 lags.  Block x takes samples
// [x chunk, (x + 1) chunk); with more than one block per entry k_curve_sum adds the partial sums, with one the block writes the
// results itself.  Where: AsxAtPitch, indexed by the entry's pair, or AsxAtList, indexed by the entry's place in the slice
// (k_curve_resolve's records).  An entry that is not valid reads nothing.
template <class Where>
__global__ __launch_bounds__(ASX_THREADS) void k_curve_dots(const float *__restrict__ src, const float *__restrict__ smp, Where at,
                                                             AsxCurve A, size_t first, double *__restrict__ part)
{
    constexpr bool listed = std::is_same<Where, AsxAtList>::value;
    __shared__ __attribute__((aligned(16))) float xs[ASX_CURVE_SWEEP + 2 * ASX_NEAR_MAX];
    __shared__ double red[ASX_THREADS / 64][ASX_CURVE_N];
    __shared__ double yv[ASX_CURVE_N];
    const int tid = threadIdx.x, h = A.E.h, n = 2 * h + 1;
    const size_t le = blockIdx.y, e = first + le;
    const size_t rec = listed ? le : e / (size_t)A.E.entries;
    const uint32_t N = A.E.N;
    if (const int32_t rv = entry_ret(A.E, e, le, at.list())) { // (block-uniform: nobody is left at a barrier)
        if (gridDim.x == 1) curve_write(A, e, rv, yv, tid);
        return;
    }
    const float *x = src + at.src_off(rec);
    const float *y = smp + at.smp_off(rec);
    const uint32_t chunk = ((N + gridDim.x - 1) / gridDim.x + 3u) & ~3u;
    const uint64_t lo = (uint64_t)blockIdx.x * chunk;
    const uint64_t hi = lo + chunk < (uint64_t)N ? lo + chunk : (uint64_t)N;
    double acc[ASX_CURVE_N];
    sweep_dots(xs, x, y, 2u * N, curve_first(A.E.center[e], N, h), lo, hi, n, tid, acc);
    sweep_wave_sums(acc, n, tid, red);
    __syncthreads();
    if (tid < n) {
        const double v = sweep_block_sum(red, tid);
        if (gridDim.x == 1) yv[tid] = v;
        else part[(le * gridDim.x + blockIdx.x) * ASX_CURVE_N + tid] = v;
    }
    if (gridDim.x == 1) {
        __syncthreads();
        curve_write(A, e, 0, yv, tid);
    }
}

// grid (entries of the slice), one wave: an entry's nb partial sums in block order, then its results; pl: the pool form's records
__global__ __launch_bounds__(64) void k_curve_sum(AsxCurve A, size_t first, unsigned nb, const double *__restrict__ part,
                                                   const AsxPoolPair *__restrict__ pl)
{
    __shared__ double yv[ASX_CURVE_N];
    const int tid = threadIdx.x, n = 2 * A.E.h + 1;
    const size_t le = blockIdx.x, e = first + le;
    const int32_t rv = entry_ret(A.E, e, le, pl);
    if (!rv && tid < n) yv[tid] = sweep_blocks_sum(part + le * nb * ASX_CURVE_N + tid, nb, ASX_CURVE_N);
    __syncthreads();
    curve_write(A, e, rv, yv, tid);
}

// the coefficient curve: virtual pair v = e (2h + 1) + j is entry e at index (i0 + j) mod 2N -- the segment the peak search would have
// left for that lag (make_seg) and the entry's tracks as a listed input record, so that the direct Pearson kernels run on them as
// they run on a pool group
__global__ __launch_bounds__(ASX_THREADS) void k_curve_segs(AsxLagEntries E, size_t first, int count, AsxSeg *__restrict__ seg,
                                                             AsxPoolPair *__restrict__ out)
{
    const int lv = (int)(blockIdx.x * ASX_THREADS + threadIdx.x);
    if (lv >= count) return;
    const size_t v = first + (size_t)lv, n = (size_t)(2 * E.h + 1), e = v / n;
    AsxPoolPair rec;
    AsxSeg s;
    if (curve_locate(E, e, rec.src_off, rec.smp_off) == 0)
        s = make_seg((curve_first(E.center[e], E.N, E.h) + (uint32_t)(v % n)) % (2u * E.N), E.N);
    else {
        s.lag = 0; s.src_off = s.smp_off = s.len = s.peak = s.flags = 0u;
        rec.src_off = rec.smp_off = 0u;
    }
    rec.sx = rec.sy = rec.flags = rec.pad = 0u;
    seg[lv] = s;
    out[lv] = rec;
}

// ---------------------------------------------------------------------------
// The lag track (asx_xcorr_track_f32_dev, asx_xcorr_pool_track_f32_dev): the curve's sum kept apart per time segment,
//     r_s[d] = sum_{b_s <= n < b_{s+1}} source[(n + p + d) mod 2N] * sample[n],   b_s = floor(s N / S),   d = -h .. h,
// over a lag range wide enough to hold a drifting peak, and behind it each segment's peak and the weighted line through the peaks.
// ---------------------------------------------------------------------------
// the first frame of segment s
__device__ __forceinline__ uint64_t track_bound(uint32_t N, int S, int s) { return (uint64_t)s * (uint64_t)N / (uint64_t)S; }

// grid (blocks per segment and tile, segments * tiles, entries of the slice): the sweep restricted to segment s = blockIdx.y / tiles
// and to the lags d = -h + ASX_CURVE_N tile .. of tile = blockIdx.y % tiles, at most ASX_CURVE_N of them (the last tile may be
// short).  Block x takes the segment's frames [b_s + x chunk, b_s + (x + 1) chunk); a segment starts at any frame, which is why the
// sweep reads the sample with 4-byte aligned loads of four.  With more than one block k_track_sum adds the partial sums; one block
// writes its values to A.r itself.  An entry that is not valid reads and writes nothing: k_track_fit fills in all of its outputs.
template <class Where>
__global__ __launch_bounds__(ASX_THREADS) void k_track_dots(const float *__restrict__ src, const float *__restrict__ smp, Where at,
                                                             AsxTrack A, size_t first, int tiles, double *__restrict__ part)
{
    constexpr bool listed = std::is_same<Where, AsxAtList>::value;
    __shared__ __attribute__((aligned(16))) float xs[ASX_CURVE_SWEEP + 2 * ASX_NEAR_MAX];
    __shared__ double red[ASX_THREADS / 64][ASX_CURVE_N];
    const int tid = threadIdx.x, h = A.E.h, n = 2 * h + 1;
    const size_t le = blockIdx.z, e = first + le;
    const size_t rec = listed ? le : e / (size_t)A.E.entries;
    const uint32_t N = A.E.N, L = 2u * N;
    if (entry_ret(A.E, e, le, at.list())) return; // (block-uniform: nobody is left at a barrier)
    const int64_t c = A.E.center[e];
    const int sg = (int)blockIdx.y / tiles, tile = (int)blockIdx.y - sg * tiles;
    const int d0 = tile * ASX_CURVE_N, nt = n - d0 < ASX_CURVE_N ? n - d0 : ASX_CURVE_N; // the tile's first value and how many
    const uint32_t i0 = (curve_first(c, N, h) + (uint32_t)d0 % L) % L;
    const float *x = src + at.src_off(rec);
    const float *y = smp + at.smp_off(rec);
    const uint64_t b0 = track_bound(N, A.S, sg), b1 = track_bound(N, A.S, sg + 1);
    const uint32_t chunk = (((uint32_t)(b1 - b0) + gridDim.x - 1) / gridDim.x + 3u) & ~3u;
    const uint64_t lo = b0 + (uint64_t)blockIdx.x * chunk;
    const uint64_t hi = lo + chunk < b1 ? lo + chunk : b1;
    double acc[ASX_CURVE_N];
    sweep_dots(xs, x, y, L, i0, lo, hi, nt, tid, acc);
    sweep_wave_sums(acc, nt, tid, red);
    __syncthreads();
    if (tid < nt) {
        const double v = sweep_block_sum(red, tid);
        if (gridDim.x == 1) A.r[(e * (size_t)A.S + (size_t)sg) * (size_t)n + (size_t)(d0 + tid)] = v;
        else part[((le * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * ASX_CURVE_N + tid] = v;
    }
}

// grid (segments * tiles, entries of the slice), one wave: a segment's tile from its nb partial sums in block order
__global__ __launch_bounds__(64) void k_track_sum(AsxTrack A, size_t first, int tiles, unsigned nb, const double *__restrict__ part,
                                                   const AsxPoolPair *__restrict__ pl)
{
    const int tid = threadIdx.x, n = 2 * A.E.h + 1;
    const size_t le = blockIdx.y, e = first + le;
    if (entry_ret(A.E, e, le, pl)) return;
    const int sg = (int)blockIdx.x / tiles, d0 = ((int)blockIdx.x - sg * tiles) * ASX_CURVE_N;
    if (tid >= ASX_CURVE_N || d0 + tid >= n) return;
    A.r[(e * (size_t)A.S + (size_t)sg) * (size_t)n + (size_t)(d0 + tid)] =
        sweep_blocks_sum(part + (le * gridDim.x + blockIdx.x) * nb * ASX_CURVE_N + tid, nb, ASX_CURVE_N);
}

// grid (entries of the slice), one wave, behind the entry's finished r: lane s takes segment s -- its peak m_s (the largest |r_s[d]|
// scanned from d = -h upwards, strict >), off_s = m_s + frac (one add; m_s alone at an edge) and w_s = |r_s[m_s]| -- then lane 0 the
// weighted line through (t_s, off_s) of the used segments in ascending s.  An entry that is not valid gets NaN everywhere, used 0.
__global__ __launch_bounds__(64) void k_track_fit(AsxTrack A, size_t first, const AsxPoolPair *__restrict__ pl)
{
    __shared__ double ts[ASX_TRACK_SEG_MAX], offs[ASX_TRACK_SEG_MAX], ws[ASX_TRACK_SEG_MAX];
    __shared__ int use[ASX_TRACK_SEG_MAX];
    const int tid = threadIdx.x, h = A.E.h, n = 2 * h + 1, S = A.S;
    const size_t le = blockIdx.x, e = first + le;
    const int32_t rv = entry_ret(A.E, e, le, pl);
    if (rv) { // (block-uniform)
        double *r = A.r + e * (size_t)S * (size_t)n;
        for (int i = tid; i < S * n; i += 64) r[i] = (double)NAN;
        if (A.seg)
            for (int i = tid; i < 2 * S; i += 64) A.seg[e * (size_t)S * 2 + i] = (double)NAN;
        if (tid < 3) A.fit[e * 3 + tid] = (double)NAN;
        if (tid == 0) { A.used[e] = 0; A.ret[e] = rv; }
        return;
    }
    if (tid < S) {
        const double *r = A.r + (e * (size_t)S + (size_t)tid) * (size_t)n;
        int m = 0;
        double best = fabs(r[0]);
        bool finite = r[0] - r[0] == 0.0;
        for (int j = 1; j < n; j++) {
            const double v = r[j], a = fabs(v);
            if (!(v - v == 0.0)) finite = false;
            if (a > best) { best = a; m = j; }
        }
        const bool interior = m > 0 && m < n - 1;
        double off = (double)(m - h);
        if (interior) off = (double)(m - h) + asx_parabola_frac(r[m - 1], r[m], r[m + 1]);
        const double w = fabs(r[m]);
        if (A.seg) {
            A.seg[(e * (size_t)S + (size_t)tid) * 2] = off;
            A.seg[(e * (size_t)S + (size_t)tid) * 2 + 1] = w;
        }
        const uint64_t b0 = track_bound(A.E.N, S, tid), b1 = track_bound(A.E.N, S, tid + 1);
        ts[tid] = (double)(b0 + b1 - 1u) * 0.5;
        offs[tid] = off;
        ws[tid] = w;
        use[tid] = interior && finite;
    }
    __syncthreads();
    if (tid != 0) return;
    int used = 0;
    double W = 0.0, swt = 0.0, swy = 0.0;
    for (int s = 0; s < S; s++) {
        if (!use[s]) continue;
        used++;
        W += ws[s];
        swt += ws[s] * ts[s];
        swy += ws[s] * offs[s];
    }
    double drift = (double)NAN, lag0 = (double)NAN, rms = (double)NAN;
    if (used >= 2) {
        const double tbar = swt / W, ybar = swy / W;
        double Stt = 0.0, Sty = 0.0, res = 0.0;
        for (int s = 0; s < S; s++) {
            if (!use[s]) continue;
            const double dt = ts[s] - tbar;
            Stt += ws[s] * dt * dt;
            Sty += ws[s] * dt * (offs[s] - ybar);
        }
        drift = Sty / Stt;
        lag0 = ybar - drift * tbar;
        for (int s = 0; s < S; s++) {
            if (!use[s]) continue;
            const double d = offs[s] - (lag0 + drift * ts[s]);
            res += ws[s] * d * d;
        }
        rms = sqrt(res / W);
    }
    A.fit[e * 3] = drift;
    A.fit[e * 3 + 1] = lag0;
    A.fit[e * 3 + 2] = rms;
    A.used[e] = used;
    A.ret[e] = 0;
}

// ---------------------------------------------------------------------------
// The warped correlation (asx_xcorr_warp_f32_dev, asx_xcorr_pool_warp_f32_dev): the curve's sum along a drift line (a, b),
//     r[d] = sum_{n<N} source[(n + p + d + k_n) mod 2N] * sample[n],   k_n = floor((b + a n) + 0.5),   d = -h .. h,
// and the reference's Pearson coefficient of the frames that line up at d = 0: the pairs (source[u_n], sample[n]) with
// u_n = n + c + k_n inside [0, 2N).  One pass over the entry's tracks gives both.
// ---------------------------------------------------------------------------
// the most k moves across a sweep of a valid line: ASX_CURVE_SWEEP * ASX_WARP_DRIFT_MAX = 16, and one for the rounding
#define ASX_WARP_STEPS 17
#define ASX_WARP_XS ((ASX_CURVE_SWEEP + 2 * ASX_NEAR_MAX + ASX_WARP_STEPS + 3) & ~3)
// what a block of k_warp_dots leaves: its ASX_CURVE_N partial sums, then its Pearson record {n, mx, my, mxx, myy, cxy}
#define ASX_WARP_REC (ASX_CURVE_N + 6)
// k_n: the multiply, the two adds and the floor each rounded on their own (no fused multiply-add), as numpy rounds
// np.floor((b + a * n) + 0.5).  It stays a double: an integer of at most N + N / 64 + 1, so differences of shifts and frame indices
// are exact there and the sweeps need no 64-bit integer conversions.
__device__ __forceinline__ double warp_shift(double a, double b, uint32_t n)
{
    return floor(__dadd_rn(__dadd_rn(b, __dmul_rn(a, (double)n)), 0.5));
}
// the ret of entry e when it is not computed: entry_ret's, over -5 for a line that is not valid -- a or b not finite (the comparisons
// fail on NaN), |a| > ASX_WARP_DRIFT_MAX or |b| > N; 0 for an entry to compute
__device__ __forceinline__ int32_t warp_ret(const AsxWarp &A, size_t e, size_t le, const AsxPoolPair *pl)
{
    if (const int32_t rv = entry_ret(A.E, e, le, pl)) return rv;
    const double a = A.line[e * A.line_stride], b = A.line[e * A.line_stride + 1];
    return (fabs(a) <= ASX_WARP_DRIFT_MAX && fabs(b) <= (double)A.E.N) ? 0 : -5;
}

// grid (blocks per entry, entries of the slice), entry e = first + blockIdx.y: the sweep along the line.  k is monotone in
// n, so a sweep's shifts lie between those of its two ends; the sweep's stretch of the source starts at (n0 + p - h + k_min) mod 2N,
// is up to 2h + ASX_WARP_STEPS longer than the sweep and goes through LDS once.  A thread reads the window of its four frames at the
// offset k_n - k_min: one window of 4 + 2h values when the four share k, and a second one for the frames behind the step otherwise
// (four consecutive frames of a valid line hold at most one step); a frame meets the window of its own k, the others a zero.  In
// the same pass the thread keeps the Pearson statistics of its frames n with 0 <= n + c + k_n < 2N, relative to the first such pair
// it meets, as k_pearson_partial does; their source values are the window's d = 0 column.  The sweep's order, with the blocks added
// by k_warp_final; with one block per entry the sums go to A.r and the record to part[le * 6].  An entry that is not valid reads and
// writes nothing: k_warp_final fills in all of its outputs.
template <class Where>
__global__ __launch_bounds__(ASX_THREADS, 4) void k_warp_dots(const float *__restrict__ src, const float *__restrict__ smp, Where at,
                                                            AsxWarp A, size_t first, double *__restrict__ part)
{
    constexpr bool listed = std::is_same<Where, AsxAtList>::value;
    __shared__ __attribute__((aligned(16))) float xs[ASX_WARP_XS];
    __shared__ double red[ASX_THREADS / 64][ASX_WARP_REC];
    const int tid = threadIdx.x, h = A.E.h, n = 2 * h + 1;
    const size_t le = blockIdx.y, e = first + le;
    const size_t rec = listed ? le : e / (size_t)A.E.entries;
    const uint32_t N = A.E.N, L = 2u * N;
    if (warp_ret(A, e, le, at.list())) return; // (block-uniform: nobody is left at a barrier)
    const int64_t c = A.E.center[e];
    const double la = A.line[e * A.line_stride], lb = A.line[e * A.line_stride + 1];
    const uint32_t i0 = curve_first(c, N, h);
    const float *x = src + at.src_off(rec);
    const float *y = smp + at.smp_off(rec);
    const uint32_t chunk = ((N + gridDim.x - 1) / gridDim.x + 3u) & ~3u;
    const uint64_t lo64 = (uint64_t)blockIdx.x * chunk;
    const uint32_t lo = lo64 < (uint64_t)N ? (uint32_t)lo64 : N, hi = N - lo < chunk ? N : lo + chunk; // (2N fits 32 bits)
    double acc[ASX_CURVE_N];
#pragma unroll
    for (int j = 0; j < ASX_CURVE_N; j++) acc[j] = 0.0;
    double px = 0, py = 0, sx = 0, sy = 0, sxy = 0, sxx = 0, syy = 0; // pivots: the first lined-up pair this thread meets
    uint32_t seen = 0;
    auto add = [&](double u, double v) {
        if (!seen) { px = u; py = v; }
        const double da = u - px, db = v - py;
        sx += da;
        sy += db;
        sxy += da * db;
        sxx += da * da;
        syy += db * db;
        seen++;
    };
    for (uint32_t n0 = lo; n0 < hi; n0 += ASX_CURVE_SWEEP) {
        const uint32_t cnt = hi - n0 < (uint32_t)ASX_CURVE_SWEEP ? hi - n0 : (uint32_t)ASX_CURVE_SWEEP;
        const uint32_t t4 = 4u * (uint32_t)tid;
        const asx_f4v yq = sweep_samples(y, n0, t4, cnt);
        // the shifts of the sweep's ends and of the thread's frames (a frame past the sweep's end takes the last one's: its offset
        // stays inside the stretch)
        const uint32_t last = n0 + cnt - 1u;
        const double ka = warp_shift(la, lb, n0), kb = warp_shift(la, lb, last), kmin = ka < kb ? ka : kb;
        const int64_t km = (int64_t)kmin, u0 = (int64_t)n0 + c + km; // u_n = u0 + (n - n0) + (k_n - kmin)
        // per frame: its offset into the stretch, whether it shares the first frame's shift, and whether it lines up at d = 0 -- inside
        // the block's frames and 0 <= u_n < 2N
        uint32_t o0 = 0u, o3 = 0u;
        unsigned same = 0u, in = 0u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t nq = n0 + t4 + (uint32_t)q < last ? n0 + t4 + (uint32_t)q : last;
            const double k = warp_shift(la, lb, nq);
            const uint32_t o = (uint32_t)(int)(k - kmin);
            if (q == 0) o0 = o;
            o3 = o;
            if (o == o0) same |= 1u << q;
            if (t4 + (uint32_t)q < cnt && (uint64_t)(u0 + (int64_t)(t4 + (uint32_t)q + o)) < (uint64_t)L) in |= 1u << q;
        }
        // xs[t] = source[(n0 + i0 + kmin + t) mod 2N] for t < cnt + 2h + (kmax - kmin), zero behind.  n0 + i0 < 3N and |kmin| < 2N:
        // two subtractions bring the index home
        uint64_t gi = (uint64_t)n0 + i0;
        if (gi >= L) gi -= L;
        gi = (uint64_t)((int64_t)gi + km + (int64_t)L);
        if (gi >= L) gi -= L;
        if (gi >= L) gi -= L;
        const uint32_t g0 = (uint32_t)gi;
        const uint32_t need = cnt + 2u * (uint32_t)h + (uint32_t)(int)((ka < kb ? kb : ka) - kmin);
        sweep_fill<ASX_WARP_XS>(xs, x, L, g0, need, t4);
        __syncthreads();
        // the frames of `take` against the window at offset o (any float: 4-byte aligned reads), one window value at a time: value i
        // meets frame q at the sum j = i - q, so every sum takes its frames in ascending order
        auto window = [&](uint32_t o, unsigned take) __attribute__((always_inline)) {
            const float *wp = xs + t4 + o;
            const double y0 = (take & 1u) ? (double)yq.x : 0.0, y1 = (take & 2u) ? (double)yq.y : 0.0;
            const double y2 = (take & 4u) ? (double)yq.z : 0.0, y3 = (take & 8u) ? (double)yq.w : 0.0;
            { // the statistics first: their four values are gone before the sums take the registers
                const asx_f4v xc = *reinterpret_cast<const asx_f4u *>(wp + h); // the d = 0 column: source[u_n] of the four frames
                const unsigned st = take & in;
                if (st & 1u) add((double)xc.x, y0);
                if (st & 2u) add((double)xc.y, y1);
                if (st & 4u) add((double)xc.z, y2);
                if (st & 8u) add((double)xc.w, y3);
            }
#pragma unroll
            for (int q = 0; q < (4 + 2 * ASX_NEAR_MAX) / 4; q++) {
                if (4 * q >= 4 + 2 * h) break; // (block-uniform) the window ends: the sums past 2h + 1 hold what nobody reads
                const asx_f4v v = *reinterpret_cast<const asx_f4u *>(wp + 4 * q);
                const float f[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = 4 * q + u;
                    const double w = (double)f[u];
                    if (i < ASX_CURVE_N) acc[i] = fma(w, y0, acc[i]);
                    if (i >= 1 && i - 1 < ASX_CURVE_N) acc[i - 1] = fma(w, y1, acc[i - 1]);
                    if (i >= 2 && i - 2 < ASX_CURVE_N) acc[i - 2] = fma(w, y2, acc[i - 2]);
                    if (i >= 3 && i - 3 < ASX_CURVE_N) acc[i - 3] = fma(w, y3, acc[i - 3]);
                }
            }
        };
        window(o0, same);
        if (same != 15u) window(o3, 15u & ~same);
        __syncthreads();
    }
    sweep_wave_sums(acc, n, tid, red);
    PStat v;
    v.n = (double)seen;
    v.mx = v.my = v.mxx = v.myy = v.cxy = 0.0;
    if (seen) {
        v.mx = px + sx / v.n;
        v.my = py + sy / v.n;
        v.mxx = sxx - sx * sx / v.n;
        v.myy = syy - sy * sy / v.n;
        v.cxy = sxy - sx * sy / v.n;
    }
    v = pstat_wave_merge(v);
    if ((tid & 63) == 0) {
        double *o = &red[tid >> 6][ASX_CURVE_N];
        o[0] = v.n; o[1] = v.mx; o[2] = v.my; o[3] = v.mxx; o[4] = v.myy; o[5] = v.cxy;
    }
    __syncthreads();
    double *out = part + (le * gridDim.x + blockIdx.x) * ASX_WARP_REC;
    if (tid < n) {
        const double s = sweep_block_sum(red, tid);
        if (gridDim.x == 1) A.r[e * (size_t)n + (size_t)tid] = s;
        else out[tid] = s;
    }
    if (tid == 64) { // (a lane of the second wave: the first one's hold the sums) the waves' records in order
        for (int w = 0; w < ASX_THREADS / 64; w++) {
            const double *p = &red[w][ASX_CURVE_N];
            PStat o;
            o.n = p[0]; o.mx = p[1]; o.my = p[2]; o.mxx = p[3]; o.myy = p[4]; o.cxy = p[5];
            v = w ? pstat_merge(v, o) : o;
        }
        double *st = gridDim.x == 1 ? part + le * 6 : out + ASX_CURVE_N;
        st[0] = v.n; st[1] = v.mx; st[2] = v.my; st[3] = v.mxx; st[4] = v.myy; st[5] = v.cxy;
    }
}

// grid (entries of the slice), one wave per entry, behind k_warp_dots: the entry's nb partial sums in block order (nb == 1: they are
// in A.r already), then frac; its nb Pearson records merged as k_pearson_final merges them -- lane b owns the blocks b, b + 64, ... --
// then coef, len = the records' count and ret (-1 for a NaN coefficient).  An entry that is not valid gets NaN everywhere, len 0.
__global__ __launch_bounds__(64) void k_warp_final(AsxWarp A, size_t first, unsigned nb, const double *__restrict__ part,
                                                    const AsxPoolPair *__restrict__ pl)
{
    __shared__ double yv[ASX_CURVE_N];
    const int tid = threadIdx.x, h = A.E.h, n = 2 * h + 1;
    const size_t le = blockIdx.x, e = first + le;
    const int32_t rv = warp_ret(A, e, le, pl);
    if (rv) { // (block-uniform)
        if (tid < n) A.r[e * (size_t)n + (size_t)tid] = (double)NAN;
        if (tid == 0) {
            A.frac[e] = (double)NAN;
            A.coef[e] = (double)NAN;
            if (A.len) A.len[e] = 0;
            A.ret[e] = rv;
        }
        return;
    }
    if (tid < n) {
        double s;
        if (nb == 1u) s = A.r[e * (size_t)n + (size_t)tid];
        else {
            s = sweep_blocks_sum(part + le * nb * ASX_WARP_REC + tid, nb, ASX_WARP_REC);
            A.r[e * (size_t)n + (size_t)tid] = s;
        }
        yv[tid] = s;
    }
    PStat v;
    v.n = v.mx = v.my = v.mxx = v.myy = v.cxy = 0.0;
    for (unsigned b = (unsigned)tid; b < nb; b += 64u) {
        const double *p = nb == 1u ? part + le * 6 : part + (le * nb + b) * ASX_WARP_REC + ASX_CURVE_N;
        PStat o;
        o.n = p[0]; o.mx = p[1]; o.my = p[2]; o.mxx = p[3]; o.myy = p[4]; o.cxy = p[5];
        v = pstat_merge(v, o);
    }
    v = pstat_wave_merge(v);
    __syncthreads();
    if (tid == 0) {
        // src/cross_correlation.c:115; no lined-up frame or a constant side gives 0/0 = NaN like the reference
        const double cf = v.cxy / sqrt(v.mxx * v.myy);
        A.frac[e] = asx_parabola_frac(yv[h - 1], yv[h], yv[h + 1]);
        A.coef[e] = cf;
        if (A.len) A.len[e] = (int64_t)v.n;
        A.ret[e] = (cf != cf) ? -1 : 0;
    }
}

// ---------------------------------------------------------------------------
// second look, DC removal (second_look, asx_api.hip): one pair, one block each.  An offset of hundreds of standard deviations
// in BOTH tracks makes the float32 error bound (proportional to |source|_2 |sample|_2) wider than the whole range of
// r, every lag a near-tie.  r'[k] = sum (source[n+k] - m) sample[n] = r[k] - m * sum(sample) for ANY constant m: the
// transforms then run on a zero-mean source, whose norm no longer carries the offset, and the constant goes back in
// when the keys are formed (peak_key_shifted).  The reference needs none of this: float64 (src/cross_correlation.c:34).
// ---------------------------------------------------------------------------
// grid (ASX_DC_BLOCKS): per-block sums of the source (2N) and the sample (N) in float64, 16-byte loads; the last
// kernel (one wave) adds the partials in block order -- a fixed tree, the same for every call
#define ASX_DC_BLOCKS 128
template <typename TIn>
__global__ __launch_bounds__(ASX_THREADS) void k_dc_partial(const TIn *__restrict__ src, const TIn *__restrict__ smp, uint32_t N,
                                                             double *__restrict__ part)
{
    __shared__ double red[2][ASX_THREADS / 64];
    typedef TIn vec4u __attribute__((ext_vector_type(4), aligned(sizeof(TIn))));
    double a = 0.0, b = 0.0;
    const size_t stride = (size_t)gridDim.x * ASX_THREADS * 4, first = ((size_t)blockIdx.x * ASX_THREADS + threadIdx.x) * 4;
    const size_t n2 = 2 * (size_t)N;
    for (size_t i = first; i < n2; i += stride) {
        if (i + 3 < n2) { const vec4u v = *reinterpret_cast<const vec4u *>(src + i); a += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }
        else for (size_t k = i; k < n2; k++) a += (double)src[k];
    }
    for (size_t i = first; i < N; i += stride) {
        if (i + 3 < N) { const vec4u v = *reinterpret_cast<const vec4u *>(smp + i); b += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }
        else for (size_t k = i; k < N; k++) b += (double)smp[k];
    }
    a = wave_sum(a); b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ASX_THREADS / 64; w++) { a += red[0][w]; b += red[1][w]; }
        part[2 * blockIdx.x] = a; part[2 * blockIdx.x + 1] = b;
    }
}
__global__ __launch_bounds__(64) void k_dc_final(const double *__restrict__ part, uint32_t N, double scale, double *__restrict__ stats)
{
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < ASX_DC_BLOCKS; i += 64) { a += part[2 * i]; b += part[2 * i + 1]; }
    a = wave_sum(a); b = wave_sum(b);
    if (threadIdx.x == 0) {
        const double mean = a / (2.0 * (double)N);
        // the device's r is the unnormalised inverse transform, F times the plain sum of products (asx_api.hip,
        // bound_scale): the constant that goes back into the keys carries the same factor
        stats[0] = mean; stats[1] = b; stats[2] = mean * b * scale;
    }
}
template <typename TIn>
__global__ __launch_bounds__(ASX_THREADS) void k_dc_apply(const TIn *__restrict__ src, uint32_t N, const double *__restrict__ stats,
                                                           float *__restrict__ out)
{
    const double mean = stats[0];
    for (size_t i = (size_t)blockIdx.x * ASX_THREADS + threadIdx.x; i < 2 * (size_t)N; i += (size_t)gridDim.x * ASX_THREADS)
        out[i] = (float)((double)src[i] - mean);
}

// ---------------------------------------------------------------------------
// double -> float conversion of the reference's f64 buffers
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ASX_THREADS) void k_cvt_f64_f32(const double *__restrict__ in,
                                                              float *__restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * ASX_THREADS + threadIdx.x; i < n;
         i += (size_t)gridDim.x * ASX_THREADS)
        out[i] = (float)in[i];
}

// ---------------------------------------------------------------------------
// synthetic pairs: bit-identical to oracle_synth_pair (oracle/xcorr_oracle.c)
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ uint64_t stream_key(uint64_t seed, uint64_t pair, uint64_t stream)
{
    return mix64(mix64(seed) + 0x632BE59BD9B4E019ull * (pair + 1) + stream);
}
__device__ __forceinline__ float u24(uint64_t h)
{
    const int32_t v = (int32_t)(h >> 40) - (1 << 23);
    return (float)v * (1.0f / 8388608.0f);
}
__device__ __forceinline__ float z22(uint64_t key, uint64_t n)
{
    const uint64_t h1 = mix64(key + 2 * n), h2 = mix64(key + 2 * n + 1);
    const int32_t a = (int32_t)(h1 >> 42), b = (int32_t)((h1 >> 20) & 0x3FFFFF);
    const int32_t c = (int32_t)(h2 >> 42), d = (int32_t)((h2 >> 20) & 0x3FFFFF);
    const int32_t v = a + b + c + d - (1 << 23);
    return (float)v * (1.0f / 4194304.0f);
}

__global__ __launch_bounds__(ASX_THREADS) void k_synth(uint64_t seed, uint64_t first_pair, uint32_t N,
                                                        float amp, float *__restrict__ src,
                                                        float *__restrict__ smp,
                                                        int64_t *__restrict__ true_lag)
{
    const uint64_t pair = first_pair + blockIdx.y;
    const uint64_t ks = stream_key(seed, pair, 1), kn = stream_key(seed, pair, 2);
    const uint64_t kl = stream_key(seed, pair, 3);
    const int64_t span = (int64_t)(3ull * N / 4);
    const int64_t lag = (int64_t)(mix64(kl) % (uint64_t)(2 * span + 1)) - span;
    float *s = src + (size_t)blockIdx.y * 2 * N;
    float *t = smp + (size_t)blockIdx.y * N;
    for (uint32_t i = blockIdx.x * ASX_THREADS + threadIdx.x; i < 2u * N; i += gridDim.x * ASX_THREADS) {
        s[i] = u24(mix64(ks + N + i));
        if (i < N) {
            const float sig = 0.5f * u24(mix64(ks + (uint64_t)((int64_t)N + (int64_t)i + lag)));
            t[i] = __fadd_rn(sig, __fmul_rn(amp, z22(kn, i)));
        }
    }
    if (true_lag && blockIdx.x == 0 && threadIdx.x == 0) true_lag[blockIdx.y] = lag;
}

#endif // ASX_HAS_PART(64)

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
static size_t lds_bytes_cols(const AsxDev &P) { return (size_t)P.M1 * P.T * sizeof(float2); }
static size_t lds_bytes_rows(const AsxDev &P) { return (size_t)4 * P.M2 * sizeof(float2); }

static int max_radix(const AsxStages &st)
{
    int m = 2;
    for (int i = 0; i < st.nstages; i++) m = st.radix[i] > m ? st.radix[i] : m;
    return m;
}

// Every packed transform pass has its launcher in the part of the build that holds the compiled-in schedules (AsxPCols / AsxPRows,
// kernel_table.h): it looks the plan's entry up there, and hands a plan without one (-1) to the run-time-schedule kernels, which
// are a part of their own (*_any: they take any plan).
void asx_launch_fwd_cols_any(const AsxDev &P, const float *src, const float *smp, float2 *zxa, float2 *zya, const AsxPeakWs &W,
                             int npairs, hipStream_t s);
void asx_launch_rows_any(const AsxDev &P, const float2 *zxa, const float2 *zya, float2 *ga, const AsxPeakWs &W, int npairs,
                         hipStream_t s);
void asx_launch_inv_cols_any(const AsxDev &P, const float2 *ga, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                             const AsxSearch &q);

template <class K>
static void launch_fwd(K kernel, const AsxDev &P, int npairs, hipStream_t s, const float *src, const float *smp, float2 *zxa,
                       float2 *zya, const AsxPeakWs &W)
{
    allow_big_lds((const void *)kernel, lds_bytes_cols(P));
    hipLaunchKernelGGL(kernel, dim3(col_grid_x(P.ntiles, P.logT), 2, npairs), dim3(P.threads_cols), lds_bytes_cols(P), s, P.self_dev,
                       src, smp, zxa, zya, W.nrm_part);
}
#if ASX_HAS_PART(1)
void asx_launch_fwd_cols(const AsxDev &P, const float *src, const float *smp, float2 *zxa, float2 *zya, const AsxPeakWs &W,
                         int npairs, hipStream_t s)
{
    if (!asx_with_entry(AsxPCols{}, P.kcols, [&](auto e) {
            launch_fwd(k_fwd_cols<e.maxr, typename decltype(e)::sched, e.t, e.nt>, P, npairs, s, src, smp, zxa, zya, W);
        }))
        asx_launch_fwd_cols_any(P, src, smp, zxa, zya, W, npairs, s);
}
#endif
#if ASX_HAS_PART(2)
void asx_launch_fwd_cols_any(const AsxDev &P, const float *src, const float *smp, float2 *zxa, float2 *zya, const AsxPeakWs &W,
                             int npairs, hipStream_t s)
{
    const int mr = max_radix(P.st1);
    if (mr <= 10) launch_fwd(k_fwd_cols<10>, P, npairs, s, src, smp, zxa, zya, W);
    else if (mr <= 12) launch_fwd(k_fwd_cols<12>, P, npairs, s, src, smp, zxa, zya, W);
    else launch_fwd(k_fwd_cols<16>, P, npairs, s, src, smp, zxa, zya, W);
}
#endif

// one task (pair, k1) per block
template <class K>
static void launch_rows(K kernel, const AsxDev &P, int npairs, hipStream_t s, const float2 *zxa, const float2 *zya, float2 *ga,
                        const AsxPeakWs &W)
{
    size_t lds = lds_bytes_rows(P);
    // diagnostic: a larger request caps the blocks per CU (occupancy sweep, tools/README.md)
    if (const char *e = getenv("ASX_DBG_ROWS_LDS")) lds = std::max(lds, (size_t)atol(e));
    allow_big_lds((const void *)kernel, lds);
    hipLaunchKernelGGL(kernel, dim3((P.M1 / 2 + 1) * npairs), dim3(P.threads_rows), lds, s, P.self_dev, zxa, zya, ga, P.row_tasks, P.M1,
                       P.M2, P.M, W);
}
#if ASX_HAS_PART(4)
void asx_launch_rows(const AsxDev &P, float2 *zxa, float2 *zya, float2 *ga, const AsxPeakWs &W, int npairs, hipStream_t s)
{
    if (!asx_with_entry(AsxPRows{}, P.krows, [&](auto e) {
            launch_rows(k_rows<e.maxr, typename decltype(e)::sched, e.nt>, P, npairs, s, zxa, zya, ga, W);
        }))
        asx_launch_rows_any(P, zxa, zya, ga, W, npairs, s);
}
#endif
#if ASX_HAS_PART(8)
void asx_launch_rows_any(const AsxDev &P, const float2 *zxa, const float2 *zya, float2 *ga, const AsxPeakWs &W, int npairs,
                         hipStream_t s)
{
    const int mr = max_radix(P.st2);
    if (mr <= 10) launch_rows(k_rows<10>, P, npairs, s, zxa, zya, ga, W);
    else if (mr <= 12) launch_rows(k_rows<12>, P, npairs, s, zxa, zya, ga, W);
    else launch_rows(k_rows<16>, P, npairs, s, zxa, zya, ga, W);
}
#endif

// one instance of the inverse column kernel with its selection
template <class K, class Sel>
static void launch_inv(K kernel, const AsxDev &P, int npairs, hipStream_t s, const float2 *ga, const AsxPeakWs &W, float *r_out, Sel sel)
{
    allow_big_lds((const void *)kernel, lds_bytes_cols(P));
    hipLaunchKernelGGL(kernel, dim3(col_grid_x(P.ntiles, P.logT), npairs), dim3(P.threads_cols), lds_bytes_cols(P), s, P.self_dev, ga,
                       W, r_out, sel);
}
// q: which flavour runs (one zone capacity in the packed kernels' top-k form, whatever q.tk_zones says)
#if ASX_HAS_PART(16)
void asx_launch_inv_cols(const AsxDev &P, const float2 *ga, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                         const AsxSearch &q)
{
    if (!asx_with_entry(AsxPCols{}, P.kcols, [&](auto e) {
            asx_with_selection<ASX_TOPK_MAX - 1>(q, [&](auto sel) {
                launch_inv(k_inv_cols<e.maxr, typename decltype(e)::sched, e.t, e.nt, decltype(sel)>, P, npairs, s, ga, W, r_out, sel);
            });
        }))
        asx_launch_inv_cols_any(P, ga, W, r_out, npairs, s, q);
}
#endif
#if ASX_HAS_PART(32)
void asx_launch_inv_cols_any(const AsxDev &P, const float2 *ga, const AsxPeakWs &W, float *r_out, int npairs, hipStream_t s,
                             const AsxSearch &q)
{
    const int mr = max_radix(P.st1);
    asx_with_selection<ASX_TOPK_MAX - 1>(q, [&](auto sel) {
        using Sel = decltype(sel);
        if (mr <= 10) launch_inv(k_inv_cols<10, void, 0, 0, Sel>, P, npairs, s, ga, W, r_out, sel);
        else if (mr <= 12) launch_inv(k_inv_cols<12, void, 0, 0, Sel>, P, npairs, s, ga, W, r_out, sel);
        else launch_inv(k_inv_cols<16, void, 0, 0, Sel>, P, npairs, s, ga, W, r_out, sel);
    });
}
#endif

#if ASX_HAS_PART(64)
void asx_launch_finalize(const AsxDev &P, const AsxPeakWs &W, AsxSeg *seg, int npairs, hipStream_t s, uint32_t pair_base,
                         const AsxSearch &q)
{
    const dim3 grid(npairs), block(ASX_THREADS);
    asx_with_selection(q, [&](auto sel) {
        if constexpr (std::is_same<decltype(sel), AsxSelTopkSeed>::value)
            hipLaunchKernelGGL((k_finalize<AsxSelTopkSeed, unsigned long long>), grid, block, 0, s, P.self_dev, W, seg, pair_base, sel, q.tk_sink);
        else
            hipLaunchKernelGGL(k_finalize<decltype(sel)>, grid, block, 0, s, P.self_dev, W, seg, pair_base, sel);
    });
}

void asx_launch_topk_step(AsxTopkWs T, const AsxSeg *seg, const AsxPeakWs &W, const AsxSearch &call, uint32_t N, int npairs, int j,
                          int k, int64_t sep, int64_t *lag, double *coef, int32_t *ret, hipStream_t s)
{
    hipLaunchKernelGGL(k_topk_step, dim3((npairs + ASX_THREADS - 1) / ASX_THREADS), dim3(ASX_THREADS), 0, s, T, seg, W, call.lo, call.hi,
                       call.rows, N, npairs, j, k, sep, lag, coef, ret);
}

void asx_launch_topk_peak(const AsxTopkWs &T, const AsxPeakWs &W, const AsxSearch &call, uint32_t N, int npairs, int j, int k, double f,
                          double *peak, hipStream_t s)
{
    hipLaunchKernelGGL(k_topk_peak, dim3((npairs + ASX_THREADS - 1) / ASX_THREADS), dim3(ASX_THREADS), 0, s, T.pairs, W.pairmax, call.rows,
                       N, npairs, j, k, f, peak);
}

void asx_launch_invalid_pairs(const AsxPoolPair *pl, int64_t *lag, double *coef, int32_t *ret, double *peak, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_invalid_pairs, dim3((npairs + ASX_THREADS - 1) / ASX_THREADS), dim3(ASX_THREADS), 0, s, pl, npairs, lag, coef, ret,
                       peak);
}

void asx_launch_invalid_pairs_k(const AsxPoolPair *pl, int k, int64_t *lag, double *coef, int32_t *ret, double *peak, int npairs,
                                hipStream_t s)
{
    const dim3 grid((npairs + ASX_THREADS - 1) / ASX_THREADS), block(ASX_THREADS);
    if (peak) hipLaunchKernelGGL(k_invalid_pairs_kp, grid, block, 0, s, pl, npairs, k, lag, coef, ret, peak);
    else hipLaunchKernelGGL(k_invalid_pairs_k, grid, block, 0, s, pl, npairs, k, lag, coef, ret);
}

void asx_launch_invalid_rows(const AsxWinRows &rows, uint32_t N, int64_t *lag, double *coef, int32_t *ret, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_invalid_rows, dim3((npairs + ASX_THREADS - 1) / ASX_THREADS), dim3(ASX_THREADS), 0, s, rows, N, npairs, lag,
                       coef, ret);
}

template <typename TIn>
void asx_launch_refine(const AsxDev &P, const AsxInputs<TIn> &in, const AsxPeakWs &W, AsxSeg *seg, int npairs, hipStream_t s,
                       int dot_blocks, bool pick, const AsxSearch &q)
{
    asx_with_inputs(in, [&](auto at) {
        hipLaunchKernelGGL((k_refine_dots<TIn, decltype(at)>), dim3(dot_blocks, npairs), dim3(ASX_THREADS), 0, s, P.self_dev, in.src,
                           in.smp, at, W);
    });
    if (!pick) return;
    const dim3 grid(npairs), block(ASX_THREADS);
    asx_with_selection(q, [&](auto sel) {
        hipLaunchKernelGGL(k_refine_pick<decltype(sel)>, grid, block, 0, s, P.self_dev, W, seg, sel);
    });
}

// Partial blocks per pair: a function of the segment's BASIS LENGTH ONLY -- one block per 16 sweeps of 256 threads x 4
// elements (a block that only makes two sweeps pays more for its reduction than for its loads: 1024 pairs of
// N = 144 000 ran at 3.0 TB/s with 64 blocks per pair against 5.7 TB/s at N = 1 440 000), at most
// ASX_PEARSON_BLOCKS_MAX.  The chunks a pair is cut into, the pivots and the merge tree -- and so the last bits of its
// coefficient -- are therefore the same whatever the batch it travels in, alone through cross_correlation(), in a group
// of 124, re-run by the second look or on another shard (round 3 derived the count from the launch size).
unsigned asx_pearson_blocks(uint32_t basis_len)
{
    const uint32_t per_block = 16u * 4u * ASX_THREADS;
    uint32_t nb = (basis_len + per_block - 1) / per_block;
    if (nb > ASX_PEARSON_BLOCKS_MAX) nb = ASX_PEARSON_BLOCKS_MAX;
    if (nb < 1) nb = 1;
    return nb;
}

// k_pearson_partial: SPEC = false with an empty S (the direct form), true with the spectral form's
template <typename TIn, bool SPEC>
static void launch_pearson_partial(const AsxInputs<TIn> &in, uint32_t basis_len, const AsxSeg *seg, const AsxSpecWs &S, double *psums,
                                   int npairs, hipStream_t s)
{
    const dim3 grid(asx_pearson_blocks(basis_len), npairs), block(ASX_THREADS);
    asx_with_inputs(in, [&](auto at) {
        hipLaunchKernelGGL((k_pearson_partial<TIn, SPEC, decltype(at)>), grid, block, 0, s, in.src, in.smp, at, basis_len, seg, psums, S);
    });
}

template <typename TIn>
void asx_launch_pearson(const AsxInputs<TIn> &in, uint32_t basis_len, const AsxSeg *seg, double *psums, int64_t *lag, double *coef,
                        int32_t *ret, int npairs, hipStream_t s)
{
    launch_pearson_partial<TIn, false>(in, basis_len, seg, AsxSpecWs{}, psums, npairs, s);
    hipLaunchKernelGGL(k_pearson_final, dim3(npairs), dim3(64), 0, s, seg, psums, asx_pearson_blocks(basis_len), lag, coef, ret);
}

void asx_launch_pearson_partial_spec_f32(const AsxInputs<float> &in, uint32_t basis_len, const AsxSeg *seg, const AsxSpecWs &S,
                                         double *psums, int npairs, hipStream_t s)
{
    launch_pearson_partial<float, true>(in, basis_len, seg, S, psums, npairs, s);
}

void asx_launch_results_to_ms(const int64_t *lag, const double *coef, const int32_t *ret, size_t batch,
                              double min_confidence, double sample_rate, int64_t *lag_ms, int32_t *accept,
                              hipStream_t s)
{
    if (batch == 0) return;
    const unsigned blocks = (unsigned)((batch + ASX_THREADS - 1) / ASX_THREADS);
    hipLaunchKernelGGL(k_results_to_ms, dim3(blocks), dim3(ASX_THREADS), 0, s, lag, coef, ret, batch, min_confidence,
                       1000.0 / sample_rate, lag_ms, accept);
}

void asx_launch_topk_best(const int64_t *lag, const double *coef, const int32_t *ret, size_t batch, int k, int64_t *best_lag,
                          double *best_coef, int32_t *best_ret, int32_t *best_entry, hipStream_t s)
{
    if (batch == 0) return;
    const unsigned blocks = (unsigned)((batch + ASX_THREADS - 1) / ASX_THREADS);
    hipLaunchKernelGGL(k_topk_best, dim3(blocks), dim3(ASX_THREADS), 0, s, lag, coef, ret, batch, k, best_lag, best_coef, best_ret,
                       best_entry);
}

void asx_launch_pool_closure(const int64_t *lag, const double *coef, const int32_t *ret, uint32_t C, int k, int64_t tol,
                             int min_confirm, int root, int32_t *votes, int64_t *best_lag, double *best_coef, int32_t *best_ret,
                             int32_t *best_entry, int32_t *confirm, int32_t *d_root, int64_t *offset, int32_t *support,
                             int32_t *placed, hipStream_t s)
{
    const dim3 block(ASX_THREADS);
    hipLaunchKernelGGL(k_closure_votes, dim3((C + ASX_CLOSURE_BT - 1) / ASX_CLOSURE_BT, C), block, 0, s, lag, coef, ret, C, k, tol,
                       votes, best_lag, best_coef, best_ret, best_entry);
    const uint32_t per = ASX_THREADS / 64;
    hipLaunchKernelGGL(k_closure_confirm, dim3((C * C + per - 1) / per), block, 0, s, (const int64_t *)best_lag,
                       (const int32_t *)best_ret, C, tol, confirm);
    hipLaunchKernelGGL(k_closure_root, dim3(1), block, 0, s, (const int64_t *)best_lag, (const int32_t *)best_ret,
                       (const int32_t *)confirm, C, min_confirm, root, d_root);
    hipLaunchKernelGGL(k_closure_offsets, dim3(C), block, 0, s, (const int64_t *)best_lag, (const int32_t *)best_ret,
                       (const int32_t *)confirm, C, tol, min_confirm, (const int32_t *)d_root, offset, support, placed);
}

unsigned asx_curve_blocks(uint32_t N)
{
    const unsigned nb = asx_pearson_blocks(N) * 6u / (unsigned)ASX_CURVE_N;
    return nb < 1u ? 1u : nb;
}

void asx_launch_curve_r(const float *src, const float *smp, const AsxCurve &A, size_t first, int count, AsxPoolPair *pl, double *part,
                        hipStream_t s)
{
    const unsigned nb = asx_curve_blocks(A.E.N);
    const dim3 grid(nb, (unsigned)count), block(ASX_THREADS);
    if (A.E.nsrc) {
        hipLaunchKernelGGL(k_curve_resolve, dim3(((unsigned)count + ASX_THREADS - 1) / ASX_THREADS), block, 0, s, A.E, first, count, pl);
        hipLaunchKernelGGL(k_curve_dots<AsxAtList>, grid, block, 0, s, src, smp, AsxAtList{ pl }, A, first, part);
    } else {
        hipLaunchKernelGGL(k_curve_dots<AsxAtPitch>, grid, block, 0, s, src, smp, AsxAtPitch{ (size_t)A.E.src_stride, (size_t)A.E.smp_stride },
                           A, first, part);
    }
    if (nb > 1u)
        hipLaunchKernelGGL(k_curve_sum, dim3((unsigned)count), dim3(64), 0, s, A, first, nb, (const double *)part,
                           (const AsxPoolPair *)(A.E.nsrc ? pl : nullptr));
}

void asx_launch_curve_segs(const AsxLagEntries &E, size_t first, int count, AsxSeg *seg, AsxPoolPair *pl, hipStream_t s)
{
    hipLaunchKernelGGL(k_curve_segs, dim3(((unsigned)count + ASX_THREADS - 1) / ASX_THREADS), dim3(ASX_THREADS), 0, s, E, first, count,
                       seg, pl);
}

unsigned asx_track_blocks(uint32_t N, int segments, int half_width)
{
    const unsigned tiles = (2u * (unsigned)half_width + ASX_CURVE_N) / (unsigned)ASX_CURVE_N;
    const unsigned nb = asx_curve_blocks(N) / ((unsigned)segments * tiles);
    return nb < 1u ? 1u : nb;
}

void asx_launch_track(const float *src, const float *smp, const AsxTrack &A, size_t first, int count, AsxPoolPair *pl, double *part,
                      hipStream_t s)
{
    const int tiles = (2 * A.E.h + ASX_CURVE_N) / ASX_CURVE_N; // ceil((2h + 1) / ASX_CURVE_N)
    const unsigned nb = asx_track_blocks(A.E.N, A.S, A.E.h);
    const dim3 grid(nb, (unsigned)(A.S * tiles), (unsigned)count), block(ASX_THREADS);
    const AsxPoolPair *list = A.E.nsrc ? pl : nullptr;
    if (A.E.nsrc) {
        hipLaunchKernelGGL(k_curve_resolve, dim3(((unsigned)count + ASX_THREADS - 1) / ASX_THREADS), block, 0, s, A.E, first, count, pl);
        hipLaunchKernelGGL(k_track_dots<AsxAtList>, grid, block, 0, s, src, smp, AsxAtList{ pl }, A, first, tiles, part);
    } else {
        hipLaunchKernelGGL(k_track_dots<AsxAtPitch>, grid, block, 0, s, src, smp, AsxAtPitch{ (size_t)A.E.src_stride, (size_t)A.E.smp_stride },
                           A, first, tiles, part);
    }
    if (nb > 1u)
        hipLaunchKernelGGL(k_track_sum, dim3((unsigned)(A.S * tiles), (unsigned)count), dim3(64), 0, s, A, first, tiles, nb,
                           (const double *)part, list);
    hipLaunchKernelGGL(k_track_fit, dim3((unsigned)count), dim3(64), 0, s, A, first, list);
}

unsigned asx_warp_blocks(uint32_t N)
{
    const unsigned nb = asx_pearson_blocks(N) * 6u / (unsigned)ASX_WARP_REC;
    return nb < 1u ? 1u : nb;
}

void asx_launch_warp(const float *src, const float *smp, const AsxWarp &A, size_t first, int count, AsxPoolPair *pl, double *part,
                     hipStream_t s)
{
    const unsigned nb = asx_warp_blocks(A.E.N);
    const dim3 grid(nb, (unsigned)count), block(ASX_THREADS);
    const AsxPoolPair *list = A.E.nsrc ? pl : nullptr;
    if (A.E.nsrc) {
        hipLaunchKernelGGL(k_curve_resolve, dim3(((unsigned)count + ASX_THREADS - 1) / ASX_THREADS), block, 0, s, A.E, first, count, pl);
        hipLaunchKernelGGL(k_warp_dots<AsxAtList>, grid, block, 0, s, src, smp, AsxAtList{ pl }, A, first, part);
    } else {
        hipLaunchKernelGGL(k_warp_dots<AsxAtPitch>, grid, block, 0, s, src, smp, AsxAtPitch{ (size_t)A.E.src_stride, (size_t)A.E.smp_stride },
                           A, first, part);
    }
    hipLaunchKernelGGL(k_warp_final, dim3((unsigned)count), dim3(64), 0, s, A, first, nb, (const double *)part, list);
}

void asx_launch_cvt_f64_f32(const double *in, float *out, size_t n, hipStream_t s)
{
    size_t blocks = (n + ASX_THREADS - 1) / ASX_THREADS;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_cvt_f64_f32, dim3((unsigned)blocks), dim3(ASX_THREADS), 0, s, in, out, n);
}

template <typename TIn>
void asx_launch_dc_remove(const TIn *src, const TIn *smp, uint32_t N, double scale, double *stats, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_dc_partial<TIn>, dim3(ASX_DC_BLOCKS), dim3(ASX_THREADS), 0, s, src, smp, N, stats + 4);
    hipLaunchKernelGGL(k_dc_final, dim3(1), dim3(64), 0, s, stats + 4, N, scale, stats);
    hipLaunchKernelGGL(k_dc_apply<TIn>, dim3(512), dim3(ASX_THREADS), 0, s, src, N, stats, out);
}

// the exact passes' instances (asx_internal.h): float32 and float64 inputs
#define ASX_EXACT_PASSES(T)                                                                                                             \
    template void asx_launch_refine<T>(const AsxDev &, const AsxInputs<T> &, const AsxPeakWs &, AsxSeg *, int, hipStream_t, int, bool,    \
                                       const AsxSearch &);                                                                              \
    template void asx_launch_pearson<T>(const AsxInputs<T> &, uint32_t, const AsxSeg *, double *, int64_t *, double *, int32_t *, int,    \
                                        hipStream_t);                                                                                   \
    template void asx_launch_dc_remove<T>(const T *, const T *, uint32_t, double, double *, float *, hipStream_t);
ASX_EXACT_PASSES(float)
ASX_EXACT_PASSES(double)
#undef ASX_EXACT_PASSES

void asx_launch_synth(uint64_t seed, uint64_t first_pair, size_t count, uint32_t N, int noise_shift,
                      float *src, float *smp, int64_t *true_lag, hipStream_t s)
{
    unsigned bx = (2u * N + ASX_THREADS - 1) / ASX_THREADS;
    if (bx > 1024) bx = 1024;
    const float amp = ldexpf(1.0f, -noise_shift);
    hipLaunchKernelGGL(k_synth, dim3(bx, (unsigned)count), dim3(ASX_THREADS), 0, s, seed, first_pair, N,
                       amp, src, smp, true_lag);
}
#endif // ASX_HAS_PART(64)
