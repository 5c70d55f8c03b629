// csrc/pearson_spectral.hip -- the Pearson coefficient (src/cross_correlation.c:74-116) WITHOUT a second pass over the inputs.
//
// The reference reads both segments twice (means, then centred sums).  Everything those sums are made of has already
// passed through this path's kernels by the time the lag is known:
//
//   coefficient = (Sxy - Sx Sy / n) / sqrt((Sxx - Sx^2 / n) (Syy - Sy^2 / n))         (the same formula, expanded)
//
//   lag >= 0   source[lag .. lag + N) against sample[0 .. N)   (:264-271)
//              Sxy = r[peak] EXACTLY the sum the transforms computed (no wrap-around: lag + N <= 2N);
//   lag <  0   source[0 .. L) against sample[N - L .. N), L = N + lag   (:256-263)
//              Sxy = r[peak] - sum_{n < -lag} source[peak + n] sample[n]   (the part of the circular sum that did not wrap):
//              |lag| products instead of L, worth it when |lag| < L;
//   Sx, Sxx, Sy, Syy   window sums: k_fwd_cols_r leaves {sum, sum of squares} of every (band of AsxDev::band_rows rows) x (tile)
//              of the [2 M1][M2] sample matrix (AsxPeakWs::band) from the loads it makes anyway; a window is whole bands (their
//              cells summed here, <= 144 KB per track) plus two band edges (at most 2 * band_rows * M2 samples, read here).
//
// r[peak] is the float32 transforms' value (k_inv_cols_r leaves the SIGNED value of each tile's best lag, AsxPeakWs::tile_peak),
// or the exact one when the pair's near-ties were re-evaluated (k_refine_dots).  Its error is bounded by the SAME bound B that
// guards the lag (asx_internal.h); the band sums are float32 sums of 128 - 160 terms: the squares eight fused multiply-adds per row pair and a
// tree over the pairs (<= 13 u relative), the plain sums a short tree (<= 10 u of sum |x|): both inside the 16 u asx_spec_pick uses.  asx_spec_pick (xcorr_dev.h; every block of k_pearson_partial runs
// it on what k_pearson_prep left, block 0 records the mode for k_pearson_final_spec) turns both into a first-order
// bound on the coefficient's error and keeps the spectral form only when that bound is below `tol` (1e-5, north_star's tolerance);
// otherwise -- quiet windows of a loud track, offsets, short segments -- the pair takes the reference's own reduction
// (k_pearson_partial over the segment, ASX_PM_DIRECT).  Float32 inputs on real-column plans only; the double ABI,
// the second look and the packed-sample kernels keep the direct reduction.
//
// Per pair the pass reads: FAST <= 2 band edges of each track (<= 0.3 MB at N = 1 440 000 instead of 11.5 MB); CORR + 8 |lag|
// bytes; DIRECT 8 L bytes as before.
#include "asx_internal.h"
#include "xcorr_dev.h"


static_assert(ASX_PREP_BLOCKS <= ASX_PREP_BLOCKS_MAX, "AsxSpecWs::part is sized for ASX_PREP_BLOCKS_MAX blocks per pair");
#ifndef ASX_PREP_THREADS
#define ASX_PREP_THREADS 1024 // per block of k_pearson_prep on the long tracks (ASX_PREP_BLOCKS blocks per pair)
#endif

namespace {

struct Acc2 {
    double s1, s2;
};

__device__ __forceinline__ void acc1(Acc2 &a, float f)
{
    const double v = (double)f;
    a.s1 += v;
    a.s2 = fma(v, v, a.s2);
}
__device__ __forceinline__ void acc4(Acc2 &a, float4 v) { acc1(a, v.x); acc1(a, v.y); acc1(a, v.z); acc1(a, v.w); }

// sum and sum of squares of track[lo .. hi) (float64 from the float32 samples), this thread's share: 16-byte loads over the
// aligned middle (the track starts on a 16-byte boundary: 2N and N are multiples of four), the ragged ends by single lanes.
// Four loads in flight per thread, each into its own accumulator (a fixed order all the same: the four are added at the end).
// NTP = the threads that share the range (all blocks of the pair), tid = this thread's index among them.
template <uint32_t NTP> __device__ __forceinline__ void direct_range(const float *__restrict__ x, uint32_t lo, uint32_t hi, Acc2 &a, uint32_t tid)
{
    if (lo >= hi) return;
    const uint32_t lo4 = (lo + 3u) & ~3u, hi4 = hi & ~3u;
    if (lo4 >= hi4) { // no aligned quad inside
        for (uint32_t i = lo + tid; i < hi; i += NTP) acc1(a, x[i]);
        return;
    }
    if (tid < lo4 - lo) acc1(a, x[lo + tid]);
    if (tid < hi - hi4) acc1(a, x[hi4 + tid]);
    const float4 *q = reinterpret_cast<const float4 *>(x);
    const uint32_t end = hi4 >> 2;
    uint32_t i = (lo4 >> 2) + tid;
    Acc2 b{ 0.0, 0.0 }, c{ 0.0, 0.0 }, d{ 0.0, 0.0 };
    for (; i + 3u * NTP < end; i += 4u * NTP) {
        const float4 v0 = q[i], v1 = q[i + NTP], v2 = q[i + 2u * NTP], v3 = q[i + 3u * NTP];
        acc4(a, v0); acc4(b, v1); acc4(c, v2); acc4(d, v3);
    }
    for (; i < end; i += NTP) acc4(a, q[i]);
    a.s1 += (b.s1 + c.s1) + d.s1;
    a.s2 += (b.s2 + c.s2) + d.s2;
}

// This thread's share of the window sums of one track over [lo, hi): whole bands from the band sums, the two edges from the samples.
//   band: [ntiles][nbands] {sum, sum of squares} as k_fwd_cols_r left them (every block its own run); a band = gs consecutive samples.
//   The (tile, band) cells of the window are dealt to the threads in order -- consecutive lanes walk the bands of a tile --
//   and added in float64: a fixed order.
template <uint32_t NTP> __device__ __forceinline__ Acc2 window_share(const float *__restrict__ x, const float2 *__restrict__ band, uint32_t gs, int ntiles,
                                             int nbands, uint32_t lo, uint32_t hi, uint32_t tid)
{
    Acc2 a{ 0.0, 0.0 };
    const uint32_t ba = (lo + gs - 1) / gs, bb = hi / gs;
    if (ba < bb) {
        direct_range<NTP>(x, lo, ba * gs, a, tid);
        direct_range<NTP>(x, bb * gs, hi, a, tid);
        const uint32_t w = bb - ba, cells = w * (uint32_t)ntiles;
        const uint32_t dq = NTP / w, dr = NTP - dq * w; // one step of the cell index, as (tiles, bands)
        uint32_t t = tid / w, b = tid - t * w;
        Acc2 e{ 0.0, 0.0 };
        uint32_t i = tid;
        for (; i + NTP < cells; i += 2u * NTP) { // two cells in flight
            uint32_t t2 = t + dq, b2 = b + dr;
            if (b2 >= w) { b2 -= w; t2++; }
            const float2 v = band[(size_t)t * nbands + ba + b], v2 = band[(size_t)t2 * nbands + ba + b2];
            a.s1 += (double)v.x; a.s2 += (double)v.y;
            e.s1 += (double)v2.x; e.s2 += (double)v2.y;
            t = t2 + dq; b = b2 + dr;
            if (b >= w) { b -= w; t++; }
        }
        if (i < cells) {
            const float2 v = band[(size_t)t * nbands + ba + b];
            a.s1 += (double)v.x; a.s2 += (double)v.y;
        }
        a.s1 += e.s1; a.s2 += e.s2;
    } else {
        direct_range<NTP>(x, lo, hi, a, tid);
    }
    return a;
}

// block-wide sums of four numbers, fixed order (lane tree, then waves in order); valid in every thread
template <int NTP> __device__ __forceinline__ void block_sum4(double (&v)[4], double (*red)[NTP / 64])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] += __shfl_xor(v[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 4; k++) red[k][wave] = v[k];
    __syncthreads();
    for (int k = 0; k < 4; k++) {
        double t = red[k][0];
        for (int w = 1; w < NTP / 64; w++) t += red[k][w];
        v[k] = t;
    }
}

} // namespace

// grid (NB, npairs), NTP threads (1024 for the long tracks -- up to 77 000 samples of band edges and 18 000 cells per pair -- 256 below:
// 1024 pairs of N = 144 000 took 61 us with 1024-thread blocks, the sixteen-wave fold of a few thousand numbers).  Picks the winner among the re-evaluated near-ties (if any) and leaves the pair's window-sum shares and r[peak] (AsxSpecWs).
// NB > 1 (the long tracks): NB blocks share a pair's cells and edges -- NB * NTP threads dealt the same way -- and each leaves its SHARE of the
// four sums; the kernels behind this one add the shares in block order (asx_spec_pick): the same bits whoever adds them, and NB is a
// constant of the plan (the same pair takes the same tree alone, in a batch, on another shard).  No merged record, hence no fence and no
// ticket: profiles/r5_experiments/18_* (one block per pair: 25 us for a single pair behind ONE block's loads) and 22_*.
// src_pitch / smp_pitch: the pairs' input steps in floats (0 = one track for every pair).
template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                    const float *__restrict__ smp, size_t src_pitch, size_t smp_pitch,
                                                                    AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg, uint32_t seed)
{
#include "pearson_prep_body.h"
}

// the per-pair form (asx_xcorr_windowed_f32_dev): the seed is the pair's own, from its row.  An invalid row has no maximum, so the pair
// takes the direct reduction (and is counted as ASX_PM_DIRECT) before k_invalid_rows overwrites its results.
template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep_p(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                      const float *__restrict__ smp, size_t src_pitch, size_t smp_pitch,
                                                                      AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg, AsxWinRows R)
{
    AsxWin Z;
    (void)asx_win_row(R, blockIdx.y, Pp->N, Z);
    const uint32_t seed = Z.seed;
#include "pearson_prep_body.h"
}

// the top-k form (asx_xcorr_topk_f32_dev, passes 2..k): the seed is the pass's, from the pair's record.  An empty A_j has no maximum,
// so the pair takes the direct reduction (counted as ASX_PM_DIRECT) before k_topk_step writes (0, NaN, -3) for it.
template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep_x(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                      const float *__restrict__ smp, size_t src_pitch, size_t smp_pitch,
                                                                      AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg,
                                                                      const AsxTopkPair *__restrict__ X)
{
    const uint32_t seed = X[blockIdx.y].z.seed;
#include "pearson_prep_body.h"
}

// the listed forms (asx_xcorr_pool_f32_dev): pair i's inputs at src + PL[i].src_off, smp + PL[i].smp_off; the plan's seed, or (_pl) the
// pair's own from its row
template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep_l(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                      const float *__restrict__ smp, const AsxPoolPair *__restrict__ PL,
                                                                      AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg, uint32_t seed)
{
#define ASX_SRC_OF(pair) PL[pair].src_off
#define ASX_SMP_OF(pair) PL[pair].smp_off
#include "pearson_prep_body.h"
}

template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep_pl(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                       const float *__restrict__ smp, const AsxPoolPair *__restrict__ PL,
                                                                       AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg, AsxWinRows R)
{
    AsxWin Z;
    (void)asx_win_row(R, blockIdx.y, Pp->N, Z);
    const uint32_t seed = Z.seed;
#define ASX_SRC_OF(pair) PL[pair].src_off
#define ASX_SMP_OF(pair) PL[pair].smp_off
#include "pearson_prep_body.h"
}

// the listed top-k form (asx_xcorr_pool_topk_f32_dev, passes 2..k): the seed from the pair's record as k_pearson_prep_x, the inputs
// from the pair's pool record as k_pearson_prep_l
template <int NTP, int NB> __global__ __launch_bounds__(NTP) void k_pearson_prep_xl(const AsxDev *__restrict__ Pp, const float *__restrict__ src,
                                                                       const float *__restrict__ smp, const AsxPoolPair *__restrict__ PL,
                                                                       AsxPeakWs W, AsxSpecWs S, AsxSeg *__restrict__ seg,
                                                                       const AsxTopkPair *__restrict__ X)
{
    const uint32_t seed = X[blockIdx.y].z.seed;
#define ASX_SRC_OF(pair) PL[pair].src_off
#define ASX_SMP_OF(pair) PL[pair].smp_off
#include "pearson_prep_body.h"
}

// grid (npairs), one wave per pair: k_pearson_final (xcorr_kernels.hip) with the two spectral modes in front of it.
__global__ __launch_bounds__(64) void k_pearson_final_spec(const AsxSeg *__restrict__ seg, const double *__restrict__ psums, uint32_t nb,
                                                            AsxSpecWs S, int64_t *__restrict__ lag,
                                                            double *__restrict__ coef, int32_t *__restrict__ ret)
{
    const size_t pair = blockIdx.x;
    const AsxSeg s = seg[pair];
    const AsxSpecPick d = asx_spec_pick(s, S.part + pair * (size_t)(S.nb * 4), S.nb, S.hdr + pair * ASX_SPEC_HDR, S.tol, S.N); // the sums
    // ... and the mode k_pearson_partial's block 0 recorded: the one its blocks wrote the partial sums for (never decided twice)
    const int mode = (int)S.hdr[pair * ASX_SPEC_HDR + 3];
    PStat v;
    v.n = v.mx = v.my = v.mxx = v.myy = v.cxy = 0.0;
    if (mode != ASX_PM_FAST) { // wave-uniform
        for (uint32_t b = threadIdx.x; b < nb; b += 64u) {
            const double *p = psums + (pair * nb + b) * 6;
            PStat o;
            o.n = p[0];
            if (o.n != 0.0) { o.mx = p[1]; o.my = p[2]; o.mxx = p[3]; o.myy = p[4]; o.cxy = p[5]; v = pstat_merge(v, o); }
        }
        v = pstat_wave_merge(v);
    }
    if (threadIdx.x == 0) {
        double c;
        if (mode == ASX_PM_DIRECT) {
            c = v.cxy / sqrt(v.mxx * v.myy); // src/cross_correlation.c:115
        } else {
            const double n = d.n, Sx = d.Sx, Sxx = d.Sxx, Sy = d.Sy, Syy = d.Syy;
            double sxy = d.r;
            if (mode == ASX_PM_CORR) sxy -= v.cxy + v.n * v.mx * v.my; // minus the products that did not wrap around
            c = (sxy - Sx * Sy / n) / sqrt((Sxx - Sx * Sx / n) * (Syy - Sy * Sy / n));
            c = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c; // the reference's value cannot leave [-1, 1]; NaN stays NaN
        }
        if (lag) lag[pair] = s.lag;
        coef[pair] = c;
        if (ret) ret[pair] = (s.flags & ASX_SEG_INEXACT) ? 1 : (c != c) ? -1 : 0; // as k_pearson_final (:276)
        atomicAdd(S.mode_count + mode, 1ull);
    }
}

// the prep kernel of the group's inputs (listed: the plan's seed, the pairs' rows or their top-k records) and search, NB blocks of NTP threads per pair
template <int NTP, int NB>
static void launch_prep(const AsxDev &P, const AsxInputs<float> &in, const AsxSearch &q, const AsxPeakWs &W, const AsxSpecWs &S,
                        AsxSeg *seg, int npairs, hipStream_t s)
{
    const dim3 grid(NB, npairs), block(NTP);
    if (in.pl && q.kind == AsxSearch::TOPK)
        hipLaunchKernelGGL((k_pearson_prep_xl<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.pl, W, S, seg, q.tk);
    else if (in.pl && q.kind == AsxSearch::ROWS)
        hipLaunchKernelGGL((k_pearson_prep_pl<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.pl, W, S, seg, q.rows);
    else if (in.pl)
        hipLaunchKernelGGL((k_pearson_prep_l<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.pl, W, S, seg, q.seed());
    else if (q.kind == AsxSearch::TOPK)
        hipLaunchKernelGGL((k_pearson_prep_x<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.src_pitch, in.smp_pitch, W, S,
                           seg, q.tk);
    else if (q.kind == AsxSearch::ROWS)
        hipLaunchKernelGGL((k_pearson_prep_p<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.src_pitch, in.smp_pitch, W, S,
                           seg, q.rows);
    else
        hipLaunchKernelGGL((k_pearson_prep<NTP, NB>), grid, block, 0, s, P.self_dev, in.src, in.smp, in.src_pitch, in.smp_pitch, W, S,
                           seg, q.seed());
}

// the long-track form of k_pearson_prep: ASX_PREP_BLOCKS blocks of ASX_PREP_THREADS threads per pair (a function of the plan alone)
static bool prep_long_tracks(const AsxDev &P) { return (size_t)P.band_rows * (size_t)P.M2 >= 16384; }

void asx_launch_pearson_spectral_f32(const AsxDev &P, const AsxInputs<float> &in, const AsxSearch &q, const AsxPeakWs &W,
                                     const AsxSpecWs &S0, AsxSeg *seg, double *psums, int64_t *lag, double *coef, int32_t *ret,
                                     int npairs, hipStream_t s)
{
    AsxSpecWs S = S0;
    S.N = P.N;
    const bool long_tracks = prep_long_tracks(P);
    S.nb = long_tracks ? ASX_PREP_BLOCKS : 1;
    if (long_tracks) launch_prep<ASX_PREP_THREADS, ASX_PREP_BLOCKS>(P, in, q, W, S, seg, npairs, s);
    else launch_prep<256, 1>(P, in, q, W, S, seg, npairs, s);
    asx_launch_pearson_partial_spec_f32(in, P.N, seg, S, psums, npairs, s);
    hipLaunchKernelGGL(k_pearson_final_spec, dim3(npairs), dim3(64), 0, s, seg, psums, asx_pearson_blocks(P.N), S, lag, coef, ret);
}

// diagnostic (asx_plan_debug_spectral, asx_api.hip): asx_spec_pick of one pair, called on the device as k_pearson_partial and
// k_pearson_final_spec call it, from what the last group left -- out = {mode, n, Sx, Sxx, Sy, Syy, r, bound}.  One thread; launched
// by the diagnostic alone.
__global__ __launch_bounds__(64) void k_debug_spec_pick(const AsxSeg *__restrict__ seg, AsxSpecWs S, size_t pair, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const AsxSpecPick d = asx_spec_pick(seg[pair], S.part + pair * (size_t)(S.nb * 4), S.nb, S.hdr + pair * ASX_SPEC_HDR, S.tol, S.N);
    out[0] = (double)d.mode; out[1] = d.n; out[2] = d.Sx; out[3] = d.Sxx; out[4] = d.Sy; out[5] = d.Syy; out[6] = d.r; out[7] = d.bound;
}

int asx_launch_debug_spec_pick(const AsxDev &P, const AsxSpecWs &S0, const AsxSeg *seg, size_t pair, double *out, hipStream_t s)
{
    AsxSpecWs S = S0;
    S.N = P.N;
    S.nb = prep_long_tracks(P) ? ASX_PREP_BLOCKS : 1; // as asx_launch_pearson_spectral_f32 sets them
    hipLaunchKernelGGL(k_debug_spec_pick, dim3(1), dim3(1), 0, s, seg, S, pair, out);
    return S.nb;
}
