// csrc/ncc.hip — normalised cross-correlation (asx_xcorr_ncc_f32_dev): the k_ncc_* kernels, which turn the float32 r of lags 0..N-1
// that an ordinary launch group left (run_group with r_out, asx_api.hip) into the Pearson coefficient of every lag and search its peak.
// They know nothing of the transform layout: they read the caller's tracks, r and a plan-owned workspace (AsxNccWs).
//
// Everything behind r32 is float64, and every sum is a fixed tree that the track length alone decides: a track is cut into chunks of
// ASX_NCC_CHUNK frames, a chunk is summed by one block (thread t takes the frames t, t + 256, ..., then lanes, then waves), the chunk
// sums by thread-strided partial sums and the same block tree.  No value of a pair depends on the batch or on its place in it.
//   k_ncc_sums     grid (source chunks + sample chunks, tracks): the plain sum of every chunk, for the means
//   k_ncc_moments  same grid: mu (every block forms it from the chunk sums, in the same order), then sum (x - mu) and sum (x - mu)^2
//                  of the chunk: an offset costs no digits
//   k_ncc_table    grid (lag chunks + 1, tracks): block b < lag chunks owns the lags [b CHUNK, (b + 1) CHUNK): the window sums of its
//                  first lag from whole chunk sums and the frames of the remainder, then a block scan of the sliding differences
//                  (x[l + N] - mu)^k - (x[l] - mu)^k, k = 1, 2 -> the per-lag table {Sx' (mu-shifted), Vx} and the track's Vmax
//                  (atomic maximum: order-free).  The extra block: Sy and Vy of the sample track.
//   k_ncc_peak     grid (lag chunks, pairs): c32 of the block's lags, the window and the competing rule, the packed (|c32|, smallest
//                  lag) maximum of the pair (asx_peak_t, atomic maximum); optionally c32 itself for the debug call
//   k_ncc_finalize a thread per pair: AsxSeg through make_seg and the peak height
//   k_ncc_invalid  a thread per pair, behind the Pearson kernels: (0, NaN, NaN, -2) for a row that is not a window of this call
// The pool calls (asx_xcorr_pool_ncc_f32_dev) run the three moment kernels over the tracks of the two pools, once per call, into the
// plan's track set (asx_launch_ncc_pool_moments: the same kernels on the same chunks, so the same trees), and k_ncc_peak finds a
// pair's table and statistics through its pool record.  The top-k calls add k_ncctop_scan and k_ncctop_step (below).
#include "asx_internal.h"
#include "xcorr_dev.h"

#define NCC_NT 256
#define NCC_PER (ASX_NCC_CHUNK / NCC_NT)
static_assert(ASX_NCC_CHUNK % NCC_NT == 0 && NCC_PER == 8, "eight frames per thread");

// ---- block-wide float64 sums and scans: lanes (shuffles), then the four waves in index order ---------------------------------------
__device__ __forceinline__ double ncc_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the sums of a and b over the block, in every thread; lds: 2 * (NCC_NT / 64) doubles
__device__ __forceinline__ void ncc_block_sum2(double &a, double &b, double *lds)
{
    a = ncc_wave_sum(a);
    b = ncc_wave_sum(b);
    __syncthreads(); // (lds may still be read from the call before)
    if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6] = a; lds[NCC_NT / 64 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    a = lds[0]; b = lds[NCC_NT / 64];
#pragma unroll
    for (int w = 1; w < NCC_NT / 64; w++) { a += lds[w]; b += lds[NCC_NT / 64 + w]; }
}
// the sums of a[0 .. n) and b[0 .. n) (b may be null: zero), in every thread
__device__ __forceinline__ void ncc_sum_arrays(const double *__restrict__ a, const double *__restrict__ b, uint32_t n, double &sa,
                                               double &sb, double *lds)
{
    sa = 0.0; sb = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += NCC_NT) { sa += a[i]; if (b) sb += b[i]; }
    ncc_block_sum2(sa, sb, lds);
}

// which track and chunk a block of the grid (source chunks + sample chunks, tracks) owns; false: none
struct NccChunk {
    const float *x;      // the track
    uint32_t len, c, nc; // its length, the block's chunk, its chunks
    size_t slot;         // where the chunk's sums go in raw / m1 / m2
    double *stat;        // the track's statistics
};
__device__ __forceinline__ bool ncc_chunk_of(const AsxNccWs &W, const float *src, size_t src_pitch, const float *smp, size_t smp_pitch,
                                             uint32_t N, NccChunk &k)
{
    const uint32_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), t = blockIdx.y;
    if (blockIdx.x < nsc) {
        if (t >= W.nsrc || !W.do_src) return false;
        k = { src + (size_t)t * src_pitch, 2u * N, blockIdx.x, nsc, (size_t)t * nsc + blockIdx.x, W.sstat + (size_t)t * ASX_NCC_STAT };
    } else {
        if (t >= W.nsmp || !W.do_smp) return false;
        k = { smp + (size_t)t * smp_pitch, N, blockIdx.x - nsc, nyc, (size_t)W.nsrc * nsc + (size_t)t * nyc + (blockIdx.x - nsc),
              W.ystat + (size_t)t * ASX_NCC_STAT };
    }
    return true;
}

__global__ __launch_bounds__(NCC_NT) void k_ncc_sums(AsxNccWs W, const float *__restrict__ src, size_t src_pitch,
                                                      const float *__restrict__ smp, size_t smp_pitch, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    NccChunk k;
    if (!ncc_chunk_of(W, src, src_pitch, smp, smp_pitch, N, k)) return;
    const uint32_t f0 = k.c * ASX_NCC_CHUNK;
    double s = 0.0, z = 0.0;
#pragma unroll
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t f = f0 + j * NCC_NT + threadIdx.x;
        if (f < k.len) s += (double)k.x[f];
    }
    ncc_block_sum2(s, z, lds);
    if (threadIdx.x == 0) {
        W.raw[k.slot] = s;
        if (k.c == 0 && blockIdx.x < asx_ncc_chunks(2u * N)) k.stat[1] = 0.0; // the source track's Vmax, which k_ncc_table raises
    }
}

__global__ __launch_bounds__(NCC_NT) void k_ncc_moments(AsxNccWs W, const float *__restrict__ src, size_t src_pitch,
                                                         const float *__restrict__ smp, size_t smp_pitch, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    NccChunk k;
    if (!ncc_chunk_of(W, src, src_pitch, smp, smp_pitch, N, k)) return;
    double tot, z;
    ncc_sum_arrays(W.raw + (k.slot - k.c), nullptr, k.nc, tot, z, lds);
    const double mu = tot / (double)k.len;
    const uint32_t f0 = k.c * ASX_NCC_CHUNK;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t f = f0 + j * NCC_NT + threadIdx.x;
        if (f < k.len) { const double a = (double)k.x[f] - mu; s1 += a; s2 += a * a; }
    }
    ncc_block_sum2(s1, s2, lds);
    if (threadIdx.x == 0) {
        W.m1[k.slot] = s1;
        W.m2[k.slot] = s2;
        if (k.c == 0) k.stat[0] = mu;
    }
}

__global__ __launch_bounds__(NCC_NT) void k_ncc_table(AsxNccWs W, const float *__restrict__ src, size_t src_pitch, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    __shared__ float head[ASX_NCC_CHUNK], tail[ASX_NCC_CHUNK];
    const uint32_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), t = blockIdx.y;
    const double dN = (double)N;
    if (blockIdx.x == nyc) {
        // the sample track: Sy and Vy about its own mean
        if (t >= W.nsmp || !W.do_smp) return;
        const size_t at = (size_t)W.nsrc * nsc + (size_t)t * nyc;
        double s1, s2;
        ncc_sum_arrays(W.m1 + at, W.m2 + at, nyc, s1, s2, lds);
        if (threadIdx.x == 0) {
            double *st = W.ystat + (size_t)t * ASX_NCC_STAT;
            st[2] = s1 + dN * st[0];
            st[3] = s2 - s1 * s1 / dN;
        }
        return;
    }
    if (t >= W.nsrc || !W.do_src) return;
    const float *x = src + (size_t)t * src_pitch;
    double *st = W.sstat + (size_t)t * ASX_NCC_STAT;
    const double mu = st[0];
    const uint32_t b = blockIdx.x, l0 = b * ASX_NCC_CHUNK;
    // the block's frames: [l0, l0 + CHUNK) leave the window one by one, [l0 + N, l0 + N + CHUNK) enter it (zero past the track's end:
    // only lags >= N would read them)
#pragma unroll
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t i = j * NCC_NT + threadIdx.x, f = l0 + i, e = l0 + N + i;
        head[i] = f < 2u * N ? x[f] : 0.f;
        tail[i] = e < 2u * N ? x[e] : 0.f;
    }
    // the window [l0, l0 + N) of the block's first lag: K whole chunks from chunk b on, then R frames
    const uint32_t K = N / ASX_NCC_CHUNK, R = N % ASX_NCC_CHUNK;
    double w1, w2;
    ncc_sum_arrays(W.m1 + (size_t)t * nsc + b, W.m2 + (size_t)t * nsc + b, K, w1, w2, lds);
    {
        double r1 = 0.0, r2 = 0.0;
        const uint32_t f0 = l0 + K * ASX_NCC_CHUNK;
        for (uint32_t i = threadIdx.x; i < R; i += NCC_NT) { const double a = (double)x[f0 + i] - mu; r1 += a; r2 += a * a; }
        ncc_block_sum2(r1, r2, lds); // (its first barrier also puts head and tail in place)
        w1 += r1; w2 += r2;
    }
    // the thread's eight consecutive lags l0 + 8 tid + k: exclusive prefix of the sliding differences inside the thread, ...
    double p1[NCC_PER], p2[NCC_PER], t1 = 0.0, t2 = 0.0;
    const uint32_t j0 = threadIdx.x * NCC_PER;
#pragma unroll
    for (int k = 0; k < NCC_PER; k++) {
        p1[k] = t1; p2[k] = t2;
        const double in = (double)tail[j0 + k] - mu, out = (double)head[j0 + k] - mu;
        t1 += in - out;
        t2 += in * in - out * out;
    }
    // ... across the lanes (an inclusive scan of the threads' totals), across the waves
    double i1 = t1, i2 = t2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double u1 = __shfl_up(i1, off, 64), u2 = __shfl_up(i2, off, 64);
        if (lane >= off) { i1 += u1; i2 += u2; }
    }
    __syncthreads();
    if (lane == 63) { lds[wave] = i1; lds[NCC_NT / 64 + wave] = i2; }
    __syncthreads();
    double o1 = __shfl_up(i1, 1, 64), o2 = __shfl_up(i2, 1, 64); // exclusive in the wave
    if (lane == 0) { o1 = 0.0; o2 = 0.0; }
    for (int w = 0; w < wave; w++) { o1 += lds[w]; o2 += lds[NCC_NT / 64 + w]; }
    double vmax = 0.0;
    double2 *tab = W.table + (size_t)t * N;
#pragma unroll
    for (int k = 0; k < NCC_PER; k++) {
        const uint32_t l = l0 + j0 + k;
        if (l < N) {
            const double s1 = w1 + (o1 + p1[k]), s2 = w2 + (o2 + p2[k]);
            const double vx = s2 - s1 * s1 / dN;
            tab[l] = make_double2(s1, vx);
            vmax = fmax(vmax, vx); // (a NaN drops out)
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, off, 64));
    // non-negative doubles order as their bits do
    if (lane == 0 && vmax > 0.0) atomicMax(reinterpret_cast<unsigned long long *>(st + 1), (unsigned long long)__double_as_longlong(vmax));
}

// c_out: c32 of pair i's lag l to c_out[i * c_pitch + l] (the debug call: [pairs][N]; a top-k group: the upper half of r, which this
// kernel does not read).  pl: a pool group's records -- pair i's table and statistics are those of its slots in the plan's track set.
__global__ __launch_bounds__(NCC_NT) void k_ncc_peak(AsxNccWs W, const float *__restrict__ r, size_t r_pitch, uint32_t N, double scale,
                                                      double min_energy, const int64_t *__restrict__ rows, size_t rows_step,
                                                      float *__restrict__ c_out, size_t c_pitch, const AsxPoolPair *__restrict__ pl)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    const size_t ts = pl ? pl[pair].sx : W.nsrc > 1 ? pair : 0, ty = pl ? pl[pair].sy : W.nsmp > 1 ? pair : 0;
    const double *sx = W.sstat + ts * ASX_NCC_STAT, *sy = W.ystat + ty * ASX_NCC_STAT;
    const double mu = sx[0], floor_v = min_energy * sx[1], Sy = sy[2], Vy = sy[3], dN = (double)N;
    int64_t lo = 0, hi = (int64_t)N - 1;
    if (rows) {
        lo = rows[2 * pair * rows_step]; hi = rows[2 * pair * rows_step + 1];
        if (!asx_ncc_row_ok(lo, hi, N)) hi = -1; // holds no lag
    }
    const double2 *tab = W.table + ts * N;
    const float *rp = r + pair * r_pitch;
    const uint32_t l0 = blockIdx.x * ASX_NCC_CHUNK;
    asx_peak_t best = 0;
#pragma unroll 2
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t l = l0 + j * NCC_NT + threadIdx.x;
        if (l >= N) break;
        const double2 e = tab[l];
        const double Sx = e.x + dN * mu;
        const double c = ((double)rp[l] / scale - Sx * Sy / dN) / sqrt(e.y * Vy);
        const float c32 = (float)c;
        const bool competes = Vy > 0.0 && e.y >= floor_v && fabs(c) <= 1.7976931348623157e308; // (false for a NaN and for +-infinity)
        if (c_out) c_out[pair * c_pitch + l] = competes ? c32 : NAN;
        if (competes && (int64_t)l >= lo && (int64_t)l <= hi) best = peak_max(best, peak_pack_key(fabsf(c32), l));
    }
    best = block_peak_max(best, red);
    if (threadIdx.x == 0 && best) atomicMax(&W.best[pair], best);
}

__global__ __launch_bounds__(NCC_NT) void k_ncc_finalize(AsxNccWs W, uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                          AsxSeg *__restrict__ seg, double *__restrict__ peak, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    const asx_peak_t best = W.best[pair];
    uint32_t first = 0; // no lag competes: the window's lag_min (an invalid row: 0, and k_ncc_invalid writes its results)
    if (rows) {
        const int64_t lo = rows[2 * (size_t)pair * rows_step], hi = rows[2 * (size_t)pair * rows_step + 1];
        if (asx_ncc_row_ok(lo, hi, N)) first = (uint32_t)lo;
    }
    seg[pair] = make_seg(best ? peak_index(best) : first, N);
    peak[pair] = best ? (double)peak_key(best) : 0.0;
}

__global__ __launch_bounds__(NCC_NT) void k_ncc_invalid(uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                         int64_t *__restrict__ lag, double *__restrict__ coef, double *__restrict__ peak,
                                                         int32_t *__restrict__ ret, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    if (asx_ncc_row_ok(rows[2 * (size_t)pair * rows_step], rows[2 * (size_t)pair * rows_step + 1], N)) return;
    if (lag) lag[pair] = 0;
    coef[pair] = (double)NAN;
    peak[pair] = (double)NAN;
    ret[pair] = -2;
}

// ---- top-k (asx_xcorr_ncc_topk_f32_dev, asx_xcorr_pool_ncc_topk_f32_dev) ---------------------------------------------------------
// Pass 0 is k_ncc_peak, which leaves c32 of every lag in the upper half of the pair's r (NaN: the lag does not compete).  A pass j >= 1
// rescans those 4N bytes with the row and the zones around the record's j earlier entries masked out; between the passes a thread per
// pair turns the pass's maximum into entry j and the segment of the direct Pearson pass, and moves entry j - 1 to the caller's arrays.
// (These kernels are k_ncctop_*, not k_ncc_*: tests/test_ncc.py holds the k_ncc_ family to the six kernels of the one-lag call.)

// the zone of an earlier entry at `lag`: the lags zlo .. zlo + zwd = [lag - sep, lag + sep] clipped to [0, N-1]
__device__ __forceinline__ void ncctop_zone(int64_t lag, int64_t sep, uint32_t N, uint32_t &zlo, uint32_t &zwd)
{
    const int64_t n1 = (int64_t)N - 1;
    const int64_t lo = sep > lag ? 0 : lag - sep, hi = sep >= n1 - lag ? n1 : lag + sep; // (0 <= lag <= N-1: neither can overflow)
    zlo = (uint32_t)lo;
    zwd = (uint32_t)(hi - lo);
}

// grid (lag chunks, pairs): pass j, 1 <= j < ASX_TOPK_MAX.  The zones are tested as (l - zlo) > zwd in unsigned arithmetic, all
// ASX_TOPK_MAX - 1 of them whatever j is: an unused one is (~0, 0), which holds no lag (AsxWinX's form, asx_internal.h).
__global__ __launch_bounds__(NCC_NT) void k_ncctop_scan(AsxNccWs W, size_t r_pitch, uint32_t N, const int64_t *__restrict__ rows,
                                                         size_t rows_step, int64_t sep, int j)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    const AsxNccTopk *T = W.tk + pair;
    if (T->flags) return; // (the whole block: an invalid row, or no lag was left for an earlier entry)
    int64_t lo = 0, hi = (int64_t)N - 1;
    if (rows) { lo = rows[2 * pair * rows_step]; hi = rows[2 * pair * rows_step + 1]; }
    uint32_t zlo[ASX_TOPK_MAX - 1], zwd[ASX_TOPK_MAX - 1];
#pragma unroll
    for (int i = 0; i < ASX_TOPK_MAX - 1; i++) {
        zlo[i] = ~0u; zwd[i] = 0u;
        if (i < j) ncctop_zone(T->lag[i], sep, N, zlo[i], zwd[i]);
    }
    const float *c = W.r + pair * r_pitch + N;
    const uint32_t l0 = blockIdx.x * ASX_NCC_CHUNK;
    asx_peak_t best = 0;
#pragma unroll 2
    for (int q = 0; q < NCC_PER; q++) {
        const uint32_t l = l0 + q * NCC_NT + threadIdx.x;
        if (l >= N) break;
        const float v = c[l];
        bool in = v == v && (int64_t)l >= lo && (int64_t)l <= hi;
#pragma unroll
        for (int i = 0; i < ASX_TOPK_MAX - 1; i++) in = in && l - zlo[i] > zwd[i];
        if (in) best = peak_max(best, peak_pack_key(fabsf(v), l));
    }
    best = block_peak_max(best, red);
    if (threadIdx.x == 0 && best) atomicMax(&W.best[pair], best);
}

// a thread per pair, 0 <= j <= k (see asx_launch_ncctop_step).  The record stays in global memory: its lags are indexed by j.
__global__ __launch_bounds__(NCC_NT) void k_ncctop_step(AsxNccWs W, uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                         int64_t sep, int j, int k, AsxSeg *__restrict__ seg,
                                                         const int64_t *__restrict__ tmp_lag, const double *__restrict__ tmp_coef,
                                                         const int32_t *__restrict__ tmp_ret, int64_t *__restrict__ lag,
                                                         double *__restrict__ coef, double *__restrict__ peak, int32_t *__restrict__ ret,
                                                         int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    AsxNccTopk *T = W.tk + pair;
    int64_t lo = 0, hi = (int64_t)N - 1;
    if (rows) { lo = rows[2 * (size_t)pair * rows_step]; hi = rows[2 * (size_t)pair * rows_step + 1]; }
    uint32_t n = 0, flags = 0;
    if (j == 0) { if (!asx_ncc_row_ok(lo, hi, N)) flags = ASX_NCC_TK_INVALID; }
    else { n = T->n; flags = T->flags; }
    if (j > 0) {
        const size_t e = (size_t)pair * (size_t)k + (size_t)(j - 1);
        const bool none = flags & ASX_NCC_TK_INVALID || n < (uint32_t)j; // n < j: no lag was left for this entry
        if (lag) lag[e] = none ? 0 : tmp_lag[pair];
        coef[e] = none ? (double)NAN : tmp_coef[pair];
        peak[e] = none ? (double)NAN : T->peak;
        ret[e] = flags & ASX_NCC_TK_INVALID ? -2 : none ? -3 : tmp_ret[pair];
    }
    if (j >= k) return;
    const asx_peak_t best = W.best[pair];
    W.best[pair] = 0;
    uint32_t at = 0;
    if (!flags) {
        double height = 0.0;
        bool have = true;
        if (best) { at = peak_index(best); height = (double)peak_key(best); }
        else {
            // no lag of A_j competes: its smallest lag, the row's lag_min pushed past every zone that holds it
            int64_t cand = lo;
            for (int round = 0; round <= j; round++) {
                bool moved = false;
                for (int i = 0; i < j; i++) {
                    uint32_t zlo, zwd;
                    ncctop_zone(T->lag[i], sep, N, zlo, zwd);
                    if (cand >= (int64_t)zlo && cand <= (int64_t)zlo + (int64_t)zwd) { cand = (int64_t)zlo + (int64_t)zwd + 1; moved = true; }
                }
                if (!moved) break;
            }
            have = cand <= hi;
            at = have ? (uint32_t)cand : 0u;
        }
        if (have) { T->lag[j] = (int64_t)at; T->peak = height; n = (uint32_t)j + 1u; }
        else flags = ASX_NCC_TK_EMPTY;
    }
    T->n = n;
    T->flags = flags;
    seg[pair] = make_seg(at, N); // (an entry that is not to be: lag 0's segment, whose coefficient the next step drops)
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
void asx_launch_ncc_moments(const AsxNccWs &W, const float *src, size_t src_pitch, const float *smp, size_t smp_pitch, uint32_t N,
                            hipStream_t s)
{
    if (!W.do_src && !W.do_smp) return;
    const unsigned nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), nt = W.nsrc > W.nsmp ? W.nsrc : W.nsmp;
    hipLaunchKernelGGL(k_ncc_sums, dim3(nsc + nyc, nt), dim3(NCC_NT), 0, s, W, src, src_pitch, smp, smp_pitch, N);
    hipLaunchKernelGGL(k_ncc_moments, dim3(nsc + nyc, nt), dim3(NCC_NT), 0, s, W, src, src_pitch, smp, smp_pitch, N);
    hipLaunchKernelGGL(k_ncc_table, dim3(nyc + 1, nt), dim3(NCC_NT), 0, s, W, src, src_pitch, N);
}

void asx_launch_ncc_pool_moments(const AsxNccWs &T, const float *srcs, size_t src_pitch, size_t nsrc, const float *smps, size_t smp_pitch,
                                 size_t nsmp, uint32_t N, hipStream_t s)
{
    const size_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), most = 65535;
    for (size_t c0 = 0; c0 < std::max(nsrc, nsmp); c0 += most) {
        // tracks c0 .. of either pool, as one "group" of the strided call's kernels: its chunk sums lie behind those of the launches before
        const size_t s0 = std::min(c0, nsrc), y0 = std::min(c0, nsmp), at = s0 * nsc + y0 * nyc;
        AsxNccWs W = T;
        W.nsrc = (uint32_t)std::min(most, nsrc - s0);
        W.nsmp = (uint32_t)std::min(most, nsmp - y0);
        W.do_src = W.nsrc > 0;
        W.do_smp = W.nsmp > 0;
        W.table += s0 * (size_t)N;
        W.raw += at; W.m1 += at; W.m2 += at;
        W.sstat += s0 * ASX_NCC_STAT;
        W.ystat += y0 * ASX_NCC_STAT;
        asx_launch_ncc_moments(W, srcs + s0 * src_pitch, src_pitch, smps + y0 * smp_pitch, smp_pitch, N, s);
    }
}

void asx_launch_ncc_peak(const AsxNccWs &W, const float *r, size_t r_pitch, uint32_t N, double scale, double min_energy,
                         const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak, int npairs, hipStream_t s,
                         const AsxPoolPair *pl, int k)
{
    (void)hipMemsetAsync(W.best, 0, (size_t)npairs * sizeof(asx_peak_t), s);
    // a top-k group keeps the curve for its later passes: r_pitch >= 2N, and lags N..2N-1 of r are not read by any NCC kernel
    float *const c = k > 1 ? W.r + N : c_out;
    hipLaunchKernelGGL(k_ncc_peak, dim3(asx_ncc_chunks(N), npairs), dim3(NCC_NT), 0, s, W, r, r_pitch, N, scale, min_energy, rows, rows_step,
                       c, k > 1 ? r_pitch : (size_t)N, pl);
    if (k > 1) return;
    hipLaunchKernelGGL(k_ncc_finalize, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, W, N, rows, rows_step, seg, peak, npairs);
}

void asx_launch_ncctop_scan(const AsxNccWs &W, size_t r_pitch, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j,
                            int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_ncctop_scan, dim3(asx_ncc_chunks(N), npairs), dim3(NCC_NT), 0, s, W, r_pitch, N, rows, rows_step, sep, j);
}

void asx_launch_ncctop_step(const AsxNccWs &W, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j, int k, AsxSeg *seg,
                            const int64_t *tmp_lag, const double *tmp_coef, const int32_t *tmp_ret, int64_t *lag, double *coef,
                            double *peak, int32_t *ret, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_ncctop_step, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, W, N, rows, rows_step, sep, j, k, seg, tmp_lag,
                       tmp_coef, tmp_ret, lag, coef, peak, ret, npairs);
}

void asx_launch_ncc_invalid(uint32_t N, const int64_t *rows, size_t rows_step, int64_t *lag, double *coef, double *peak, int32_t *ret,
                            int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_ncc_invalid, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, N, rows, rows_step, lag, coef, peak, ret,
                       npairs);
}

// ---- the full range (asx_xcorr_ncc_full_f32_dev and its top-k form): the lags -(N-1)..N-1 ----------------------------------------
// The curve has 2N - 1 values, index i = l + N - 1.  Its upper half (l >= 0) is k_ncc_peak's in every bit: the same moment kernels on
// the same chunks, the same r32 (pass A) and the same expression.  A lag l < 0 overlaps in m = N + l = i + 1 frames, source[0, m)
// against sample[N - m, N), the reference's own segments; its r is rlo32[2N + l] of pass B, which ran on x_lo (AsxNccFullWs).
//   k_nccfull_stage    grid (vectors of a staged track, source tracks): x_lo = the first N frames, then zeros
//   k_nccfull_prefix   grid (2 chunks(N), tracks): block c of a source track starts from the chunk sums m1 / m2 of the chunks before c
//                      and scans its 2048 frames forwards -> {P1[m], Vx}; block c of a sample track starts from the chunks behind c and
//                      scans its frames backwards -> {T1[m], Vy}; thread, lanes, waves, as k_ncc_table scans
//   k_nccfull_peak     grid (chunks of the 2N - 1 indices, pairs): c32 of both halves, the row and the two competing rules, the packed
//                      (|c32|, smallest index) maximum; optionally the curve
//   k_nccfull_finalize / k_nccfull_invalid, k_nccfull_scan / k_nccfull_step: the tails of the one-lag and the top-k call in indices
// (k_nccfull_*, not k_ncc_*: see the note at k_ncctop_scan.)
// The pool calls (asx_xcorr_pool_ncc_full_f32_dev) run k_nccfull_stage and k_nccfull_prefix over the tracks of the two pools, once per
// call, into the plan's full-range track set (asx_launch_nccfull_pool_tracks: the same kernels against the same chunk sums, so the
// same tables), k_nccfp_peak finds a pair's tables and statistics through its pool record, and the tails, which read nothing of a
// track, are the strided call's kernels.
__global__ __launch_bounds__(NCC_NT) void k_nccfull_stage(AsxNccFullWs F, const float *__restrict__ src, size_t src_pitch, uint32_t N)
{
    const size_t v = (size_t)blockIdx.x * NCC_NT + threadIdx.x;
    if (4 * v >= F.pitch) return;
    const float *x = src + (size_t)blockIdx.y * src_pitch;
    const uint32_t f = (uint32_t)(4 * v);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f + 3 < N && ((uintptr_t)x & 15u) == 0) o = *reinterpret_cast<const float4 *>(x + f);
    else {
        if (f < N) o.x = x[f];
        if (f + 1 < N) o.y = x[f + 1];
        if (f + 2 < N) o.z = x[f + 2];
        if (f + 3 < N) o.w = x[f + 3];
    }
    *reinterpret_cast<float4 *>(F.stage + (size_t)blockIdx.y * F.pitch + f) = o;
}

__global__ __launch_bounds__(NCC_NT) void k_nccfull_prefix(AsxNccWs W, AsxNccFullWs F, const float *__restrict__ src, size_t src_pitch,
                                                            const float *__restrict__ smp, size_t smp_pitch, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    __shared__ float fr[ASX_NCC_CHUNK];
    const uint32_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), t = blockIdx.y;
    const bool back = blockIdx.x >= nyc; // a sample track: the suffix sums
    const uint32_t c = back ? blockIdx.x - nyc : blockIdx.x, f0 = c * ASX_NCC_CHUNK;
    if (back ? (t >= W.nsmp || !W.do_smp) : (t >= W.nsrc || !W.do_src)) return;
    const float *x = back ? smp + (size_t)t * smp_pitch : src + (size_t)t * src_pitch;
    const double mu = (back ? W.ystat : W.sstat)[(size_t)t * ASX_NCC_STAT];
    // the chunk's frames of the first N (zero past them), in scan order: a sample's chunk from its last frame down
#pragma unroll
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t i = j * NCC_NT + threadIdx.x, f = f0 + i;
        fr[back ? ASX_NCC_CHUNK - 1 - i : i] = f < N ? x[f] : 0.f;
    }
    // where the scan starts: the whole chunks in front of c (behind c), which lie inside the first N frames (a sample's last chunk
    // holds the sums of its own frames only)
    const size_t at = back ? (size_t)W.nsrc * nsc + (size_t)t * nyc + c + 1 : (size_t)t * nsc;
    double w1, w2;
    ncc_sum_arrays(W.m1 + at, W.m2 + at, back ? nyc - 1 - c : c, w1, w2, lds); // (its first barrier also puts fr in place)
    // the thread's eight consecutive places 8 tid + k: the inclusive prefix inside the thread, ...
    double p1[NCC_PER], p2[NCC_PER], t1 = 0.0, t2 = 0.0;
    const uint32_t j0 = threadIdx.x * NCC_PER;
#pragma unroll
    for (int k = 0; k < NCC_PER; k++) {
        const uint32_t f = back ? f0 + ASX_NCC_CHUNK - 1 - (j0 + k) : f0 + j0 + k;
        const double a = f < N ? (double)fr[j0 + k] - mu : 0.0;
        t1 += a;
        t2 += a * a;
        p1[k] = t1; p2[k] = t2;
    }
    // ... across the lanes (an inclusive scan of the threads' totals), across the waves
    double i1 = t1, i2 = t2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double u1 = __shfl_up(i1, off, 64), u2 = __shfl_up(i2, off, 64);
        if (lane >= off) { i1 += u1; i2 += u2; }
    }
    __syncthreads();
    if (lane == 63) { lds[wave] = i1; lds[NCC_NT / 64 + wave] = i2; }
    __syncthreads();
    double o1 = __shfl_up(i1, 1, 64), o2 = __shfl_up(i2, 1, 64); // exclusive in the wave
    if (lane == 0) { o1 = 0.0; o2 = 0.0; }
    for (int w = 0; w < wave; w++) { o1 += lds[w]; o2 += lds[NCC_NT / 64 + w]; }
    double2 *tab = (back ? F.ttab : F.ptab) + (size_t)t * N;
#pragma unroll
    for (int k = 0; k < NCC_PER; k++) {
        // the overlap whose sums end at this place: frames [0, f] of a source, [f, N) of a sample
        const uint32_t f = back ? f0 + ASX_NCC_CHUNK - 1 - (j0 + k) : f0 + j0 + k;
        const uint32_t m = back ? N - f : f + 1;
        if (f < N && m >= 1 && m < N) {
            const double s1 = w1 + (o1 + p1[k]), s2 = w2 + (o2 + p2[k]);
            tab[m] = make_double2(s1, s2 - s1 * s1 / (double)m);
        }
    }
}

// c_out: c32 of pair i's index j to c_out[i * c_pitch + j] (the debug call), or null.  keep: a top-k group -- c32 also goes to the
// halves of the pair's two r buffers that this kernel does not read (index j < N - 1 to rlo[j], the others to r[j + 1]).
// (the body of k_nccfull_peak and k_nccfp_peak: pair's tables and statistics are those of source track ts and sample track ty)
__device__ __forceinline__ void nccfull_peak_pair(const AsxNccWs &W, const AsxNccFullWs &F, size_t pair, size_t ts, size_t ty,
                                                  size_t r_pitch, uint32_t N, double scale, double min_energy, int64_t min_overlap,
                                                  const int64_t *__restrict__ rows, size_t rows_step, float *__restrict__ c_out,
                                                  size_t c_pitch, bool keep, asx_peak_t *red)
{
    const double *sx = W.sstat + ts * ASX_NCC_STAT, *sy = W.ystat + ty * ASX_NCC_STAT;
    const double mu = sx[0], floor_v = min_energy * sx[1], my = sy[0], Sy = sy[2], Vy = sy[3], dN = (double)N;
    const int64_t n1 = (int64_t)N - 1;
    int64_t lo = -n1, hi = n1;
    if (rows) {
        lo = rows[2 * pair * rows_step]; hi = rows[2 * pair * rows_step + 1];
        if (!asx_nccfull_row_ok(lo, hi, N)) { lo = 1; hi = 0; } // holds no lag
    }
    const double2 *tab = W.table + ts * N, *pt = F.ptab + ts * N, *tt = F.ttab + ty * N;
    float *ra = W.r + pair * r_pitch, *rl = F.rlo + pair * r_pitch;
    const uint32_t i0 = blockIdx.x * ASX_NCC_CHUNK, span = 2u * N - 1u;
    asx_peak_t best = 0;
#pragma unroll 2
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t i = i0 + j * NCC_NT + threadIdx.x;
        if (i >= span) break;
        double c;
        bool competes;
        if (i >= N - 1u) {
            // (k_ncc_peak's lines: the same bits)
            const uint32_t l = i - (N - 1u);
            const double2 e = tab[l];
            const double Sx = e.x + dN * mu;
            c = ((double)ra[l] / scale - Sx * Sy / dN) / sqrt(e.y * Vy);
            competes = Vy > 0.0 && e.y >= floor_v && fabs(c) <= 1.7976931348623157e308;
        } else {
            const uint32_t m = i + 1u; // the overlap; l = m - N, and r of its m products is at index 2N + l = N + m
            const double2 p = pt[m], q = tt[m];
            const double dm = (double)m, Sxl = p.x + dm * mu, Syl = q.x + dm * my, vv = p.y * q.y;
            c = ((double)rl[N + m] / scale - Sxl * Syl / dm) / sqrt(vv);
            competes = (int64_t)m >= min_overlap && Vy > 0.0 && vv >= floor_v * Vy && fabs(c) <= 1.7976931348623157e308;
        }
        const float c32 = (float)c;
        const float v = competes ? c32 : NAN;
        if (c_out) c_out[pair * c_pitch + i] = v;
        if (keep) { if (i < N - 1u) rl[i] = v; else ra[i + 1u] = v; }
        const int64_t l = (int64_t)i - n1;
        if (competes && l >= lo && l <= hi) best = peak_max(best, peak_pack_key(fabsf(c32), i));
    }
    best = block_peak_max(best, red);
    if (threadIdx.x == 0 && best) atomicMax(&W.best[pair], best);
}

__global__ __launch_bounds__(NCC_NT) void k_nccfull_peak(AsxNccWs W, AsxNccFullWs F, size_t r_pitch, uint32_t N, double scale,
                                                          double min_energy, int64_t min_overlap, const int64_t *__restrict__ rows,
                                                          size_t rows_step, float *__restrict__ c_out, size_t c_pitch, bool keep)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    nccfull_peak_pair(W, F, pair, W.nsrc > 1 ? pair : 0, W.nsmp > 1 ? pair : 0, r_pitch, N, scale, min_energy, min_overlap, rows,
                      rows_step, c_out, c_pitch, keep, red);
}

// The pool form (asx_xcorr_pool_ncc_full_f32_dev): W.table, W.sstat and W.ystat are the plan's NCC track set, F.ptab and F.ttab the
// full-range track set, and pair i's are those of its pool record's slots, as in k_ncc_peak; W.r, F.rlo and W.best are the group's.
// An invalid pair's record names slot 0 and its r is NaN: no lag competes.  (k_nccfp_*, not k_nccfull_*: tests/test_ncc_full.py holds
// that family to the seven kernels of the strided call.)
__global__ __launch_bounds__(NCC_NT) void k_nccfp_peak(AsxNccWs W, AsxNccFullWs F, size_t r_pitch, uint32_t N, double scale,
                                                        double min_energy, int64_t min_overlap, const int64_t *__restrict__ rows,
                                                        size_t rows_step, bool keep, const AsxPoolPair *__restrict__ pl)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    nccfull_peak_pair(W, F, pair, pl[pair].sx, pl[pair].sy, r_pitch, N, scale, min_energy, min_overlap, rows, rows_step, nullptr, 0, keep,
                      red);
}

// the segment of the curve's index i: the lag l = i - (N - 1) as the circular index the windowed call would have found it at
__device__ __forceinline__ AsxSeg nccfull_seg(uint32_t i, uint32_t N) { return make_seg(i >= N - 1u ? i - (N - 1u) : N + 1u + i, N); }

__global__ __launch_bounds__(NCC_NT) void k_nccfull_finalize(AsxNccWs W, uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                              AsxSeg *__restrict__ seg, double *__restrict__ peak, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    const asx_peak_t best = W.best[pair];
    uint32_t first = 0; // no lag competes: the row's lag_min (an invalid row: the first lag, and k_nccfull_invalid writes its results)
    if (rows) {
        const int64_t lo = rows[2 * (size_t)pair * rows_step], hi = rows[2 * (size_t)pair * rows_step + 1];
        if (asx_nccfull_row_ok(lo, hi, N)) first = (uint32_t)(lo + (int64_t)N - 1);
    }
    seg[pair] = nccfull_seg(best ? peak_index(best) : first, N);
    peak[pair] = best ? (double)peak_key(best) : 0.0;
}

__global__ __launch_bounds__(NCC_NT) void k_nccfull_invalid(uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                             int64_t *__restrict__ lag, double *__restrict__ coef,
                                                             double *__restrict__ peak, int32_t *__restrict__ ret, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    if (asx_nccfull_row_ok(rows[2 * (size_t)pair * rows_step], rows[2 * (size_t)pair * rows_step + 1], N)) return;
    if (lag) lag[pair] = 0;
    coef[pair] = (double)NAN;
    peak[pair] = (double)NAN;
    ret[pair] = -2;
}

// k_ncctop_scan over the 2N - 1 indices: the record's lags are indices, and a zone is clipped at the curve's two ends (no wrap)
__global__ __launch_bounds__(NCC_NT) void k_nccfull_scan(AsxNccWs W, AsxNccFullWs F, size_t r_pitch, uint32_t N,
                                                          const int64_t *__restrict__ rows, size_t rows_step, int64_t sep, int j)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    const AsxNccTopk *T = W.tk + pair;
    if (T->flags) return; // (the whole block: an invalid row, or no lag was left for an earlier entry)
    const uint32_t span = 2u * N - 1u;
    int64_t lo = 0, hi = (int64_t)span - 1;
    if (rows) { lo = rows[2 * pair * rows_step] + (int64_t)N - 1; hi = rows[2 * pair * rows_step + 1] + (int64_t)N - 1; }
    uint32_t zlo[ASX_TOPK_MAX - 1], zwd[ASX_TOPK_MAX - 1];
#pragma unroll
    for (int i = 0; i < ASX_TOPK_MAX - 1; i++) {
        zlo[i] = ~0u; zwd[i] = 0u;
        if (i < j) ncctop_zone(T->lag[i], sep, span, zlo[i], zwd[i]);
    }
    const float *ca = W.r + pair * r_pitch + 1, *cl = F.rlo + pair * r_pitch;
    const uint32_t i0 = blockIdx.x * ASX_NCC_CHUNK;
    asx_peak_t best = 0;
#pragma unroll 2
    for (int q = 0; q < NCC_PER; q++) {
        const uint32_t l = i0 + q * NCC_NT + threadIdx.x;
        if (l >= span) break;
        const float v = l < N - 1u ? cl[l] : ca[l];
        bool in = v == v && (int64_t)l >= lo && (int64_t)l <= hi;
#pragma unroll
        for (int i = 0; i < ASX_TOPK_MAX - 1; i++) in = in && l - zlo[i] > zwd[i];
        if (in) best = peak_max(best, peak_pack_key(fabsf(v), l));
    }
    best = block_peak_max(best, red);
    if (threadIdx.x == 0 && best) atomicMax(&W.best[pair], best);
}

// k_ncctop_step in indices
__global__ __launch_bounds__(NCC_NT) void k_nccfull_step(AsxNccWs W, uint32_t N, const int64_t *__restrict__ rows, size_t rows_step,
                                                          int64_t sep, int j, int k, AsxSeg *__restrict__ seg,
                                                          const int64_t *__restrict__ tmp_lag, const double *__restrict__ tmp_coef,
                                                          const int32_t *__restrict__ tmp_ret, int64_t *__restrict__ lag,
                                                          double *__restrict__ coef, double *__restrict__ peak, int32_t *__restrict__ ret,
                                                          int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    AsxNccTopk *T = W.tk + pair;
    const uint32_t span = 2u * N - 1u;
    int64_t lo = 0, hi = (int64_t)span - 1;
    bool row_ok = true;
    if (rows) {
        const int64_t a = rows[2 * (size_t)pair * rows_step], b = rows[2 * (size_t)pair * rows_step + 1];
        row_ok = asx_nccfull_row_ok(a, b, N);
        if (row_ok) { lo = a + (int64_t)N - 1; hi = b + (int64_t)N - 1; }
    }
    uint32_t n = 0, flags = 0;
    if (j == 0) { if (!row_ok) flags = ASX_NCC_TK_INVALID; }
    else { n = T->n; flags = T->flags; }
    if (j > 0) {
        const size_t e = (size_t)pair * (size_t)k + (size_t)(j - 1);
        const bool none = flags & ASX_NCC_TK_INVALID || n < (uint32_t)j; // n < j: no lag was left for this entry
        if (lag) lag[e] = none ? 0 : tmp_lag[pair];
        coef[e] = none ? (double)NAN : tmp_coef[pair];
        peak[e] = none ? (double)NAN : T->peak;
        ret[e] = flags & ASX_NCC_TK_INVALID ? -2 : none ? -3 : tmp_ret[pair];
    }
    if (j >= k) return;
    const asx_peak_t best = W.best[pair];
    W.best[pair] = 0;
    uint32_t at = N - 1u; // (an entry that is not to be: lag 0's segment, whose coefficient the next step drops)
    if (!flags) {
        double height = 0.0;
        bool have = true;
        if (best) { at = peak_index(best); height = (double)peak_key(best); }
        else {
            // no lag of A_j competes: its smallest lag, the row's lag_min pushed past every zone that holds it
            int64_t cand = lo;
            for (int round = 0; round <= j; round++) {
                bool moved = false;
                for (int i = 0; i < j; i++) {
                    uint32_t zlo, zwd;
                    ncctop_zone(T->lag[i], sep, span, zlo, zwd);
                    if (cand >= (int64_t)zlo && cand <= (int64_t)zlo + (int64_t)zwd) { cand = (int64_t)zlo + (int64_t)zwd + 1; moved = true; }
                }
                if (!moved) break;
            }
            have = cand <= hi;
            if (have) at = (uint32_t)cand;
        }
        if (have) { T->lag[j] = (int64_t)at; T->peak = height; n = (uint32_t)j + 1u; }
        else flags = ASX_NCC_TK_EMPTY;
    }
    T->n = n;
    T->flags = flags;
    seg[pair] = nccfull_seg(at, N);
}

void asx_launch_nccfull_stage(const AsxNccFullWs &F, const float *src, size_t src_pitch, uint32_t nsrc, uint32_t N, hipStream_t s)
{
    const unsigned nv = (unsigned)(F.pitch / 4);
    hipLaunchKernelGGL(k_nccfull_stage, dim3((nv + NCC_NT - 1) / NCC_NT, nsrc), dim3(NCC_NT), 0, s, F, src, src_pitch, N);
}

void asx_launch_nccfull_prefix(const AsxNccWs &W, const AsxNccFullWs &F, const float *src, size_t src_pitch, const float *smp,
                               size_t smp_pitch, uint32_t N, hipStream_t s)
{
    if (!W.do_src && !W.do_smp) return;
    const unsigned nyc = asx_ncc_chunks(N), nt = W.nsrc > W.nsmp ? W.nsrc : W.nsmp;
    hipLaunchKernelGGL(k_nccfull_prefix, dim3(2 * nyc, nt), dim3(NCC_NT), 0, s, W, F, src, src_pitch, smp, smp_pitch, N);
}

void asx_launch_nccfull_peak(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, double scale, double min_energy,
                             int64_t min_overlap, const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak,
                             int npairs, hipStream_t s, int k)
{
    (void)hipMemsetAsync(W.best, 0, (size_t)npairs * sizeof(asx_peak_t), s);
    hipLaunchKernelGGL(k_nccfull_peak, dim3(asx_ncc_chunks(2u * N - 1u), npairs), dim3(NCC_NT), 0, s, W, F, r_pitch, N, scale, min_energy,
                       min_overlap, rows, rows_step, c_out, (size_t)(2u * N - 1u), k > 1);
    if (k > 1) return;
    hipLaunchKernelGGL(k_nccfull_finalize, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, W, N, rows, rows_step, seg, peak, npairs);
}

void asx_launch_nccfull_pool_tracks(const AsxNccWs &T, const AsxNccFullWs &F, const float *srcs, size_t src_pitch, size_t nsrc,
                                    const float *smps, size_t smp_pitch, size_t nsmp, uint32_t N, hipStream_t s)
{
    const size_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N), most = 65535;
    for (size_t c0 = 0; c0 < std::max(nsrc, nsmp); c0 += most) {
        // asx_launch_ncc_pool_moments' shares: the chunk sums of tracks c0 .. lie where that launch left them
        const size_t s0 = std::min(c0, nsrc), y0 = std::min(c0, nsmp), at = s0 * nsc + y0 * nyc;
        AsxNccWs W = T;
        W.nsrc = (uint32_t)std::min(most, nsrc - s0);
        W.nsmp = (uint32_t)std::min(most, nsmp - y0);
        W.do_src = W.nsrc > 0;
        W.do_smp = W.nsmp > 0;
        W.m1 += at; W.m2 += at;
        W.sstat += s0 * ASX_NCC_STAT;
        W.ystat += y0 * ASX_NCC_STAT;
        AsxNccFullWs G = F;
        G.stage += s0 * F.pitch;
        G.ptab += s0 * (size_t)N;
        G.ttab += y0 * (size_t)N;
        if (W.do_src) asx_launch_nccfull_stage(G, srcs + s0 * src_pitch, src_pitch, W.nsrc, N, s);
        asx_launch_nccfull_prefix(W, G, srcs + s0 * src_pitch, src_pitch, smps + y0 * smp_pitch, smp_pitch, N, s);
    }
}

void asx_launch_nccfp_peak(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, double scale, double min_energy,
                           int64_t min_overlap, const int64_t *rows, size_t rows_step, AsxSeg *seg, double *peak, int npairs,
                           hipStream_t s, const AsxPoolPair *pl, int k)
{
    (void)hipMemsetAsync(W.best, 0, (size_t)npairs * sizeof(asx_peak_t), s);
    hipLaunchKernelGGL(k_nccfp_peak, dim3(asx_ncc_chunks(2u * N - 1u), npairs), dim3(NCC_NT), 0, s, W, F, r_pitch, N, scale, min_energy,
                       min_overlap, rows, rows_step, k > 1, pl);
    if (k > 1) return;
    hipLaunchKernelGGL(k_nccfull_finalize, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, W, N, rows, rows_step, seg, peak, npairs);
}

void asx_launch_nccfull_scan(const AsxNccWs &W, const AsxNccFullWs &F, size_t r_pitch, uint32_t N, const int64_t *rows, size_t rows_step,
                             int64_t sep, int j, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_nccfull_scan, dim3(asx_ncc_chunks(2u * N - 1u), npairs), dim3(NCC_NT), 0, s, W, F, r_pitch, N, rows, rows_step, sep, j);
}

void asx_launch_nccfull_step(const AsxNccWs &W, uint32_t N, const int64_t *rows, size_t rows_step, int64_t sep, int j, int k, AsxSeg *seg,
                             const int64_t *tmp_lag, const double *tmp_coef, const int32_t *tmp_ret, int64_t *lag, double *coef,
                             double *peak, int32_t *ret, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_nccfull_step, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, W, N, rows, rows_step, sep, j, k, seg, tmp_lag,
                       tmp_coef, tmp_ret, lag, coef, peak, ret, npairs);
}

void asx_launch_nccfull_invalid(uint32_t N, const int64_t *rows, size_t rows_step, int64_t *lag, double *coef, double *peak,
                                int32_t *ret, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_nccfull_invalid, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, N, rows, rows_step, lag, coef, peak, ret,
                       npairs);
}

// ---- ragged tracks (asx_xcorr_ncc_ragged_f32_dev and its top-k form): pair i holds Ls <= 2N source and Lm <= N sample frames ---------
// The curve is the full-range call's in shape: 2N - 1 values, index i = l + N - 1, so the row rule, the zones, k_nccfull_scan and
// k_nccfull_step and the places where a top-k group keeps the curve are that call's.  What differs is what a lag's moments are taken
// over: sample frames [n0, n1) = [max(0, -l), min(Lm, Ls - l)) against source frames [n0 + l, n1 + l), m = n1 - n0 of them (m <= 0:
// the lag does not exist), from prefix tables over the frames that count, about the means of those frames.  Frames at and beyond a
// length are never read: the kernels below read the caller's tracks once (k_nccrag_stage) and then the staged copies, whose tails
// are zero, and the two transform passes read only those (pass A: x', pass B: x_lo').  Every pair is staged and summed by itself, a
// broadcast track too: each pair may cut it differently.  The trees are fixed by N and the pair's lengths.
//   k_nccrag_stage     grid (source chunks + sample chunks, pairs): x', x_lo' and y' of the chunk, its plain sum
//   k_nccrag_moments   same grid: the mean over [0, len) from the chunk sums, then sum (x - mu) and sum (x - mu)^2 of the chunk
//   k_nccrag_prefix    same grid: block c starts from the chunk sums in front of c and scans its frames -> {PA1, PA2}[j], j <= len
//   k_nccrag_vmax      grid (chunks(N), pairs): the largest energy of a window x[j, j + w), w = min(Ls, Lm) (atomic maximum)
//   k_nccrag_peak      grid (chunks of the 2N - 1 indices, pairs): c32, the row and the competing rule, the packed maximum
//   k_nccrag_finalize / k_nccrag_seg / k_nccrag_invalid: a thread per pair -- the winner's (a top-k entry's) segment, the -5 rows
// (k_nccrag_*, not k_nccfull_*: see the note at k_nccfp_peak.)
#define NCCRAG_VEC (ASX_NCC_CHUNK / 4 / NCC_NT)
static_assert(NCCRAG_VEC == 2, "two 16-byte vectors of a chunk per thread");

// which track and chunk a block of the grid (source chunks + sample chunks, pairs) owns
struct NccRagChunk {
    bool src;
    uint32_t len, c, nc, f0; // the track's length, the block's chunk, the track's chunks, the chunk's first frame
    size_t slot;             // where the chunk's sums go in raw / m1 / m2
};
__device__ __forceinline__ NccRagChunk nccrag_chunk_of(const AsxRagLens &L, uint32_t N)
{
    const uint32_t nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N);
    uint32_t Ls, Lm;
    asx_nccrag_lens(L, blockIdx.y, N, Ls, Lm);
    NccRagChunk k;
    k.src = blockIdx.x < nsc;
    k.c = k.src ? blockIdx.x : blockIdx.x - nsc;
    k.nc = k.src ? nsc : nyc;
    k.len = k.src ? Ls : Lm;
    k.f0 = k.c * ASX_NCC_CHUNK;
    k.slot = (size_t)blockIdx.y * (nsc + nyc) + blockIdx.x;
    return k;
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_stage(AsxNccRagWs R, AsxRagLens L, const float *__restrict__ src, size_t src_pitch,
                                                          const float *__restrict__ smp, size_t smp_pitch, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    const NccRagChunk k = nccrag_chunk_of(L, N);
    const size_t pair = blockIdx.y, pitch = k.src ? R.xpitch : R.ypitch;
    const float *x = k.src ? src + pair * src_pitch : smp + pair * smp_pitch;
    float *out = (k.src ? R.xs : R.ys) + pair * pitch;
    const bool vec = ((uintptr_t)x & 15u) == 0;
    double s = 0.0, z = 0.0;
#pragma unroll
    for (int j = 0; j < NCCRAG_VEC; j++) {
        const uint32_t f = k.f0 + 4u * (j * NCC_NT + threadIdx.x);
        if (f >= pitch) continue; // (the pitch is a whole number of vectors)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec && f + 3 < k.len) v = *reinterpret_cast<const float4 *>(x + f);
        else {
            if (f < k.len) v.x = x[f];
            if (f + 1 < k.len) v.y = x[f + 1];
            if (f + 2 < k.len) v.z = x[f + 2];
            if (f + 3 < k.len) v.w = x[f + 3];
        }
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        *reinterpret_cast<float4 *>(out + f) = v;
        if (k.src) {
            if (f >= N) v.x = 0.f;
            if (f + 1 >= N) v.y = 0.f;
            if (f + 2 >= N) v.z = 0.f;
            if (f + 3 >= N) v.w = 0.f;
            *reinterpret_cast<float4 *>(R.xlo + pair * pitch + f) = v;
        }
    }
    ncc_block_sum2(s, z, lds);
    if (threadIdx.x == 0) {
        R.raw[k.slot] = s;
        if (blockIdx.x == 0) R.stat[pair * ASX_NCC_STAT + 1] = 0.0; // Vmax, which k_nccrag_vmax raises
    }
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_moments(AsxNccRagWs R, AsxRagLens L, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    const NccRagChunk k = nccrag_chunk_of(L, N);
    const size_t pair = blockIdx.y, pitch = k.src ? R.xpitch : R.ypitch;
    const float *x = (k.src ? R.xs : R.ys) + pair * pitch;
    double tot, z;
    ncc_sum_arrays(R.raw + (k.slot - k.c), nullptr, k.nc, tot, z, lds);
    const double mu = k.len ? tot / (double)k.len : 0.0;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < NCCRAG_VEC; j++) {
        const uint32_t f = k.f0 + 4u * (j * NCC_NT + threadIdx.x);
        if (f >= k.len) continue; // (f < len <= pitch: the vector lies inside the staged track)
        const float4 v = *reinterpret_cast<const float4 *>(x + f);
        const float e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (f + q < k.len) { const double a = (double)e[q] - mu; s1 += a; s2 += a * a; }
    }
    ncc_block_sum2(s1, s2, lds);
    if (threadIdx.x == 0) {
        R.m1[k.slot] = s1;
        R.m2[k.slot] = s2;
        if (k.c == 0) R.stat[pair * ASX_NCC_STAT + (k.src ? 0 : 2)] = mu;
    }
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_prefix(AsxNccRagWs R, AsxRagLens L, uint32_t N)
{
    __shared__ double lds[2 * (NCC_NT / 64)];
    const NccRagChunk k = nccrag_chunk_of(L, N);
    const size_t pair = blockIdx.y, pitch = k.src ? R.xpitch : R.ypitch;
    const float *x = (k.src ? R.xs : R.ys) + pair * pitch;
    const double mu = R.stat[pair * ASX_NCC_STAT + (k.src ? 0 : 2)];
    // where the scan starts: the whole chunks in front of c
    double w1, w2;
    ncc_sum_arrays(R.m1 + (k.slot - k.c), R.m2 + (k.slot - k.c), k.c, w1, w2, lds);
    // the thread's eight consecutive frames f .. f + 7: the inclusive prefix inside the thread, ...
    const uint32_t f = k.f0 + threadIdx.x * NCC_PER;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
    if (f < k.len) u = *reinterpret_cast<const float4 *>(x + f);
    if (f + 4 < k.len) v = *reinterpret_cast<const float4 *>(x + f + 4);
    const float e[NCC_PER] = { u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w };
    double p1[NCC_PER], p2[NCC_PER], t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int q = 0; q < NCC_PER; q++) {
        const double a = f + q < k.len ? (double)e[q] - mu : 0.0;
        t1 += a;
        t2 += a * a;
        p1[q] = t1; p2[q] = t2;
    }
    // ... across the lanes (an inclusive scan of the threads' totals), across the waves: k_nccfull_prefix's order
    double i1 = t1, i2 = t2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double u1 = __shfl_up(i1, off, 64), u2 = __shfl_up(i2, off, 64);
        if (lane >= off) { i1 += u1; i2 += u2; }
    }
    __syncthreads();
    if (lane == 63) { lds[wave] = i1; lds[NCC_NT / 64 + wave] = i2; }
    __syncthreads();
    double o1 = __shfl_up(i1, 1, 64), o2 = __shfl_up(i2, 1, 64); // exclusive in the wave
    if (lane == 0) { o1 = 0.0; o2 = 0.0; }
    for (int w = 0; w < wave; w++) { o1 += lds[w]; o2 += lds[NCC_NT / 64 + w]; }
    double2 *tab = k.src ? R.pa + pair * (2 * (size_t)N + 1) : R.pb + pair * ((size_t)N + 1);
#pragma unroll
    for (int q = 0; q < NCC_PER; q++)
        if (f + q < k.len) tab[f + q + 1] = make_double2(w1 + (o1 + p1[q]), w2 + (o2 + p2[q])); // (f + q + 1 <= len: inside the table)
    if (k.c == 0 && threadIdx.x == 0) tab[0] = make_double2(0.0, 0.0);
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_vmax(AsxNccRagWs R, AsxRagLens L, uint32_t N)
{
    const size_t pair = blockIdx.y;
    uint32_t Ls, Lm;
    if (!asx_nccrag_lens(L, pair, N, Ls, Lm)) return;
    // the windows x[j, j + w), 0 <= j <= min(Ls - w, N - 1): j + w <= Ls, inside the table
    const uint32_t w = Ls < Lm ? Ls : Lm, jmax = Ls - w < N - 1u ? Ls - w : N - 1u;
    const double2 *pa = R.pa + pair * (2 * (size_t)N + 1);
    const double dw = (double)w;
    double vmax = 0.0;
#pragma unroll 2
    for (int q = 0; q < NCC_PER; q++) {
        const uint32_t j = blockIdx.x * ASX_NCC_CHUNK + q * NCC_NT + threadIdx.x;
        if (j > jmax) break;
        const double2 a0 = pa[j], a1 = pa[j + w];
        const double s1 = a1.x - a0.x;
        vmax = fmax(vmax, (a1.y - a0.y) - s1 * s1 / dw); // (a NaN drops out)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, off, 64));
    // non-negative doubles order as their bits do
    if ((threadIdx.x & 63) == 0 && vmax > 0.0)
        atomicMax(reinterpret_cast<unsigned long long *>(R.stat + pair * ASX_NCC_STAT + 1), (unsigned long long)__double_as_longlong(vmax));
}

// the overlap of the curve's index i in the caller's tracks (no frames: an empty segment, whose coefficient is NaN)
__device__ __forceinline__ AsxSeg nccrag_seg(uint32_t i, uint32_t N, uint32_t Ls, uint32_t Lm)
{
    const int64_t l = (int64_t)i - ((int64_t)N - 1), n0 = l < 0 ? -l : 0, n1 = min((int64_t)Lm, (int64_t)Ls - l);
    AsxSeg s;
    s.lag = l;
    s.peak = i >= N - 1u ? i - (N - 1u) : N + 1u + i;
    s.flags = 0;
    s.src_off = s.smp_off = s.len = 0;
    if (n1 > n0) { s.src_off = (uint32_t)(n0 + l); s.smp_off = (uint32_t)n0; s.len = (uint32_t)(n1 - n0); }
    return s;
}

// c_out and keep: as in k_nccfull_peak
__global__ __launch_bounds__(NCC_NT) void k_nccrag_peak(AsxNccRagWs R, AsxRagLens L, size_t r_pitch, uint32_t N, double scale,
                                                         double min_energy, int64_t min_overlap, const int64_t *__restrict__ rows,
                                                         size_t rows_step, float *__restrict__ c_out, size_t c_pitch, bool keep)
{
    __shared__ asx_peak_t red[NCC_NT / 64];
    const size_t pair = blockIdx.y;
    uint32_t Ls, Lm;
    asx_nccrag_lens(L, pair, N, Ls, Lm); // (not a pair of lengths: (0, 0), no lag exists)
    const double *st = R.stat + pair * ASX_NCC_STAT;
    const double mu = st[0], my = st[2];
    const double2 *pa = R.pa + pair * (2 * (size_t)N + 1), *pb = R.pb + pair * ((size_t)N + 1);
    double Vy = 0.0;
    if (Lm) { const double2 e = pb[Lm]; Vy = e.y - e.x * e.x / (double)Lm; }
    const double floor_v = min_energy * st[1] * Vy;
    const int64_t need = min(min_overlap, (int64_t)min(Ls, Lm));
    const int64_t n1 = (int64_t)N - 1;
    int64_t lo = -n1, hi = n1;
    if (rows) {
        lo = rows[2 * pair * rows_step]; hi = rows[2 * pair * rows_step + 1];
        if (!asx_nccfull_row_ok(lo, hi, N)) { lo = 1; hi = 0; } // holds no lag
    }
    float *ra = R.r + pair * r_pitch, *rl = R.rlo + pair * r_pitch;
    const uint32_t i0 = blockIdx.x * ASX_NCC_CHUNK, span = 2u * N - 1u;
    asx_peak_t best = 0;
#pragma unroll 2
    for (int j = 0; j < NCC_PER; j++) {
        const uint32_t i = i0 + j * NCC_NT + threadIdx.x;
        if (i >= span) break;
        const int64_t l = (int64_t)i - n1, f0 = l < 0 ? -l : 0, f1 = min((int64_t)Lm, (int64_t)Ls - l), m = f1 - f0;
        float c32 = NAN;
        bool competes = false;
        if (m > 0) {
            // 0 <= f0 + l < f1 + l <= Ls and 0 <= f0 < f1 <= Lm: inside the tables; r of lag l >= 0 at ra[l], of l < 0 at rl[2N + l]
            const double2 a0 = pa[f0 + l], a1 = pa[f1 + l], b0 = pb[f0], b1 = pb[f1];
            const double dm = (double)m, s1x = a1.x - a0.x, s1y = b1.x - b0.x;
            const double vx = (a1.y - a0.y) - s1x * s1x / dm, vy = (b1.y - b0.y) - s1y * s1y / dm, vv = vx * vy;
            const double Sx = s1x + dm * mu, Sy = s1y + dm * my;
            const double r32 = (double)(l >= 0 ? ra[l] : rl[2 * (int64_t)N + l]);
            const double c = (r32 / scale - Sx * Sy / dm) / sqrt(vv);
            c32 = (float)c;
            competes = m >= need && Vy > 0.0 && vv >= floor_v && fabs(c) <= 1.7976931348623157e308;
        }
        const float v = competes ? c32 : NAN;
        if (c_out) c_out[pair * c_pitch + i] = v;
        if (keep) { if (i < N - 1u) rl[i] = v; else ra[i + 1u] = v; }
        if (competes && l >= lo && l <= hi) best = peak_max(best, peak_pack_key(fabsf(c32), i));
    }
    best = block_peak_max(best, red);
    if (threadIdx.x == 0 && best) atomicMax(&R.best[pair], best);
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_finalize(AsxNccRagWs R, AsxRagLens L, uint32_t N, const int64_t *__restrict__ rows,
                                                             size_t rows_step, AsxSeg *__restrict__ seg, double *__restrict__ peak,
                                                             int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    uint32_t Ls, Lm;
    asx_nccrag_lens(L, (size_t)pair, N, Ls, Lm);
    const asx_peak_t best = R.best[pair];
    uint32_t first = 0; // no lag competes: the row's lag_min (a row that is none: the first lag, and the invalid kernels write its results)
    if (rows) {
        const int64_t lo = rows[2 * (size_t)pair * rows_step], hi = rows[2 * (size_t)pair * rows_step + 1];
        if (asx_nccfull_row_ok(lo, hi, N)) first = (uint32_t)(lo + (int64_t)N - 1);
    }
    seg[pair] = nccrag_seg(best ? peak_index(best) : first, N, Ls, Lm);
    peak[pair] = best ? (double)peak_key(best) : 0.0;
}

// behind k_nccfull_step(j), which left the full-range call's segment of entry j: the ragged one, or an empty one where the record
// holds no entry j (its coefficient is dropped by the next step)
__global__ __launch_bounds__(NCC_NT) void k_nccrag_seg(AsxNccRagWs R, AsxRagLens L, uint32_t N, int j, AsxSeg *__restrict__ seg, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    uint32_t Ls, Lm;
    asx_nccrag_lens(L, (size_t)pair, N, Ls, Lm);
    const AsxNccTopk *T = R.tk + pair;
    const bool have = !T->flags && T->n == (uint32_t)j + 1u;
    seg[pair] = have ? nccrag_seg((uint32_t)T->lag[j], N, Ls, Lm) : nccrag_seg(N - 1u, N, 0u, 0u);
}

__global__ __launch_bounds__(NCC_NT) void k_nccrag_invalid(AsxRagLens L, uint32_t N, int k, int64_t *__restrict__ lag,
                                                            double *__restrict__ coef, double *__restrict__ peak,
                                                            int32_t *__restrict__ ret, int npairs)
{
    const int pair = blockIdx.x * NCC_NT + threadIdx.x;
    if (pair >= npairs) return;
    uint32_t Ls, Lm;
    if (asx_nccrag_lens(L, (size_t)pair, N, Ls, Lm)) return;
    for (int j = 0; j < k; j++) {
        const size_t e = (size_t)pair * (size_t)k + (size_t)j;
        if (lag) lag[e] = 0;
        coef[e] = (double)NAN;
        peak[e] = (double)NAN;
        ret[e] = -5;
    }
}

void asx_launch_nccrag_tracks(const AsxNccRagWs &R, const AsxRagLens &L, const float *src, size_t src_pitch, const float *smp,
                              size_t smp_pitch, uint32_t N, int npairs, hipStream_t s)
{
    const unsigned nsc = asx_ncc_chunks(2u * N), nyc = asx_ncc_chunks(N);
    hipLaunchKernelGGL(k_nccrag_stage, dim3(nsc + nyc, npairs), dim3(NCC_NT), 0, s, R, L, src, src_pitch, smp, smp_pitch, N);
    hipLaunchKernelGGL(k_nccrag_moments, dim3(nsc + nyc, npairs), dim3(NCC_NT), 0, s, R, L, N);
    hipLaunchKernelGGL(k_nccrag_prefix, dim3(nsc + nyc, npairs), dim3(NCC_NT), 0, s, R, L, N);
    hipLaunchKernelGGL(k_nccrag_vmax, dim3(nyc, npairs), dim3(NCC_NT), 0, s, R, L, N);
}

void asx_launch_nccrag_peak(const AsxNccRagWs &R, const AsxRagLens &L, uint32_t N, double scale, double min_energy, int64_t min_overlap,
                            const int64_t *rows, size_t rows_step, float *c_out, AsxSeg *seg, double *peak, int npairs, hipStream_t s,
                            int k)
{
    (void)hipMemsetAsync(R.best, 0, (size_t)npairs * sizeof(asx_peak_t), s);
    hipLaunchKernelGGL(k_nccrag_peak, dim3(asx_ncc_chunks(2u * N - 1u), npairs), dim3(NCC_NT), 0, s, R, L, (size_t)(2u * N), N, scale,
                       min_energy, min_overlap, rows, rows_step, c_out, (size_t)(2u * N - 1u), k > 1);
    if (k > 1) return;
    hipLaunchKernelGGL(k_nccrag_finalize, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, R, L, N, rows, rows_step, seg, peak,
                       npairs);
}

void asx_launch_nccrag_seg(const AsxNccRagWs &R, const AsxRagLens &L, uint32_t N, int j, AsxSeg *seg, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_nccrag_seg, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, R, L, N, j, seg, npairs);
}

void asx_launch_nccrag_invalid(const AsxRagLens &L, uint32_t N, int k, int64_t *lag, double *coef, double *peak, int32_t *ret, int npairs,
                               hipStream_t s)
{
    hipLaunchKernelGGL(k_nccrag_invalid, dim3((npairs + NCC_NT - 1) / NCC_NT), dim3(NCC_NT), 0, s, L, N, k, lag, coef, peak, ret, npairs);
}
