// csrc/place.hip — placement of a clip pool over chains of usable pairs (asx_pool_place_dev): the k_place_* kernels, which read the
// picked tables of asx_pool_closure_dev (L = best_lag, R = best_ret, F = confirm, [C][C], pair (a, b) at a * C + b) and the root from
// device memory.  Everything is int64 sums and integer counts; a clip's median is the rank-counting one of closure_dev.h over
// estimates that are never stored, so no output depends on the launch geometry.
//   k_place_init     a thread per clip: hops (0 for the root, -1 otherwise), offset 0 in the buffer the layers work in, step 0, and
//                    the frontier word
//   k_place_layer    one launch per layer h = 1 .. max_hops, a block per clip b.  A clip counts as placed when 0 <= hops[c] < h, so
//                    a hops[c] = h that another block writes meanwhile reads as "not placed" whether it is seen or not, and so does
//                    the -1 it replaces: offsets and hops need no second buffer.  A block whose clip is reached exits at once.
//   k_place_sweep    one launch per sweep, a block per clip: the median over ALL reached neighbours, read from one buffer and
//                    written to the other (Jacobi); the launcher starts the layers in the buffer that makes the last sweep end in
//                    d_offset
//   k_place_verdict  a block per clip b: degree and support of b, then resid and state of the pairs (b, .)
// No kernel waits for another block.  The frontier word is d_degree[0] until k_place_verdict overwrites it: the largest layer that
// placed a clip, -1 when the root is no clip.  A layer that places nothing leaves it behind, and every block of a later layer reads
// that and leaves.  Its value at the start of launch h decides: it is below h - 1 exactly when layer h - 1 placed nothing, then no
// block of layer h goes on and none raises it, so a stale or a fresh read give the same answer; at h - 1 or above every block goes on.
#include "asx_internal.h"
#include "closure_dev.h"

// Clip b's estimates of T_b - T_root through the clips c that THIS thread takes and that count as placed (0 <= hops[c] < before),
// each handed to fn: o[c] + L_cb where (c, b) is usable, o[c] - L_bc where (b, c) is (closure_usable is false for c == b)
template <typename Fn>
__device__ __forceinline__ void place_estimates(const int64_t *L, const int32_t *R, const int32_t *F, uint32_t C, int min_confirm,
                                                const int32_t *hops, const int64_t *o, int32_t before, uint32_t b, Fn &&fn)
{
    for (uint32_t c = threadIdx.x; c < C; c += ASX_THREADS) {
        const int32_t hc = hops[c];
        if (hc < 0 || hc >= before) continue;
        const int64_t oc = o[c];
        if (closure_usable(L, R, F, C, min_confirm, c, b)) fn(oc + L[c * C + b]);
        if (closure_usable(L, R, F, C, min_confirm, b, c)) fn(oc - L[b * C + c]);
    }
}

__global__ __launch_bounds__(ASX_THREADS) void k_place_init(const int32_t *__restrict__ root, uint32_t C, int32_t *__restrict__ hops,
                                                             int64_t *__restrict__ o, int64_t *__restrict__ step,
                                                             int32_t *__restrict__ frontier)
{
    const uint32_t b = blockIdx.x * ASX_THREADS + threadIdx.x;
    const int32_t r = root[0];
    const bool is_clip = r >= 0 && (uint32_t)r < C;
    if (b == 0) frontier[0] = is_clip ? 0 : -1;
    if (b >= C) return;
    hops[b] = is_clip && b == (uint32_t)r ? 0 : -1;
    o[b] = 0;
    step[b] = 0;
}

// (hops and o are read and written through one pointer each: other blocks write elements that this one reads)
__global__ __launch_bounds__(ASX_THREADS) void k_place_layer(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                              const int32_t *__restrict__ F, uint32_t C, int min_confirm, int32_t h,
                                                              int32_t *hops, int64_t *o, int32_t *frontier)
{
    __shared__ ClosureLds sh;
    __shared__ int32_t go;
    const uint32_t b = blockIdx.x;
    if (threadIdx.x == 0) go = hops[b] < 0 && frontier[0] >= h - 1 ? 1 : 0;    // one thread decides for the block
    __syncthreads();
    if (!go) return;
    auto each = [&](auto &&fn) { place_estimates(L, R, F, C, min_confirm, hops, o, h, b, fn); };
    int turn = 1;
    int64_t med = 0;
    const int32_t total = closure_lower_median(each, sh, turn, med);
    if (threadIdx.x == 0 && total > 0) {
        o[b] = med;
        hops[b] = h;
        atomicMax(frontier, h);
    }
}

__global__ __launch_bounds__(ASX_THREADS) void k_place_sweep(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                              const int32_t *__restrict__ F, uint32_t C, int min_confirm,
                                                              const int32_t *__restrict__ hops, const int64_t *__restrict__ from,
                                                              int64_t *__restrict__ to, int64_t *__restrict__ step)
{
    __shared__ ClosureLds sh;
    const uint32_t b = blockIdx.x;
    if (hops[b] <= 0) {                                         // the root stays 0; a clip that was not reached is 0
        if (threadIdx.x == 0) { to[b] = 0; step[b] = 0; }
        return;
    }
    auto each = [&](auto &&fn) { place_estimates(L, R, F, C, min_confirm, hops, from, INT32_MAX, b, fn); };
    int turn = 1;
    int64_t med = 0;
    const int32_t total = closure_lower_median(each, sh, turn, med);
    if (threadIdx.x == 0) {                                     // (a reached clip has the neighbour that reached it: total > 0)
        const int64_t was = from[b], now = total > 0 ? med : was;
        to[b] = now;
        step[b] = now - was;
    }
}

__global__ __launch_bounds__(ASX_THREADS) void k_place_verdict(const int64_t *__restrict__ L, const int32_t *__restrict__ R,
                                                                const int32_t *__restrict__ F, uint32_t C, int64_t tol,
                                                                int min_confirm, const int32_t *__restrict__ hops,
                                                                const int64_t *__restrict__ o, int32_t *__restrict__ support,
                                                                int32_t *__restrict__ degree, int64_t *__restrict__ resid,
                                                                int32_t *__restrict__ state)
{
    __shared__ ClosureLds sh;
    const uint32_t b = blockIdx.x;
    const bool reached = hops[b] >= 0;
    const int64_t ob = o[b];
    int32_t deg = 0, sup = 0;
    if (reached) {                                              // (the same in every thread of the block)
        auto each = [&](auto &&fn) { place_estimates(L, R, F, C, min_confirm, hops, o, INT32_MAX, b, fn); };
        int turn = 1;
        deg = closure_count_le(each, INT64_MAX, sh, turn);
        sup = deg > 0 ? closure_count_near(each, ob, tol, sh, turn) : 0;
    }
    if (threadIdx.x == 0) { support[b] = sup; degree[b] = deg; }
    for (uint32_t c = threadIdx.x; c < C; c += ASX_THREADS) {
        const uint32_t i = b * C + c;
        const bool ok = reached && hops[c] >= 0 && closure_usable(L, R, F, C, min_confirm, b, c);
        const int64_t d = ok ? L[i] - (o[c] - ob) : 0;
        resid[i] = d;
        state[i] = !ok ? 0 : (d >= -tol && d <= tol) ? 1 : 2;
    }
}

void asx_launch_pool_place(const int64_t *lag, const int32_t *ret, const int32_t *confirm, uint32_t C, int64_t tol, int min_confirm,
                           const int32_t *d_root, int max_hops, int sweeps, int64_t *scratch, int64_t *offset, int32_t *hops,
                           int32_t *support, int32_t *degree, int64_t *step, int64_t *resid, int32_t *state, hipStream_t s)
{
    const dim3 block(ASX_THREADS), per_clip(C);
    int64_t *cur = (sweeps & 1) ? scratch : offset, *other = (sweeps & 1) ? offset : scratch;   // the last sweep writes `offset`
    int32_t *frontier = degree;
    hipLaunchKernelGGL(k_place_init, dim3((C + ASX_THREADS - 1) / ASX_THREADS), block, 0, s, d_root, C, hops, cur, step, frontier);
    for (int h = 1; h <= max_hops; h++)
        hipLaunchKernelGGL(k_place_layer, per_clip, block, 0, s, lag, ret, confirm, C, min_confirm, (int32_t)h, hops, cur, frontier);
    for (int i = 0; i < sweeps; i++) {
        hipLaunchKernelGGL(k_place_sweep, per_clip, block, 0, s, lag, ret, confirm, C, min_confirm, (const int32_t *)hops,
                           (const int64_t *)cur, other, step);
        int64_t *t = cur;
        cur = other;
        other = t;
    }
    hipLaunchKernelGGL(k_place_verdict, per_clip, block, 0, s, lag, ret, confirm, C, tol, min_confirm, (const int32_t *)hops,
                       (const int64_t *)cur, support, degree, resid, state);
}
