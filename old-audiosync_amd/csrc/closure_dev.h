// closure_dev.h -- device helpers that the kernels of asx_pool_closure_dev (xcorr_kernels.hip) and of asx_pool_place_dev (place.hip)
// share: what a valid, a good and a usable pair is, the block-wide sum, and the lower median of a multiset by rank counting.
// The picked tables are [C][C], pair (a, b) at a * C + b; everything is integer arithmetic.
#pragma once
#include "asx_internal.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ bool closure_valid(int64_t lag, int32_t ret)
{
    return ret == 0 && lag >= -ASX_CLOSURE_LAG_LIMIT && lag <= ASX_CLOSURE_LAG_LIMIT;
}

// a pair with a valid picked entry off the diagonal
__device__ __forceinline__ bool closure_good(const int64_t *L, const int32_t *R, uint32_t C, uint32_t x, uint32_t y)
{
    return x != y && closure_valid(L[x * C + y], R[x * C + y]);
}

// a pair the offsets may use: good, and confirmed by at least min_confirm clips
__device__ __forceinline__ bool closure_usable(const int64_t *L, const int32_t *R, const int32_t *F, uint32_t C, int min_confirm,
                                               uint32_t x, uint32_t y)
{
    return closure_good(L, R, C, x, y) && F[x * C + y] >= min_confirm;
}

// the sum of v over a block of ASX_THREADS threads, in every thread, with one barrier; red: ASX_THREADS / 64 ints of LDS that the sum
// before this one did not use (two buffers in turn: the barrier of a sum lies between the reads of the one before it and the
// writes of the one after it)
__device__ __forceinline__ int32_t closure_block_sum(int32_t v, int32_t *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int32_t s = 0;
#pragma unroll
    for (int i = 0; i < ASX_THREADS / 64; i++) s += red[i];
    return s;
}

// The LDS of one block's counts over a multiset that is never stored: `each(fn)` hands every element that THIS thread holds to fn,
// the same elements at every call, and the block's threads hold the multiset between them.  `turn` names the buffer the sum before
// used; a block starts with turn = 1 and hands the same variable to every call below.
struct ClosureLds {
    int32_t red[2][ASX_THREADS / 64];
    int64_t lo[ASX_THREADS / 64], hi[ASX_THREADS / 64];
};

// how many elements are <= v, in every thread
template <typename Each>
__device__ __forceinline__ int32_t closure_count_le(Each &each, int64_t v, ClosureLds &sh, int &turn)
{
    int32_t m = 0;
    each([&](int64_t x) { m += x <= v ? 1 : 0; });
    turn ^= 1;
    return closure_block_sum(m, sh.red[turn]);
}

// how many elements lie within tol of `centre`
template <typename Each>
__device__ __forceinline__ int32_t closure_count_near(Each &each, int64_t centre, int64_t tol, ClosureLds &sh, int &turn)
{
    const int32_t upto = closure_count_le(each, centre + tol, sh, turn);
    return upto - closure_count_le(each, centre - tol - 1, sh, turn);
}

// The lower median by rank counting -- the smallest v with #(x <= v) > (n - 1) / 2, found by bisection between the smallest and the
// largest element, each step one count over the block.  Returns the number of elements n in every thread; med = 0 when n == 0.  To
// be called at most once per block (sh.lo and sh.hi are written once).
template <typename Each>
__device__ __forceinline__ int32_t closure_lower_median(Each &each, ClosureLds &sh, int &turn, int64_t &med)
{
    int32_t n = 0;
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    each([&](int64_t x) { n++; lo = x < lo ? x : lo; hi = x > hi ? x : hi; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63u) == 0) { sh.lo[threadIdx.x >> 6] = lo; sh.hi[threadIdx.x >> 6] = hi; }
    turn ^= 1;
    const int32_t total = closure_block_sum(n, sh.red[turn]);   // (its barrier also covers sh.lo and sh.hi)
#pragma unroll
    for (int i = 0; i < ASX_THREADS / 64; i++) {
        lo = sh.lo[i] < lo ? sh.lo[i] : lo;
        hi = sh.hi[i] > hi ? sh.hi[i] : hi;
    }
    med = 0;
    if (total > 0) {
        const int32_t want = (total - 1) / 2 + 1;               // the median is the smallest v with at least this many at or below it
        lo -= 1;                                                // count_le(lo) = 0 < want <= total = count_le(hi)
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (closure_count_le(each, mid, sh, turn) >= want) hi = mid; else lo = mid;
        }
        med = hi;
    }
    return total;
}
