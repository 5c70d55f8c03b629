// csrc/refine_dots_body.h -- the body of k_refine_dots and of its listed form k_refine_dots_l (xcorr_kernels.hip), included INSIDE
// both kernels (k_refine_dots has to stay the kernel it was).  ASX_SRC_OF(pair) / ASX_SMP_OF(pair): where pair's inputs start, in
// elements from src / smp (by default pair * src_pitch / pair * smp_pitch; the listed form defines its own before the include).
#ifndef ASX_SRC_OF
#define ASX_SRC_OF(pair) pair * src_pitch
#define ASX_SMP_OF(pair) pair * smp_pitch
#endif
    __shared__ double red[2][ASX_THREADS / 64];
    const size_t pair = blockIdx.y;
    const uint32_t ncand = W.refine_n[pair];
    if (blockIdx.x >= ncand) return;
    const uint32_t N = Pp->N, L = 2u * N;
    const TIn *x = src + ASX_SRC_OF(pair);
    const TIn *y = smp + ASX_SMP_OF(pair);
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
#undef ASX_SRC_OF
#undef ASX_SMP_OF
