// csrc/refine_pick_body.h -- the body of k_refine_pick and of its per-pair form k_refine_pick_p (xcorr_kernels.hip), included INSIDE
// both kernels (k_refine_pick has to stay the kernel it was).  The including kernel defines seed (uint32_t): the index whose exact
// value competes signed.
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
