// csrc/pearson_prep_body.h -- the body of k_pearson_prep and of its per-pair form k_pearson_prep_p (pearson_spectral.hip), included
// INSIDE both kernels (k_pearson_prep has to stay the kernel it was).  The including kernel defines seed (uint32_t): the index whose
// exact value competes signed.  ASX_SRC_OF(pair) / ASX_SMP_OF(pair): where pair's inputs start in floats from src / smp (by default
// pair * src_pitch / pair * smp_pitch; the listed forms k_pearson_prep_l / _pl define their own before the include).
#ifndef ASX_SRC_OF
#define ASX_SRC_OF(pair) pair * src_pitch
#define ASX_SMP_OF(pair) pair * smp_pitch
#endif
    __shared__ double red[4][NTP / 64];
    __shared__ double s_exact;
    __shared__ int s_have_exact;
    __shared__ double rkey[NTP / 64], rval[NTP / 64];
    __shared__ uint32_t ridx[NTP / 64];
    __shared__ AsxSeg s_seg;
    const size_t pair = blockIdx.y;
    const uint32_t blk = blockIdx.x, gtid = blk * (uint32_t)NTP + threadIdx.x;
    const uint32_t N = Pp->N;
    const int M2 = Pp->M2, nbands = Pp->nbands;
    const uint32_t gs = (uint32_t)Pp->band_rows * (uint32_t)M2;
    const asx_peak_t best = W.pairmax[pair];
    // ---- k_refine_pick's part (xcorr_kernels.hip; this kernel stands in for it in the spectral form: one launch less): the
    // reference's max_abs_index rule (src/cross_correlation.c:52-67) on the exact values of the re-evaluated near-ties --
    // key(seed) = r[seed] signed (seed = 0, or a lag window's first index), key(i) = |r[i]|, largest key, smallest lag among equal
    // keys, a NaN never wins unless at the seed --
    // and, kept here, the winner's exact SIGNED value: the cross term of the coefficient
    const uint32_t nref = W.refine_n[pair];
    if (nref >= 2u) { // block-uniform
        double bk = -INFINITY, bv = 0.0;
        uint32_t bi = 0xFFFFFFFFu;
        for (uint32_t i = threadIdx.x; i < nref; i += NTP) {
            const uint32_t idx = W.refine_idx[pair * (size_t)W.cap + i];
            const double v = W.refine_val[pair * (size_t)W.cap + i];
            double key;
            if (idx == seed) key = (v != v) ? (double)INFINITY : v + 0.0;
            else { key = fabs(v); if (key != key) key = -(double)INFINITY; }
            if (key > bk || (key == bk && idx < bi)) { bk = key; bi = idx; bv = v; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ok = __shfl_xor(bk, off, 64), ov = __shfl_xor(bv, off, 64);
            const uint32_t oi = (uint32_t)__shfl_xor((int)bi, off, 64);
            if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; bv = ov; }
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { rkey[wave] = bk; ridx[wave] = bi; rval[wave] = bv; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < NTP / 64; w++)
                if (rkey[w] > bk || (rkey[w] == bk && ridx[w] < bi)) { bk = rkey[w]; bi = ridx[w]; bv = rval[w]; }
            AsxSeg sg = seg[pair];
            if (bi != 0xFFFFFFFFu) { sg = make_seg(bi, N); if (blk == 0) seg[pair] = sg; } // every block of the pair finds the same winner
            s_seg = sg;
            s_exact = bv;
            s_have_exact = bi != 0xFFFFFFFFu;
        }
    } else if (threadIdx.x == 0) {
        s_seg = seg[pair];
        s_have_exact = 0;
    }
    __syncthreads();
    const AsxSeg s = s_seg;
    // A pair the transforms had nothing to say about (silent or NaN track: no maximum), an empty segment, or a lag that is still
    // the float32 placeholder of an overflowed list (the second look redoes it): the direct reduction, whatever it yields.
    const bool direct = best == 0 || s.len == 0 || (s.flags & ASX_SEG_INEXACT) != 0;
    if (blk == 0 && threadIdx.x == 0) {
        // the header: r[peak] in the plain-sum scale and the bound on its error
        double r = 0.0, rb = 0.0;
        if (!direct) {
            if (s_have_exact) r = s_exact;
            else {
                const int T = Pp->T;
                r = (double)W.tile_peak[pair * (size_t)(M2 / T) + (s.peak % (uint32_t)M2) / (uint32_t)T] / (double)Pp->F;
                rb = 0.5 * (double)W.bound2[pair] / (double)Pp->F; // bound2 = 2B in the device's scale (F times the plain sum)
            }
        }
        double *hdr = S.hdr + pair * ASX_SPEC_HDR;
        hdr[0] = r; hdr[1] = rb; hdr[2] = direct ? 1.0 : 0.0; hdr[3] = 0.0;
    }
    if (direct) return; // block-uniform, and the same in every block of the pair: nobody reads its shares
    const float *x = src + ASX_SRC_OF(pair), *y = smp + ASX_SMP_OF(pair);
    const int ntiles = Pp->ntiles;
    const float2 *bx = W.band + (size_t)pair * 2 * ntiles * nbands, *by = bx + (size_t)ntiles * nbands;
    const Acc2 ax = window_share<(uint32_t)NTP * NB>(x, bx, gs, ntiles, nbands, s.src_off, s.src_off + s.len, gtid);
    const Acc2 ay = window_share<(uint32_t)NTP * NB>(y, by, gs, ntiles, nbands, s.smp_off, s.smp_off + s.len, gtid);
    double v[4] = { ax.s1, ax.s2, ay.s1, ay.s2 };
    block_sum4<NTP>(v, red);
    if (threadIdx.x == 0) {
        double *mine = S.part + (pair * NB + blk) * 4;
        mine[0] = v[0]; mine[1] = v[1]; mine[2] = v[2]; mine[3] = v[3];
    }
#undef ASX_SRC_OF
#undef ASX_SMP_OF
