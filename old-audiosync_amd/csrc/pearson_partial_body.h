// csrc/pearson_partial_body.h -- the body of k_pearson_partial and of its listed form k_pearson_partial_l (xcorr_kernels.hip),
// included INSIDE both kernels (k_pearson_partial has to stay the kernel it was).  ASX_SRC_OF(pair) / ASX_SMP_OF(pair): where pair's
// inputs start, in elements from src / smp (by default pair * src_pitch / pair * smp_pitch; the listed form defines its own).
#ifndef ASX_SRC_OF
#define ASX_SRC_OF(pair) pair * src_pitch
#define ASX_SMP_OF(pair) pair * smp_pitch
#endif
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
    const TIn *x = src + ASX_SRC_OF(pair) + s.src_off;
    const TIn *y = smp + ASX_SMP_OF(pair) + s.smp_off;
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
#undef ASX_SRC_OF
#undef ASX_SMP_OF
