// csrc/finalize_body.h -- the body of k_finalize and of its per-pair form k_finalize_p (xcorr_kernels.hip), included INSIDE both
// kernels (a call boundary changes the instruction stream, and k_finalize has to stay the kernel it was).  The including kernel
// defines seed (uint32_t): the index an empty running maximum stands for.
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
