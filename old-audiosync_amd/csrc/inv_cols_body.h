// csrc/inv_cols_body.h -- the body of k_inv_cols and of its lag-window form k_inv_cols_w (xcorr_kernels.hip), included INSIDE both
// kernels (a call boundary changes the instruction stream, and k_inv_cols has to stay the kernel it was).  The including kernel
// defines WIN (constexpr bool) and Z (AsxWin).  WIN: only the lags of Z compete and Z.seed is the one whose key is signed (the
// generalisation of the idx < nout test).  The fast scans see out-of-window values as NaN (never a maximum there, never a
// candidate); the general scans skip them; r_out still receives every lag.
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
