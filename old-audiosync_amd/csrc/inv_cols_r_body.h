// csrc/inv_cols_r_body.h -- the body of k_inv_cols_r and of its lag-window form k_inv_cols_rw (rlayout.hip), included INSIDE both
// kernels.  Written inside the __global__ itself rather than in a function they call: a call boundary changes the instruction stream
// (see rows_r_body), and k_inv_cols_r has to stay the kernel it was.  The including kernel defines WIN (constexpr bool) and Z (AsxWin).
// WIN: only the lags of Z compete, and Z.seed is the one whose key is signed.  Out-of-window values become NaN in the fast scan (a
// NaN never wins there and is never a candidate) and are skipped everywhere else; r_out still receives every lag.
    constexpr int M1 = S1::n, T = TC, logT = asx_ilog2(TC), H = T / 2, logH = logT - 1;
    __shared__ asx_peak_t red[NT / 64];
    __shared__ asx_peak_t s_run0;
    __shared__ float s_b2;
    // TILE-major launch order, grid (npairs, tiles): the tiles of one pair are spread over the life of the launch, so the running
    // maximum a block fetches at its start (`run0`) already holds the maximum of the tiles before it, and a tile that cannot hold
    // the peak -- nearly all of them -- never enters the candidate path with its returning atomic.  Pair-major (the 150 tiles of a
    // pair resident together, run0 == 0 for all of them): 0.405 against 0.367 ms at 600 rows, 0.423 against 0.299 ms per 1024 pairs
    // at 300 rows (profiles/r5_experiments/02_*).
    const size_t pair = blockIdx.x;
#ifdef ASX_INV_BODY_TILE // k_inv_cols_rq: the tile its prologue chose; every other kernel: the tile of its place in the grid, as before
    const int tile = ASX_INV_BODY_TILE;
#else
    const int tile = rcol_tile_of_block(blockIdx.y, logT);
#endif
    if (tile * T >= P.M2) return; // the tile count is rounded up; the tile width is this kernel's own (it reads only)
    {
        // Stagger: the blocks that share a CU run the same program -- a load phase (the tile's rows), then compute phases of about
        // the same length -- and, started together, stay in step: both wait for memory, then both compute.  The blocks of the FIRST
        // generation start half a block's life apart, by the parity of their position in the launch order (the split that measured
        // best); later generations inherit the offset.  0.370 -> 0.349 ms at 600 rows, -3 .. -6 % at 400 (rows and
        // forward columns: nothing, profiles/r5_experiments/05_*).  Speed only.  (What it staggers is not the two blocks of a CU -- those are
        // 256 apart in launch order, same parity -- but HALF THE CHIP against the other half: a read-only kernel whose blocks all take the
        // same time otherwise loads in step and computes in step chip-wide, and the memory system idles between the bursts.  On the round's
        // final kernel: 0.373 ms without, 0.301 with; more phases or other lengths: the same, profiles/r5_experiments/25_*.)
        // The first generation = the blocks resident at once: two per CU for 600- and 400-row tiles, four for 300-row tiles.  (Round 5 had
        // left the 300-row instance alone -- with the FIRST 512 of its 1024 resident blocks treated that way it was 1.5 % slower; with the
        // whole first generation: 0.310 -> 0.278 ms per 1024 pairs of N = 144 000, profiles/r5_experiments/25_*.)
        // first_gen comes from the launcher (occupancy of this kernel x the device's CUs: nothing here assumes 256 CUs).
        const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
        if (gridDim.x * gridDim.y > first_gen && lin < first_gen && (lin & 1u)) // (a launch of one generation has nobody to inherit the offset)
            for (unsigned i = 0; i < (unsigned)(M1 * 27 / 64 / 2); i += 16) __builtin_amdgcn_s_sleep(16); // half a block's life; 64 cycles per unit
    }
    const double shift = W.shift ? W.shift[pair] : 0.0; // non-zero only in the second look (asx_api.hip)
    const int M2 = P.M2, c0 = tile * T;
    const float2 *in = qi + RWS_PAIR(pair) * pair_pitch;
    float4 *lds4 = reinterpret_cast<float4 *>(asx_lds_r);
    const LdsLayout Lc = col_layout(T, logT, NT);
    // the pair's running maximum so far and the width of the near-maximum window: fetched now, used behind the barriers
    const float b2_early = W.bound2[pair];
    // (thread 0 asks for the running maximum here and leaves it in LDS BEHIND the tile loads: stored at once, its wave sat out a memory
    // round trip before it issued its share of the tile's loads, and the block's first barrier waited for that wave: 0.3195 -> 0.3145 ms
    // at 600 rows, -1 % at 400; every thread asking instead: +3 % at 600 rows, profiles/r5_experiments/20_*)
    asx_peak_t run0_early = 0;
    if (threadIdx.x == 0) run0_early = W.pairmax[pair];
    // ---- first stage to run (the innermost, radix RL = R_last, RL consecutive slots per butterfly), fed from HBM --------
    // Butterfly b of a column pair holds the frequencies u_b + MB t (t < RL, MB = M1 / RL, u_b = digit swap of b); their
    // tangling partners M1 - u_b - MB t are element RL-1-t of butterfly b' (u_b' = MB - u_b).  A work item takes BOTH
    // butterflies: 2 RL rows of 16 bytes straight from HBM, the tangling in registers
    //     Z'[u] = S + i conj(w) D,  Z'[M1-u] = conj(S - i conj(w) D),  S = Q[u] + conj Q[M1-u], D = Q[u] - conj Q[M1-u], w = w_{2 M1}^u
    // (w = w_{2 M1}^u_b times the compile-time root w_{2 RL}^t), the two inverse butterflies, 2 RL slots written: no fill
    // phase, no index table, no barrier before the first stage.  u_b = 0 (rows 0, MB, ..., M1: the extra row is its own
    // partner row set) and u_b = MB/2 pair with themselves: one butterfly.
    static_assert(S1::nstages == 3, "three-stage column schedules");
    constexpr StageK KL = S1::stage(2), KM = S1::stage(1);
    constexpr int RL = KL.R, R0c = S1::stage(0).R, R1c = KM.R, MB = M1 / RL;
    static_assert(KL.q == 1 && MB == R0c * R1c && MB % 2 == 0, "innermost stage of consecutive slots");
    constexpr int NITEMS = (MB / 2) * H; // v = 0 takes both butterflies that pair with themselves (u_b = 0 and MB/2)
    const size_t sblock = pair * (size_t)(P.M2 / T) + tile; (void)sblock;
    RSTAMP(2, sblock, 0);
    const TwPre pre_mid = tw_prefetch_exec<S1, 1, true, true, true>(Lc, P.tw1);
    static_assert(NITEMS <= NT, "one work item per thread at most");
    if (const int e = rcol_item_of_thread<NITEMS, H, NT>(threadIdx.x); e >= 0) {
        const int g = e & (H - 1), v = e >> logH;  // v = u_b in [0, MB/2)
        const int ub = v, ubp = v == 0 ? MB / 2 : MB - v; // first rows of the two butterflies' row sets
        const float2 *ca = in + (size_t)ub * M2 + c0 + 2 * g, *cb = in + (size_t)ubp * M2 + c0 + 2 * g;
        // The tangling twiddle w_{2 M1}^u_b = w_F^(u_b M2).  WU_FRONT: asked for IN FRONT of the rows (vmcnt completes in order) and used by
        // both branches below (u_b = 0: exactly 1), which keeps the compiler from sinking the look-up into the one branch that needs it,
        // behind the rows, where its second table value was only issued when the rows had arrived: 0.317 -> 0.3055 ms at 600 rows.  The
        // 400- and 300-row instances lose 1 - 1.6 % with it (profiles/r5_experiments/23_*) and keep the look-up where it was.
        constexpr bool WU_FRONT = ASX_INV_WU && M1 == 600;
        float2 wu_all = make_float2(1.f, 0.f);
        if constexpr (WU_FRONT) wu_all = tw_F(P, (uint32_t)ub * (uint32_t)M2);
        Cx2 A[RL], B[RL];
        static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
            constexpr int t = decltype(TT)::value;
            const float4 x = ld_f4(ca + (size_t)(t * MB) * M2, ASX_RNT & 1);
            const float4 y = ld_f4(cb + (size_t)(t * MB) * M2, ASX_RNT & 1);
            A[t] = Cx2{ v2f{ x.x, x.z }, v2f{ x.y, x.w } };
            B[t] = Cx2{ v2f{ y.x, y.z }, v2f{ y.y, y.w } };
        });
        Cx2 za[RL], zb[RL];
        if (v != 0) {
            const float2 wu = WU_FRONT ? wu_all : tw_F(P, (uint32_t)ub * (uint32_t)M2);
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 b = B[RL - 1 - t];
                const Cx2 S = Cx2{ A[t].re + b.re, A[t].im - b.im };
                const Cx2 D = Cx2{ A[t].re - b.re, A[t].im + b.im };
                const Cx2 tt = mul_pos_i(mul_root<2 * RL, t, true>(mulwc(D, wu))); // i conj(w) D, w = wu * w_{2 RL}^t
                za[t] = S + tt;
                const Cx2 m = S - tt;
                zb[RL - 1 - t] = Cx2{ m.re, -m.im };
            });
        } else {
            // u_b = 0: Q[MB t] pairs with Q[MB (RL - t)], t = 0 with the extra row M1; u_b = MB/2: within the butterfly
            const float4 xm = ld_f4(in + (size_t)M1 * M2 + c0 + 2 * g, ASX_RNT & 1);
            const Cx2 QM = Cx2{ v2f{ xm.x, xm.z }, v2f{ xm.y, xm.w } };
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                Cx2 b = QM;
                if constexpr (t != 0) b = A[RL - t];
                const Cx2 S = Cx2{ A[t].re + b.re, A[t].im - b.im };
                const Cx2 D = Cx2{ A[t].re - b.re, A[t].im + b.im };
                if constexpr (WU_FRONT) za[t] = S + mul_pos_i(mul_root<2 * RL, t, true>(mulwc(D, wu_all))); // wu_all = w_F^0 = 1 here
                else za[t] = S + mul_pos_i(mul_root<2 * RL, t, true>(D));
            });
            static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const Cx2 b = B[RL - 1 - t];
                const Cx2 S = Cx2{ B[t].re + b.re, B[t].im - b.im };
                const Cx2 D = Cx2{ B[t].re - b.re, B[t].im + b.im };
                zb[t] = S + mul_pos_i(mul_root<4 * RL, 2 * t + 1, true>(D));
            });
        }
        // slots: butterfly b = d0 * R1 + d1 for u_b = d0 + R0 * d1
        const int d1 = ub / R0c, d0 = ub - d1 * R0c, e1 = ubp / R0c, e0 = ubp - e1 * R0c;
        float4 *pa = lds4 + (((d0 * R1c + d1) * RL) << logH) + g, *pb = lds4 + (((e0 * R1c + e1) * RL) << logH) + g;
        Bfly<RL, true>::run(za);
        Bfly<RL, true>::run(zb);
        static_for<0, RL>([&](auto TT) __attribute__((always_inline)) {
            lds_put(pa + (decltype(TT)::value << logH), za[TT]);
            lds_put(pb + (decltype(TT)::value << logH), zb[TT]);
        });
    }
    if (threadIdx.x == 0) {
        s_run0 = run0_early;
        s_b2 = b2_early;
    }
    RSTAMP(2, sblock, 1);
    // A digitally silent track (zero norm: r is exactly zero everywhere): the running maximum stays zero, which k_finalize
    // reads as index 0, the reference's answer (see k_inv_cols).  Checked HERE, behind the tile loads: in front of them the
    // block waited a memory latency for this one float before it issued anything.  Block-uniform.
    if (b2_early == 0.f && r_out == nullptr) return;
    __syncthreads();
    const TwPre pre_last = lds_fft_static_steps<S1, true, true, S1::nstages - 1, true, 1>(lds4, Lc, P.tw1, pre_mid);
    RSTAMP(2, sblock, 2);
    const asx_peak_t run0 = s_run0;
    const float b2 = s_b2;
    auto last_stage = [&](auto &&sink) __attribute__((always_inline)) {
        lds_last_stage_static<S1, true, true>(lds4, Lc, P.tw1, pre_last, sink);
    };
    const uint32_t uM2 = (uint32_t)M2;
    // the seed's tile takes the general form (lag 0's tile without a window)
    const uint32_t seed = WIN ? Z.seed : 0u;
    const bool fast = (WIN ? (uint32_t)tile != (seed % uM2) / (uint32_t)T : tile != 0) && (r_out == nullptr) && shift == 0.0;
    auto inw = [&](uint32_t idx) __attribute__((always_inline)) { return !WIN || asx_win_has(Z, idx); };
    auto examine_again = [&](float thr) __attribute__((always_inline)) {
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + (uint32_t)(h & 1) * uM2 + (uint32_t)(h >> 1);
                    const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                    if (inw(idx) && key >= thr) cand_append(W, pair, idx, key);
                }
            });
        });
    };
    float thr_again = 0.f;
    bool again = false;
    if (fast) {
        // The scan keeps ONE number per thread: the largest |r| of its 4 R lags (NaNs drop out of fmaxf).  Which lag it was is
        // looked up again only by a tile that can matter (below): with the tile-major launch order nearly every tile finds its
        // maximum under the window of the running maximum it fetched at its start and is done behind one barrier -- no index,
        // no second maximum, no atomic.  (Tracking index, slot and runner-up in the scan: 17 instead of 3 instructions per slot,
        // k_inv_cols_r 0.353 against 0.332 ms at 600 rows, 1.15 against 1.08 ms per 1024 pairs at 400, equal at 600 x 480,
        // 0.31 against 0.32 at 300 rows; profiles/r5_experiments/06_*.)
        float best_m = -INFINITY;
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                if constexpr (WIN) {
                    const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
                    const float a0 = inw(i0) ? fabsf(v[t].re.x) : NAN, a1 = inw(i0 + uM2) ? fabsf(v[t].im.x) : NAN;
                    const float a2 = inw(i0 + 1) ? fabsf(v[t].re.y) : NAN, a3 = inw(i0 + uM2 + 1) ? fabsf(v[t].im.y) : NAN;
                    best_m = fmaxf(fmaxf(best_m, fmaxf(a0, a1)), fmaxf(a2, a3));
                } else {
                    best_m = fmaxf(fmaxf(best_m, fmaxf(fabsf(v[t].re.x), fabsf(v[t].im.x))), fmaxf(fabsf(v[t].re.y), fabsf(v[t].im.y)));
                }
            });
        });
        RSTAMP(2, sblock, 4);
        const float wmax = wave_max_nonneg(fmaxf(best_m, 0.f));
        float *redf = reinterpret_cast<float *>(red);
        if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = wmax;
        __syncthreads();
        float bm = redf[0];
        for (int w = 1; w < NT / 64; w++) bm = fmaxf(bm, redf[w]);
        // the final maximum is >= run0: below run0's window nothing of this tile can be the peak or near it (run0 == 0, nothing
        // seen yet, gives a NaN threshold: no exit)
        if (bm < near_max_threshold(peak_key(run0), b2)) return; // block-uniform
        RSTAMP(2, sblock, 5);
        // ---- a tile that can matter (the first generation of blocks, record setters, the peak's tile): the last stage again for
        // the threads that hold its maximum or a near-maximum -- smallest lag and signed value of the maximum, candidates.
        // (The holders publishing for themselves, without the fold and its two barriers: the same time, and 8 bytes of scratch.)
        const float thr = near_max_threshold(fmaxf(bm, peak_key(run0)), b2); // key(run0) is NaN when nothing was seen: fmaxf drops it
        uint32_t my_idx = 0xFFFFFFFFu;
        float my_val = 0.f;
        if (best_m >= thr || best_m == bm) {
            last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
                static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                    constexpr int t = decltype(TT)::value;
                    const float val[4] = { v[t].re.x, v[t].re.y, v[t].im.x, v[t].im.y }; // in lag order: i0, i0 + 1, i0 + M2, i0 + M2 + 1
                    const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const uint32_t idx = i0 + (uint32_t)(h >> 1) * uM2 + (uint32_t)(h & 1);
                        const float a = inw(idx) ? fabsf(val[h]) : NAN;
                        if (a == bm && idx < my_idx) { my_idx = idx; my_val = val[h]; }
                        if (a >= thr) cand_append(W, pair, idx, a);
                    }
                });
            });
        }
        __syncthreads(); // redf is read by every thread above
        const asx_peak_t mine = my_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(bm, my_idx);
        const asx_peak_t tb = block_peak_max(mine, red);
        if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], tb); red[0] = tb; }
        __syncthreads();
        // the one thread that holds the tile's best lag: its SIGNED value (the key is |r|) for the spectral Pearson form
        if (W.tile_peak && mine != 0 && mine == red[0]) W.tile_peak[pair * (size_t)(P.M2 / T) + tile] = my_val;
    } else {
        // general form: first tile (lag 0 competes signed), r dumped for tests, shifted keys of the second look
        float best_key = -INFINITY, best_val = 0.f;
        uint32_t best_idx = 0xFFFFFFFFu;
        last_stage([&](auto RC, auto &v, int g, int pos0, int q) __attribute__((always_inline)) {
            static_for<0, decltype(RC)::value>([&](auto TT) __attribute__((always_inline)) {
                constexpr int t = decltype(TT)::value;
                const float val[4] = { v[t].re.x, v[t].im.x, v[t].re.y, v[t].im.y };
                const uint32_t i0 = (uint32_t)(2 * (pos0 + t * q)) * uM2 + (uint32_t)(c0 + 2 * g);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t idx = i0 + (uint32_t)(h & 1) * uM2 + (uint32_t)(h >> 1);
                    const float key = shift == 0.0 ? peak_key_of(val[h], idx, seed) : peak_key_shifted(val[h], idx, shift, seed);
                    if (inw(idx) && (key > best_key || (key == best_key && idx < best_idx) || best_idx == 0xFFFFFFFFu)) { best_key = key; best_idx = idx; best_val = val[h]; }
                    if (r_out) r_out[pair * (size_t)P.nout + idx] = val[h];
                }
            });
        });
        const asx_peak_t mine = best_idx == 0xFFFFFFFFu ? 0 : peak_pack_key(best_key, best_idx);
        asx_peak_t best = block_peak_max(mine, red);
        if (threadIdx.x == 0) { atomicMax(&W.pairmax[pair], best); red[0] = best; }
        __syncthreads();
        if (W.tile_peak && mine != 0 && mine == red[0]) W.tile_peak[pair * (size_t)(P.M2 / T) + tile] = best_val; // one thread: indices are unique
        const float thr = near_max_threshold(peak_key(peak_max(red[0], run0)), b2);
        again = best_key >= thr;
        thr_again = thr;
    }
    if (again) examine_again(thr_again);
    RSTAMP(2, sblock, 3);
