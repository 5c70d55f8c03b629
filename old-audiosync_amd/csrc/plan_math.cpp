// csrc/plan_math.cpp — see plan_math.h.  Pure host arithmetic.
#include <cstring>
#include <cstdlib>
#include <functional>
#include <algorithm>
#include "plan_math.h"
#include "kernel_table.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

bool asx_is_smooth(uint64_t n)
{
    if (n == 0) return false;
    for (uint64_t p : { 2ull, 3ull, 5ull })
        while (n % p == 0) n /= p;
    return n == 1;
}

uint64_t asx_next_smooth_even(uint64_t n)
{
    n += n & 1ull;
    if (n < 2) n = 2;
    while (!asx_is_smooth(n)) n += 2;
    return n;
}

// Radix schedule: the fewest passes over LDS using radices the kernels implement
// (lds_fft.h), ties broken by the smallest radix sum.  Order: even radices first
// (largest first), odd radices last -- the innermost stages (small q) then stride
// LDS by an odd number of elements, which spreads over the banks.
static const int kRadices[] = { 16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2 };

static void search_radices(int rem, int depth, int sum, int *cur, int *best, int *best_depth, int *best_sum,
                           int min_next)
{
    if (rem == 1) {
        if (depth < *best_depth || (depth == *best_depth && sum < *best_sum)) {
            *best_depth = depth;
            *best_sum = sum;
            for (int i = 0; i < depth; i++) best[i] = cur[i];
        }
        return;
    }
    if (depth + 1 > *best_depth || depth >= ASX_MAX_STAGES) return;
    for (int R : kRadices) {
        if (R > min_next || rem % R) continue; // non-increasing: each multiset visited once
        cur[depth] = R;
        search_radices(rem / R, depth + 1, sum + R, cur, best, best_depth, best_sum, R);
    }
}

bool asx_make_stages(int n, AsxStages *st)
{
    *st = AsxStages{};
    st->n = n;
    int cur[ASX_MAX_STAGES], best[ASX_MAX_STAGES];
    int best_depth = ASX_MAX_STAGES + 1, best_sum = 1 << 30;
    if (n < 1) return false;
    search_radices(n, 0, 0, cur, best, &best_depth, &best_sum, 16);
    if (best_depth > ASX_MAX_STAGES) return false;
    // even radices (descending) first, then odd (descending)
    std::vector<int> order;
    for (int i = 0; i < best_depth; i++) if (best[i] % 2 == 0) order.push_back(best[i]);
    for (int i = 0; i < best_depth; i++) if (best[i] % 2 != 0) order.push_back(best[i]);
    // diagnostic: other orders of the same radices ([10,10,12] does fewer twiddle
    // multiplications than [12,10,10] but its innermost stage strides 12 slots = 4-way bank conflicts, +17 % k_rows)
    if (const char *e = getenv("ASX_STAGE_ORDER")) {
        if (!strcmp(e, "asc")) std::sort(order.begin(), order.end());
        else if (!strcmp(e, "desc")) std::sort(order.begin(), order.end(), std::greater<int>());
    }
    int ns = n;
    for (int i = 0; i < (int)order.size(); i++) {
        const int R = order[i];
        st->radix[i] = R;
        st->ns[i] = ns;
        st->q[i] = ns / R;
        st->nbf[i] = n / R;
        st->twmul[i] = n / ns;
        st->inv_q[i] = 1.0f / (float)(ns / R);
        st->inv_nbf[i] = 1.0f / (float)(n / R);
        ns /= R;
    }
    st->nstages = (int)order.size();
    return true;
}

std::vector<int> asx_position_table(const AsxStages &st)
{
    // k = u0 + R0*u1 + R0*R1*u2 + ...  ->  pos = u0*(n/R0) + u1*(n/(R0*R1)) + ...
    std::vector<int> pos(st.n);
    for (int k = 0; k < st.n; k++) {
        int rem = k, p = 0, stride = st.n;
        for (int i = 0; i < st.nstages; i++) {
            stride /= st.radix[i];
            p += (rem % st.radix[i]) * stride;
            rem /= st.radix[i];
        }
        pos[k] = p;
    }
    return pos;
}

static float2 unit_root(uint64_t num, uint64_t den)
{
    // exp(-2*pi*i*num/den) evaluated in double, rounded once to float
    num %= den;
    const double x = (double)num / (double)den;
    float2 w;
    if (num == 0) return make_float2(1.f, 0.f);
    if (4 * num == den) return make_float2(0.f, -1.f);
    if (2 * num == den) return make_float2(-1.f, 0.f);
    if (4 * num == 3 * den) return make_float2(0.f, 1.f);
    const double a = 2.0 * M_PI * x;
    w.x = (float)cos(a);
    w.y = (float)(-sin(a));
    return w;
}

static int pow2_floor(size_t v)
{
    int p = 1;
    while ((size_t)p * 2 <= v) p *= 2;
    return p;
}

static int tile_for(int M1)
{
    size_t cap = ASX_LDS_COLS_MAX / sizeof(float2) / (size_t)M1;
    if (cap < 1) return 0;
    int T = pow2_floor(cap);
    if (T > 64) T = 64;
    return T;
}

// transform length for sample_len N: 2N if that is {2,3,5}-smooth, else the next smooth even
// length >= 3N-1 (embedding, see asx_host_plan_build)
static uint64_t transform_len(size_t N)
{
    const uint64_t F = 2 * (uint64_t)N;
    return asx_is_smooth(F) ? F : asx_next_smooth_even(3 * (uint64_t)N - 1);
}

std::vector<std::string> asx_host_plan_candidates(size_t N, size_t max_count)
{
    std::vector<std::pair<double, std::string>> all;
    if (N == 0 || N > (size_t)1 << 27) return {};
    const uint64_t F = transform_len(N);
    if (F >= (1ull << 31)) return {};
    const uint32_t M = (uint32_t)(F / 2);
    const int rows_max = (int)(ASX_LDS_ROWS_MAX / (4 * sizeof(float2)));
    for (uint32_t a = 1; a <= M && a <= 8192u; a++) {
        if (M % a) continue;
        const uint32_t b = M / a;
        if ((int)b > rows_max) continue;
        AsxStages s1, s2;
        if (!asx_make_stages((int)a, &s1) || !asx_make_stages((int)b, &s2)) continue;
        int maxr = 2;
        for (int i = 0; i < s1.nstages; i++) maxr = std::max(maxr, s1.radix[i]);
        for (int i = 0; i < s2.nstages; i++) maxr = std::max(maxr, s2.radix[i]);
        const int tmax = tile_for((int)a);
        for (int t = 2; t <= tmax; t <<= 1) {
            if ((uint32_t)t > b && t > 2) continue;
            if (t < 8 && tmax >= 8) continue; // narrow tiles only where nothing wider fits
            const double lds = (double)std::max((size_t)a * t * sizeof(float2), (size_t)4 * b * sizeof(float2)) / 1024.0;
            const double cost = lds + 8.0 * (s1.nstages + s2.nstages) + (maxr > 12 ? 20.0 : 0.0);
            char buf[64];
            snprintf(buf, sizeof buf, "%ux%ux%d", a, b, t);
            all.emplace_back(cost, buf);
        }
    }
    std::sort(all.begin(), all.end());
    std::vector<std::string> out;
    for (size_t i = 0; i < all.size() && out.size() < max_count; i++) out.push_back(all[i].second);
    return out;
}

// Block size: a multiple of 64 (<= ASX_FFT_THREADS_MAX).  First enough waves per CU to hide
// LDS/HBM latency given how many blocks the LDS footprint admits (target >= 12 waves per CU),
// then the size that wastes the fewest thread slots over the stages (each stage has
// `groups * n / radix` work items); ties go to the larger block.
static int pick_threads(const AsxStages &st, int groups, int min_threads, size_t lds_bytes)
{
    long blocks_per_cu = lds_bytes ? (long)(160 * 1024 / lds_bytes) : 8;
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    if (blocks_per_cu > 8) blocks_per_cu = 8;
    int want = 64 * (int)((12 + blocks_per_cu - 1) / blocks_per_cu);
    if (want > ASX_FFT_THREADS_MAX) want = ASX_FFT_THREADS_MAX;
    if (min_threads < want) min_threads = want;
    long best_cost = -1;
    int best = ASX_FFT_THREADS_MAX;
    for (int bd = 64; bd <= ASX_FFT_THREADS_MAX; bd += 64) {
        if (bd < min_threads) continue;
        long cost = 0;
        for (int i = 0; i < st.nstages; i++) {
            const long items = (long)groups * st.nbf[i];
            cost += (items + bd - 1) / bd * bd;
        }
        if (st.nstages == 0) cost = bd;
        if (best_cost < 0 || cost <= best_cost) { best_cost = cost; best = bd; }
    }
    return best;
}

// Which kernels the plan h runs.  The real-column kernels when the plan allows them (h.rlayout), nothing forces the packed ones and
// BOTH a column and a row entry match; else the packed kernels, columns and rows each on a compiled-in schedule that matches the
// split and the block size, or on the run-time schedule (generic: always that).
static AsxKernelChoice choose_kernels(const AsxHostPlan &h, bool packed, bool generic)
{
    AsxKernelChoice k;
    k.threads_cols = pick_threads(h.st1, h.T / 2, 64, (size_t)h.M1 * h.T * sizeof(float2));
    k.threads_rows = pick_threads(h.st2, 2, (h.M2 + ASX_ROW_STEPS - 1) / ASX_ROW_STEPS, (size_t)4 * h.M2 * sizeof(float2));
    if (const char *e = getenv("ASX_THREADS_COLS")) k.threads_cols = atoi(e);
    if (const char *e = getenv("ASX_THREADS_ROWS")) k.threads_rows = atoi(e);
    if (h.rlayout && !packed) {
        const int c = asx_match_entry(AsxRCols{}, [&](auto e) { return h.T == e.t && schedule_is<typename decltype(e)::sched>(h.st1); });
        const int r = asx_match_entry(AsxRRows{}, [&](auto e) { return h.M2 == e.m2; });
        if (c >= 0 && r >= 0) {
            k.rlayout = true;
            k.cols = c; k.rows = r;
            asx_with_entry(AsxRCols{}, c, [&](auto e) { k.band_rows = 2 * rcol_rows_per_group(decltype(e)::sched::n, e.nt, e.t); });
            // the tile width k_rows_re sums energies for, whole tiles only (AsxSelPrune indexes its flags by M2 / T), and a tile
            // per thread of a k_tile_bounds block
            k.prunable = h.T == ASX_PRUNE_T && h.M2 % ASX_PRUNE_T == 0 && h.ntiles <= 1024;
            return k;
        }
    }
    if (generic) return k;
    k.cols = asx_match_entry(AsxPCols{}, [&](auto e) { return h.T == e.t && k.threads_cols == e.nt && schedule_is<typename decltype(e)::sched>(h.st1); });
    k.rows = asx_match_entry(AsxPRows{}, [&](auto e) { return k.threads_rows == e.nt && schedule_is<typename decltype(e)::sched>(h.st2); });
    return k;
}

static_assert(ASX_ENTRY_INTS <= ASX_KERNEL_ENTRY_CAP, "an entry of kernel_table.h no longer fits the diagnostics' buffers");
bool asx_kernel_table_spell(int list, int index, int *out)
{
    auto spell = [&](auto e) { asx_entry_spell(e, out); };
    out[0] = -1;
    return list == 0 ? asx_with_entry(AsxRCols{}, index, spell) : list == 1 ? asx_with_entry(AsxRRows{}, index, spell)
         : list == 2 ? asx_with_entry(AsxPCols{}, index, spell) : list == 3 && asx_with_entry(AsxPRows{}, index, spell);
}

std::string asx_host_plan_build(size_t N, const char *split_override, AsxHostPlan *hp)
{
    if (N == 0) return "sample_len must be > 0";
    if (N > (size_t)1 << 27) return "sample_len too large";
    hp->N = N;
    uint64_t F = 2 * (uint64_t)N, valid = 2 * (uint64_t)N;
    if (!asx_is_smooth(F)) {
        // embed: r[k] = sum_n s'[n+k] sample[n] with s' the source extended periodically to
        // 3N-1 samples; any smooth even F >= 3N-1 gives the same r[0..2N) without wrap-around.
        valid = 3 * (uint64_t)N - 1;
        F = asx_next_smooth_even(valid);
    }
    if (F >= (1ull << 31)) return "transform length too large";
    hp->F = (uint32_t)F;
    hp->M = (uint32_t)(F / 2);
    hp->src_valid = (uint32_t)valid;
    const uint32_t M = hp->M;
    const int rows_max = (int)(ASX_LDS_ROWS_MAX / (4 * sizeof(float2)));

    int M1 = 0, M2 = 0, T = 0;
    // Measured-best splits for the reference's six interval lengths (src/audiosync.c:50-57) on
    // MI355X, from tools/tune.py (batched float32 path).  Other lengths use the cost model below.
    // The two longest lengths take 2400-point rows so that their column tiles are 400 / 600 packed rows of SIXTEEN real
    // columns (64-byte input pieces, whole 128-byte lines of the intermediates): with 800 / 1200 rows a tile holds eight,
    // and the real-column kernels (rlayout.hip) then re-fetch input lines between four sibling tiles (round 4, measured:
    // k_fwd_cols_r 6.15 GB against 5.09 GB per launch).  $ASX_LAYOUT=packed (the packed-sample kernels, xcorr_kernels.hip)
    // keeps round 3's table: its row kernels have no 2400-point schedule compiled in.
    static const struct { uint32_t M; const char *split; const char *split_packed; } kTuned[] = {
        { 144000u, "300x480x16", nullptr }, { 288000u, "600x480x16", nullptr }, { 480000u, "400x1200x16", nullptr },
        { 720000u, "600x1200x16", nullptr }, { 960000u, "400x2400x16", "800x1200x8" },
        { 1440000u, "600x2400x16", "1200x1200x8" },
    };
    // ASX_LAYOUT=packed forces the packed-sample kernels (A/B runs); ASX_GENERIC their run-time-schedule forms (diagnostic)
    const char *lay = getenv("ASX_LAYOUT");
    const bool generic = getenv("ASX_GENERIC") != nullptr, packed = (lay && !strcmp(lay, "packed")) || generic;
    if (!(split_override && *split_override)) {
        for (const auto &t : kTuned)
            if (t.M == M && F == 2 * (uint64_t)N) split_override = (packed && t.split_packed) ? t.split_packed : t.split;
    }
    if (split_override && *split_override) {
        if (sscanf(split_override, "%dx%dx%d", &M1, &M2, &T) != 3 || M1 < 1 || M2 < 1 ||
            (uint64_t)M1 * (uint64_t)M2 != M || T < 2 || (T & (T - 1)) || T > 64 ||
            (size_t)M1 * T * sizeof(float2) > ASX_LDS_HW_MAX ||
            (size_t)4 * M2 * sizeof(float2) > ASX_LDS_HW_MAX)
            return "bad ASX_SPLIT override";
    } else {
        // Cost of a split: the larger LDS footprint of the two kernel families (KiB; it bounds
        // the blocks per CU), 8 per pass over LDS (stage), 20 if any stage needs radix 15/16
        // (those bodies spill at 128 VGPRs).  Tiles of at least 8 columns (64-byte row
        // segments in HBM) are preferred; narrower ones only if nothing else fits.
        double best_cost = 1e30;
        for (int pass = 0; pass < 2 && M1 == 0; pass++) {
            const int min_T = pass == 0 ? 8 : 2;
            for (uint32_t a = 1; a <= M && a <= 8192u; a++) {
                if (M % a) continue;
                const uint32_t b = M / a;
                if ((int)b > rows_max) continue;
                int t = tile_for((int)a);
                if (t < min_T) continue;
                while (t > 2 && (uint32_t)t > b) t >>= 1; // not wider than the row (but always a column pair)
                AsxStages s1, s2;
                if (!asx_make_stages((int)a, &s1) || !asx_make_stages((int)b, &s2)) continue;
                int maxr = 2;
                for (int i = 0; i < s1.nstages; i++) maxr = std::max(maxr, s1.radix[i]);
                for (int i = 0; i < s2.nstages; i++) maxr = std::max(maxr, s2.radix[i]);
                const double lds = (double)std::max((size_t)a * t * sizeof(float2), (size_t)4 * b * sizeof(float2)) / 1024.0;
                const double cost = lds + 8.0 * (s1.nstages + s2.nstages) + (maxr > 12 ? 20.0 : 0.0);
                if (cost < best_cost || (cost == best_cost && t > T)) {
                    best_cost = cost;
                    M1 = (int)a; M2 = (int)b; T = t;
                }
            }
        }
        if (M1 == 0) return "transform length does not split into LDS-sized factors";
    }
    hp->M1 = M1; hp->M2 = M2; hp->T = T;
    hp->logT = 0;
    while ((1 << hp->logT) < T) hp->logT++;
    hp->ntiles = (M2 + T - 1) / T;
    if (!asx_make_stages(M1, &hp->st1) || !asx_make_stages(M2, &hp->st2))
        return "factor is not {2,3,5}-smooth";

    hp->tw1.resize(M1);
    for (int q = 0; q < M1; q++) hp->tw1[q] = unit_root(q, M1);
    hp->tw2.resize(M2);
    for (int q = 0; q < M2; q++) hp->tw2[q] = unit_root(q, M2);
    hp->tw_lo.resize(ASX_TW_LO);
    for (uint32_t q = 0; q < ASX_TW_LO; q++) hp->tw_lo[q] = unit_root(q, F);
    const uint32_t nhi = (uint32_t)((F + ASX_TW_LO - 1) >> ASX_TW_LOG) + 1;
    hp->tw_hi.resize(nhi);
    for (uint32_t h = 0; h < nhi; h++) hp->tw_hi[h] = unit_root((uint64_t)h << ASX_TW_LOG, F);

    hp->pos1_of_k1 = asx_position_table(hp->st1);
    hp->k1_of_pos1.assign(M1, 0);
    for (int k = 0; k < M1; k++) hp->k1_of_pos1[hp->pos1_of_k1[k]] = k;
    hp->pos2_of_k2 = asx_position_table(hp->st2);
    // w_M2^k2 in SLOT order (tw2s[pos2_of_k2[k2]] = w_M2^k2): the spectral combine of k_rows walks a row
    // slot by slot.  It relies on digit reversal mapping k2 -> M2-1-k2 to slot -> M2-1-slot (all digits
    // complemented); checked here so that a different position table cannot silently break it.
    hp->tw2s.resize(M2);
    for (int k2 = 0; k2 < M2; k2++) {
        if (hp->pos2_of_k2[M2 - 1 - k2] != M2 - 1 - hp->pos2_of_k2[k2]) return "position table is not a digit reversal";
        hp->tw2s[hp->pos2_of_k2[k2]] = hp->tw2[k2];
    }
    hp->row_tasks.resize(M1 / 2 + 1);
    for (int k1 = 0; k1 <= M1 / 2; k1++) {
        const int m1 = (M1 - k1) % M1;
        hp->row_tasks[k1] = make_int4(hp->pos1_of_k1[k1], hp->pos1_of_k1[m1], k1, m1);
    }
    // The real-column kernels (rlayout.hip) untangle the column transforms inside the tile: frequencies u and M1 - u,
    // u <= M1/2, pair up.  One entry per pair, {u, slot of u, slot of M1 - u}, ordered by the first slot so that
    // consecutive lanes walk LDS (almost) slot by slot; col_tw = w_{2 M1}^u in the same order.
    hp->col_pairs.clear();
    hp->col_tw.clear();
    hp->rlayout = false;
    if (M1 % 2 == 0 && F == 2 * (uint64_t)N && M2 % T == 0 && T >= 4 && M2 % 4 == 0) {
        std::vector<std::pair<int, int>> order; // (slot of u, u)
        for (int u = 0; u <= M1 / 2; u++) order.push_back({ hp->pos1_of_k1[u], u });
        std::sort(order.begin(), order.end());
        for (const auto &o : order) {
            const int u = o.second;
            hp->col_pairs.push_back(make_int4(u, o.first, hp->pos1_of_k1[(M1 - u) % M1], 0));
            hp->col_tw.push_back(unit_root((uint64_t)u, 2 * (uint64_t)M1));
        }
        hp->rlayout = true;
    }
    hp->kernels = choose_kernels(*hp, packed, generic);
    return "";
}

// The form of a launch group.  Every rule is stated here and nowhere else.
AsxGroupForm asx_group_form(const AsxGroupAsk &a)
{
    AsxGroupForm f{};
    f.weight = a.weight;
    f.bc = a.bc;
    // A weighted (PHAT) group: the PHAT row flavours and k_phat_finalize, which lists nothing; no pruned pass and no spectral form
    // whatever the plan's switches say -- none of them means anything for a whitened spectrum.
    const bool phat = a.weight != ASX_W_NONE;
    // A caller that does not read the overflow list behind the group (the asynchronous mode) must not leave entries on it.
    f.appends = a.listed && !phat;
    // The spectral Pearson form (pearson_spectral.hip) reads the band sums and tile peaks this group's transform kernels leave: float32
    // inputs of a float32 entry point, on a workspace that has them.
    const bool spectral = a.f32_inputs && a.plan_spectral && a.f32_abi && a.band_sums && !phat;
    f.tail = phat ? ASX_TAIL_PHAT : spectral ? ASX_TAIL_SPECTRAL : ASX_TAIL_DIRECT;
    // The pruned pair of passes (rlayout.hip: k_rows_re, and k_tile_bounds and k_inv_cols_r<..., AsxSelPrune> around k_prune_select):
    // a float32 entry point's group, every lag competing, no broadcast operand and no pool, one pass, r not asked for, the lane's own
    // lists.  Whether the plan's Pearson form is spectral plays no part.  (The plan's switch is only ever on where the pass can run:
    // AsxKernelChoice::prunable, real-column plans.)
    f.pruned = a.plan_prune && !phat && a.f32_inputs && a.f32_abi && !a.pool && a.bc == 0 && !a.r_out && !a.own_lists && a.k == 1 &&
               a.search == AsxSearch::ALL;
    // Partial storing of Q (k_rows_rm): a pruned group of a call that reads the overflow list behind it -- the list is how a pair
    // whose stored set fell short gets its second run, so the asynchronous mode keeps k_rows_re -- and not that second run itself.
    f.qstore = f.pruned && a.listed && a.qstore && a.over_list;
    f.takeback = f.qstore && spectral; // (k_qstore_takeback corrects the spectral form's mode counters)
    f.fwd = a.pool ? ASX_FWD_POOL : a.rlayout ? ASX_FWD_REAL : ASX_FWD_PACKED;
    f.rows = !a.rlayout ? ASX_ROWS_PACKED : f.pruned ? ASX_ROWS_ENERGY : a.pool ? ASX_ROWS_LISTED : ASX_ROWS_PLAIN;
    return f;
}
