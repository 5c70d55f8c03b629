// csrc/asx_api.hip — host side of the HIP layer: plans, workspaces, the C-ABI
// declared in include/audiosync/xcorr_hip.h.  No CPU fallback anywhere: when
// HIP is not usable every entry point fails and says so.
#include "audiosync/xcorr_hip.h"

#include "asx_internal.h"
#include "dev_mem.h"
#include "plan_math.h"
#include "shard_driver.h"
#include "host_narrow.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    // same channel and prefix as the reference's perror("audiosync: ...") calls
    fprintf(stderr, "audiosync: %s\n", buf);
    return -1;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define HIP_TRY_NULL(expr)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
            return nullptr;                                                                   \
        }                                                                                     \
    } while (0)

extern "C" const char *asx_last_error(void) { return g_err.c_str(); }
extern "C" int asx_abi_version(void) { return 2; }

extern "C" int asx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

struct EventPair { // two events that go with their scope
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() { for (hipEvent_t e : { e0, e1 }) if (e) (void)hipEventDestroy(e); }
};

struct DevGuard {
    int prev = -1;
    bool ok = false;
    explicit DevGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// whether s is capturing; a stream that cannot be asked counts as not capturing (the error is cleared)
static bool stream_capturing(hipStream_t s)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
    return cap != hipStreamCaptureStatusNone;
}

extern "C" int asx_current_device(void)
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) return -1;
    return d;
}

// csrc/dev_mem.h bound to HIP: every set of device buffers below is an AsxMemSet over this pair.  A failed take leaves its error
// in g_take_err for the caller's message and no sticky error behind.
static thread_local hipError_t g_take_err = hipSuccess;
static const AsxMemOps hip_mem = {
    [](void **out, size_t bytes) { return (g_take_err = hipMalloc(out, bytes)) == hipSuccess ? 0 : ((void)hipGetLastError(), -1); },
    [](void *ptr) { (void)hipFree(ptr); }
};

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
struct asx_plan {
    int device = 0;
    AsxHostPlan host;
    AsxDev dev{};
    size_t group = 1;          // pairs per launch group
    size_t stamp_blocks = 0;   // diagnostic stamp buffer: blocks x 8 slots
    hipStream_t stream = nullptr;
    std::mutex lock;

    // Who owns the plan's device memory (asx_plan_workspace_bytes: all but the bank's and the NCC sets').  mem: what plan_init takes and, once created,
    // the lazy sets (big, bslot, st, st64: whole or absent); cxy0: lane 0's C_x / C_y, which tune_placement may replace; bank.mem; ncc.mem;
    // ncc.tmem; nccfull.mem; nccfull.pmem; nccrag.mem.
    AsxMemSet mem{ hip_mem }, cxy0{ hip_mem };
    // "Lanes": each owns the workspaces of one launch group and a stream.  With two lanes
    // (ASX_LANES=2) consecutive groups of a batch alternate lanes so that kernels of different
    // groups may overlap; measured gain 0..4 %, less than simply doubling the group, so one
    // lane is the default.
    struct Lane {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        float2 *zxa = nullptr, *zya = nullptr, *ga = nullptr;
        AsxPeakWs pk{};
        AsxSeg *seg = nullptr;
        double *psums = nullptr;
        AsxSpecWs spec{};      // spectral Pearson (pearson_spectral.hip): work list, window sums, mode counters
        AsxTopkWs tk{};        // top-k passes (asx_xcorr_topk_f32_dev): per-pair records and one pass's results
        AsxPrune prune{};      // pruned inverse pass (asx_plan_set_prune): tile energies of Q, bounds, flags
        AsxPoolPair *pool = nullptr; // pool calls (asx_xcorr_pool_f32_dev): the group's pairs as slots and input offsets (k_pool_resolve)
    } lanes[2];
    int nlanes = 1;   // ASX_LANES=2 enables the second lane (measured: +0..4 %)
    hipEvent_t fork = nullptr;
    // Second look for pairs whose near-tie list overflowed (lazy; see second_look): lists that hold
    // every lag of ONE pair
    struct BigPeak {
        AsxCand *cand = nullptr;
        uint32_t *refine_idx = nullptr, *cand_n = nullptr, *refine_n = nullptr;
        double *refine_val = nullptr;
        unsigned long long *overflows = nullptr;
        float *src_dc = nullptr;     // the pair's source minus its mean (float32, 2N)
        double *stats = nullptr;     // {mean of source, sum of sample, their product = the shift of r}
        size_t cap = 0;
    } big;
    // Broadcast slot of asx_xcorr_strided_f32_dev (real-column plans, lazy, like BigPeak): the forward column pass of a track that
    // every pair of a call shares (a stride of 0) -- C_x / C_y of ONE pair, its norm partials and band sums in the AsxPeakWs layout
    // of pair 0 -- written once per call before the launch groups, read by every group's row kernel (k_rows_r, BC != 0)
    AsxSpectra bslot{};
    // Bank of asx_xcorr_pool_f32_dev (real-column plans; allocated at the first pool call, grown when a call names more tracks): the
    // forward column pass of every track of a call's two pools -- source a at row a of cx, sample b at row b of cy, their norm partials
    // and band sums in the AsxPeakWs layout of "pair" a, operand 0, and "pair" b, operand 1 -- written once per call before the launch
    // groups, read by slot (k_pool_resolve, k_rows_rl).  Its own set, replaced wholesale on growth: not part of asx_plan_workspace_bytes.
    struct Bank {
        AsxSpectra c{};
        AsxMemSet mem{ hip_mem };
        size_t nsrc = 0, nsmp = 0;      // capacity in tracks
        unsigned long long fills = 0;   // pool calls that filled it (diagnostic: asx_plan_debug_bank)
    } bank;
    // Normalised cross-correlation (asx_xcorr_ncc_f32_dev; lazy, whole or absent, allocated at the plan's first such call): r of every
    // lag of one NCC group, the per-lag tables of its source tracks and the small sums (AsxNccWs).  group <= the plan's: the set is
    // bounded by ASX_NCC_WS_BYTES (or one pair's share where that is larger).  Its own set: not part of asx_plan_workspace_bytes.
    // The pool calls' track set (asx_xcorr_pool_ncc_f32_dev; lazy, whole or absent, grown like the bank and like it replaced wholesale):
    // the per-lag table, the chunk sums and the statistics of nsrc source and nsmp sample tracks, in the AsxNccWs pointers of those
    // names (`tracks`: its r, best and tk stay null).  Its own set too.  built_*: source tables and sample moment sets formed over
    // the plan's life, by every NCC call (host-side counts: asx_plan_debug_ncc).
    struct Ncc {
        AsxNccWs w{};
        AsxMemSet mem{ hip_mem };
        size_t group = 0;
        AsxNccWs tracks{};
        AsxMemSet tmem{ hip_mem };
        size_t nsrc = 0, nsmp = 0;
        unsigned long long built_src = 0, built_smp = 0;
    } ncc;
    // The full-range NCC calls (asx_xcorr_ncc_full_f32_dev; lazy, whole or absent, allocated at the plan's first such call): what an
    // NCC group holds (w: pass A's r, the tables of the lags >= 0, the small sums) and what the negative lags add (f: pass B's r, the
    // staged sources, the prefix and suffix tables), for one group of `group` pairs.  Its own set, with its own bound
    // (ensure_ncc_full): not part of asx_plan_workspace_bytes.
    struct NccFull {
        struct Set { AsxNccWs w{}; AsxNccFullWs f{}; } set;
        AsxMemSet mem{ hip_mem };
        size_t group = 0;
        // The pool calls' track set (asx_xcorr_pool_ncc_full_f32_dev; lazy, whole or absent, grown like the bank and like it replaced
        // wholesale): per source track x_lo (tracks.stage), its forward column pass (bank.cx: pass B's source rows; its norm partials
        // and band sums in bank.nrm / bank.band, next to a copy of the samples' from the plan's bank) and the prefix table
        // (tracks.ptab), per sample track the suffix table (tracks.ttab).  tracks.rlo and bank.cy stay null in the set: a group's
        // rlo is `set`'s, and pass B's sample rows are the plan's bank's.  Its own set too.  staged / suffixed: sources staged and
        // suffix tables built over the plan's life (host-side counts: asx_plan_debug_ncc_full).
        struct Tracks { AsxNccFullWs tracks{}; AsxSpectra bank{}; } pool;
        AsxMemSet pmem{ hip_mem };
        size_t nsrc = 0, nsmp = 0;
        unsigned long long staged = 0, suffixed = 0;
    } nccfull;
    // The ragged NCC calls (asx_xcorr_ncc_ragged_f32_dev; lazy, whole or absent, allocated at the plan's first such call): per pair of
    // one group the staged tracks, the two r buffers, the prefix tables and the small sums (AsxNccRagWs).  Its own set, with its own
    // bound (ensure_ncc_ragged): not part of asx_plan_workspace_bytes.
    struct NccRag {
        AsxNccRagWs w{};
        AsxMemSet mem{ hip_mem };
        size_t group = 0;
    } nccrag;
    // pairs whose near-tie list overflowed since the list was last emptied (k_finalize appends, resolve_overflows reads)
    uint32_t *over_list = nullptr, *over_n = nullptr;
    volatile uint32_t *h_over_n = nullptr; // page-locked host mirror of *over_n (device-visible: AsxPeakWs::over_host)
    size_t over_cap = 0;
    std::vector<uint32_t> h_over;
    unsigned long long repaired = 0;   // pairs that took the second look
    bool exact = true;                 // asx_plan_set_exact: every entry point takes the second look (default)
    int64_t win_lo = 0, win_hi = 0;    // asx_plan_set_lag_window: the lags whose peak is searched, [-N, N-1] (set at creation) = all
    bool spectral = false;             // float32 groups take the spectral Pearson form (asx_plan_set_pearson; real-column plans)
    unsigned long long *mode_count = nullptr; // [ASX_PM_NMODES], cumulative over the plan's life
    bool prunable = false;             // AsxKernelChoice::prunable: the lanes have their AsxPrune workspaces
    bool prune = false;                // asx_plan_set_prune: in-scope groups skip the inverse column tiles a bound rules out
    unsigned long long *prune_stats = nullptr; // [2] tiles transformed, tiles in all, by the pruned groups; cumulative
    // asx_plan_set_qstore: 0 off, 1 auto, 2 always -- which pruned groups of an exact call store only the predicted tiles of Q
    // (rlayout.hip: asx_qstore_rows, k_rows_rm, k_q_predict; the exact check in k_prune_select, the redo in resolve_overflows)
    int qstore = 1;
    unsigned long long *qstore_stats = nullptr; // [4] pairs given a list, pairs given all, -, tiles stored; cumulative
    uint64_t qstore_redone = 0;                 // pairs whose stored set fell short and that ran again
    // "measure" plans only: at the first device-resident batch the forward column kernel is timed against the caller's buffers
    // on TWO allocations of its output workspaces and the faster set is kept (tune_placement)
    bool tune_placement = false, placement_done = false;
    double placement_ms[2] = { 0.0, 0.0 };
    int placement_kept = -1;
    // staging for the host-pointer entry points (lazy): a group's float32 inputs and results, one pair's float64 inputs
    struct Staging {
        float *src = nullptr, *smp = nullptr;
        int64_t *lag = nullptr; double *coef = nullptr; int32_t *ret = nullptr;
    } st;
    struct Staging64 { double *src = nullptr, *smp = nullptr; } st64;
    float *pin32 = nullptr;            // page-locked staging of the double ABI's narrowed frames (3N floats, lazy)
    unsigned long long narrowed = 0;   // asx_xcorr_f64 calls whose frames crossed PCIe as float32

    // Profiling: HIP events around every kernel family, on the stream the kernels run on.  A ring of
    // the last `prof_depth` batch calls is kept so that consecutive steps can be timed without a
    // host synchronisation between them (6 events per launch group, every group of a call).
    bool profiling = false;
    size_t prof_depth = 1, prof_calls = 0, prof_ring = 0;
    std::vector<std::vector<hipEvent_t>> evr; // ring slot -> 6 events per launch group of that call, grown as needed
    std::vector<size_t> prof_groups; // groups recorded by the call in ring slot i
    size_t ev_groups = 0;            // groups recorded by the call in progress / the latest call
};

// What an entry point on a plan starts with: the plan's lock (the diagnostics take none), the plan's device selected until the
// call returns, and the stream the call works on: the caller's, or the plan's own.
struct PlanCall {
    std::unique_lock<std::mutex> guard;
    DevGuard dg;
    hipStream_t s;
    explicit PlanCall(asx_plan *p, void *stream = nullptr, bool lock = true)
        : guard(lock ? std::unique_lock<std::mutex>(p->lock) : std::unique_lock<std::mutex>()), dg(p->device),
          s(stream ? (hipStream_t)stream : p->stream) {}
};

template <typename T> static int dev_alloc(AsxMemSet &m, T **out, size_t count)
{
    return m.take(out, count) ? fail("hipMalloc(&ptr, bytes) failed: %s (%s:%d)", hipGetErrorString(g_take_err), __FILE__, __LINE__) : 0;
}

template <typename T> static int dev_upload(AsxMemSet &m, const T **out, const std::vector<T> &v)
{
    T *d = nullptr;
    if (dev_alloc(m, &d, v.size()) != 0) return -1;
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return 0;
}

// An AsxSpectra as a set of passes for nsrc source and nsmp sample tracks, its pieces taken from m: the plan's broadcast slot
// (1, 1) and its bank.  -1 when a piece cannot be had; the message is the caller's.
static int take_spectra(const AsxDev &P, AsxMemSet &m, AsxSpectra &c, size_t nsrc, size_t nsmp)
{
    const size_t pitch = asx_spectrum_len(P), na = std::max(nsrc, nsmp), nt = P.ntiles, nb = nt * (size_t)P.nbands;
    return m.take(&c.cx, nsrc * pitch) || m.take(&c.cy, nsmp * pitch) || m.take(&c.nrm, na * 2 * nt) || (nb && m.take(&c.band, na * 2 * nb)) ? -1 : 0;
}

static int plan_init(asx_plan *p, size_t N, size_t max_batch, const char *split)
{
    std::string err = asx_host_plan_build(N, split, &p->host);
    if (!err.empty()) return fail("plan for sample_len=%zu: %s", N, err.c_str());
    const AsxHostPlan &h = p->host;
    AsxDev &d = p->dev;
    AsxMemSet &m = p->mem;
    d.N = (uint32_t)N;
    d.F = h.F; d.M = h.M; d.M1 = h.M1; d.M2 = h.M2; d.T = h.T; d.logT = h.logT; d.ntiles = h.ntiles;
    d.src_valid = h.src_valid;
    d.src_period = (uint32_t)(2 * N);
    d.nout = (uint32_t)(2 * N);
    // the device's r is the unnormalised inverse transform: F times the plain sum of products
    d.bound_scale = 2.0f * ASX_BOUND_C * 5.9604645e-8f * log2f((float)h.F) * (float)h.F;
    d.st1 = h.st1; d.st2 = h.st2;
    // Which kernels run was decided with the host plan (AsxKernelChoice, plan_math.cpp): the real-column kernels (rlayout.hip) when
    // the plan allows them and they are compiled in for its schedules (the reference's six lengths), else the packed-sample kernels
    const AsxKernelChoice &k = h.kernels;
    // (the one check of it: a real-column plan without an entry has no kernel; the launchers look up and do not ask again)
    if (k.rlayout && (k.cols < 0 || k.rows < 0 || !h.rlayout)) return fail("internal: a real-column plan without its kernels");
    d.threads_cols = k.threads_cols; d.threads_rows = k.threads_rows;
    d.rlayout = k.rlayout ? 1 : 0;
    d.kcols = k.cols; d.krows = k.rows;
    d.band_rows = k.band_rows;
    d.nbands = k.band_rows ? 2 * h.M1 / k.band_rows : 0;
    p->prunable = k.prunable;
    if (dev_upload(m, &d.tw1, h.tw1) || dev_upload(m, &d.tw2, h.tw2) || dev_upload(m, &d.tw2s, h.tw2s) || dev_upload(m, &d.tw_lo, h.tw_lo) ||
        dev_upload(m, &d.tw_hi, h.tw_hi) ||
        dev_upload(m, &d.k1_of_pos1, h.k1_of_pos1) || dev_upload(m, &d.pos1_of_k1, h.pos1_of_k1) ||
        dev_upload(m, &d.pos2_of_k2, h.pos2_of_k2) || dev_upload(m, &d.row_tasks, h.row_tasks))
        return -1;

    d.col_pairs = nullptr;
    d.col_tw = nullptr;
    if (k.rlayout && (dev_upload(m, &d.col_pairs, h.col_pairs) || dev_upload(m, &d.col_tw, h.col_tw))) return -1;
    // group size: keep the three inter-kernel intermediates (24*M bytes per pair) of one
    // group around the size of the 256 MiB Infinity Cache so the next kernel re-reads them on die
    size_t ws_mb = 4096;
    if (const char *e = getenv("ASX_WS_MB")) ws_mb = (size_t)atol(e) > 0 ? (size_t)atol(e) : ws_mb;
    size_t per_pair = (size_t)3 * h.M * sizeof(float2);
    size_t g = (ws_mb << 20) / per_pair / (getenv("ASX_LANES") && atoi(getenv("ASX_LANES")) == 2 ? 2 : 1);
    if (g < 1) g = 1;
    if (g > 65535) g = 65535; // grid.y / grid.z limit
    if (max_batch < 1) max_batch = 1;
    if (g > max_batch) g = max_batch;
    p->group = g;
    if (const char *e = getenv("ASX_LANES")) p->nlanes = atoi(e) == 2 ? 2 : 1;
    // candidate capacity per pair of the peak refinement (asx_internal.h): all 2N lags for short
    // tracks, else N/64 clamped to [ASX_CAND_MIN, ASX_CAND_MAX]
    size_t cap = std::min<size_t>(std::max<size_t>(N / 64, ASX_CAND_MIN), ASX_CAND_MAX);
    cap = std::min<size_t>(cap, 2 * N);
    for (int l = 0; l < p->nlanes; l++) {
        asx_plan::Lane &ln = p->lanes[l];
        ln.pk.cap = (uint32_t)cap;
        const size_t mz = asx_spectrum_len(d);
        AsxMemSet &cxy = l == 0 ? p->cxy0 : m;
        if (dev_alloc(cxy, &ln.zxa, g * mz) || dev_alloc(cxy, &ln.zya, g * mz) || dev_alloc(m, &ln.ga, g * mz) ||
            dev_alloc(m, &ln.pk.nrm_part, g * 2 * (size_t)h.ntiles) || dev_alloc(m, &ln.pk.bound2, g) ||
            dev_alloc(m, &ln.pk.pairmax, g) || dev_alloc(m, &ln.pk.cand_n, g) ||
            dev_alloc(m, &ln.pk.cand, g * cap) || dev_alloc(m, &ln.pk.refine_n, g) ||
            dev_alloc(m, &ln.pk.refine_idx, g * cap) || dev_alloc(m, &ln.pk.refine_val, g * cap) ||
            dev_alloc(m, &ln.pk.overflows, 1) ||
            dev_alloc(m, &ln.seg, g) || dev_alloc(m, &ln.psums, g * (size_t)asx_pearson_blocks((uint32_t)N) * 6) ||
            dev_alloc(m, &ln.tk.pairs, g) || dev_alloc(m, &ln.tk.lag, g) || dev_alloc(m, &ln.tk.coef, g) || dev_alloc(m, &ln.tk.ret, g) ||
            dev_alloc(m, &ln.tk.sink, 1) || dev_alloc(m, &ln.pool, g))
            return -1;
        HIP_TRY(hipMemset(ln.pk.overflows, 0, sizeof(unsigned long long)));
        ln.pk.band = nullptr; ln.pk.tile_peak = nullptr;
        if (d.rlayout) {
            // spectral Pearson: band sums of both tracks (the sample fills the first half of its bands), one signed peak value
            // per inverse tile, the work list and the window sums of the group's pairs
            const size_t nbands = (size_t)d.nbands;
            if (!p->mode_count) {
                if (dev_alloc(m, &p->mode_count, ASX_PM_NMODES)) return -1;
                HIP_TRY(hipMemset(p->mode_count, 0, ASX_PM_NMODES * sizeof(unsigned long long)));
            }
            if (dev_alloc(m, &ln.pk.band, g * 2 * nbands * (size_t)h.ntiles) || dev_alloc(m, &ln.pk.tile_peak, g * (size_t)(h.M2 / h.T)) ||
                dev_alloc(m, &ln.spec.part, g * ASX_PREP_BLOCKS_MAX * 4) || dev_alloc(m, &ln.spec.hdr, g * ASX_SPEC_HDR))
                return -1;
            ln.spec.mode_count = p->mode_count;
            ln.spec.tol = 1e-5;
        }
        if (p->prunable) {
            // pruned inverse pass: 4 (M1 + 1) ntiles bytes per pair, about 1 % of Q; the group size does not depend on it
            if (!p->prune_stats) {
                if (dev_alloc(m, &p->prune_stats, 2)) return -1;
                HIP_TRY(hipMemset(p->prune_stats, 0, 2 * sizeof(unsigned long long)));
            }
            if (dev_alloc(m, &ln.prune.eng, g * ((size_t)h.M1 + 1) * (size_t)h.ntiles) || dev_alloc(m, &ln.prune.ub, g * (size_t)h.ntiles) ||
                dev_alloc(m, &ln.prune.best, g) || dev_alloc(m, &ln.prune.skip, g * (size_t)h.ntiles) ||
                dev_alloc(m, &ln.prune.part, g * 1024) || dev_alloc(m, &ln.prune.ticket, g) || dev_alloc(m, &ln.prune.list, g) ||
                dev_alloc(m, &ln.prune.redo, g))
                return -1;
            if (!p->qstore_stats) {
                if (dev_alloc(m, &p->qstore_stats, 4)) return -1;
                HIP_TRY(hipMemset(p->qstore_stats, 0, 4 * sizeof(unsigned long long)));
            }
            HIP_TRY(hipMemset(ln.prune.redo, 0, g));
            ln.prune.qstats = p->qstore_stats;
            // part: [slices][tiles rounded up to 32] of 1024 doubles per pair whatever the length; every slot a launch reads it has
            // written itself, the zeroing is for a defined first state only.  The tickets must be zero: k_tile_bounds counts on it
            // and leaves them zero behind every launch
            HIP_TRY(hipMemset(ln.prune.part, 0, g * 1024 * sizeof(double)));
            HIP_TRY(hipMemset(ln.prune.ticket, 0, g * sizeof(unsigned)));
            ln.prune.stats = p->prune_stats;
        }
        HIP_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
    }
    // the list of overflowed pairs is one per plan (the lanes append with atomics); a "window" of a device-resident
    // batch between two looks at it never holds more pairs than this
    p->over_cap = std::max<size_t>(g * (size_t)p->nlanes, 1024);
    if (dev_alloc(m, &p->over_list, p->over_cap) || dev_alloc(m, &p->over_n, 1)) return -1;
    HIP_TRY(hipMemset(p->over_n, 0, sizeof(uint32_t)));
    uint32_t *d_over_host = nullptr;
    {
        void *h = nullptr, *dptr = nullptr;
        HIP_TRY(hipHostMalloc(&h, sizeof(uint32_t), hipHostMallocMapped));
        p->h_over_n = (volatile uint32_t *)h;
        *p->h_over_n = 0;
        HIP_TRY(hipHostGetDevicePointer(&dptr, h, 0));
        d_over_host = (uint32_t *)dptr;
    }
    for (int l = 0; l < p->nlanes; l++) {
        p->lanes[l].pk.over_list = p->over_list;
        p->lanes[l].pk.over_n = p->over_n;
        p->lanes[l].pk.over_host = d_over_host;
        p->lanes[l].pk.over_cap = (uint32_t)p->over_cap;
    }
    p->spectral = d.rlayout != 0;
    if (const char *e = getenv("ASX_PEARSON")) p->spectral = p->spectral && strcmp(e, "direct") != 0; // A/B of the two forms
    p->prune = p->prunable;
    if (const char *e = getenv("ASX_PRUNE")) p->prune = p->prune && atoi(e) != 0; // A/B of the pruned inverse pass
    if (const char *e = getenv("ASX_QSTORE")) p->qstore = std::min(2, std::max(0, atoi(e))); // A/B of partial storing
    if (const char *e = getenv("ASX_EXACT")) p->exact = atoi(e) != 0; // initial value of asx_plan_set_exact (A/B of its cost)
    p->win_lo = -(int64_t)p->host.N; // the full lag window
    p->win_hi = (int64_t)p->host.N - 1;
    HIP_TRY(hipEventCreateWithFlags(&p->fork, hipEventDisableTiming));
    d.stamps = nullptr;
    d.stamp_kernel = 0;
    if (const char *e = getenv("ASX_STAMPS")) {
        unsigned long long *st = nullptr;
        p->stamp_blocks = g * (size_t)std::max(h.M1 + 1, 2 * h.ntiles);
        if (dev_alloc(m, &st, p->stamp_blocks * 8)) return -1;
        HIP_TRY(hipMemset(st, 0, p->stamp_blocks * 8 * sizeof(unsigned long long)));
        d.stamps = st;
        d.stamp_kernel = !strcmp(e, "fwd") ? 1 : !strcmp(e, "inv") ? 2 : 0;
    }
    {
        AsxDev *dcopy = nullptr;
        if (dev_alloc(m, &dcopy, 1)) return -1;
        d.self_dev = dcopy;
        HIP_TRY(hipMemcpy(dcopy, &d, sizeof(AsxDev), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipStreamCreate(&p->stream));
    // the tables and the memsets above went through the null stream; the lanes' streams are non-blocking
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// Measured mode (what FFTW_MEASURE is to FFTW_ESTIMATE): the planner's cost model is only a model --
// for lengths outside its tuned table its pick was up to 27 % slower than the best split -- so time
// its cheapest candidates (plus its own pick) on the device, on synthetic pairs, and return the
// fastest.  About 20 plans are built and run; a fraction of a second per sample length.
static std::string measure_best_split(size_t N, size_t max_batch, int device)
{
    std::vector<std::string> cands = asx_host_plan_candidates(N, 16);
    {
        AsxHostPlan h;
        if (asx_host_plan_build(N, "", &h).empty()) {
            char buf[64];
            snprintf(buf, sizeof buf, "%dx%dx%d", h.M1, h.M2, h.T);
            if (std::find(cands.begin(), cands.end(), std::string(buf)) == cands.end()) cands.insert(cands.begin(), buf);
        }
    }
    if (cands.empty()) return "";
    size_t probe = ((size_t)512 << 20) / (12 * N); // at most 512 MB of float32 inputs
    probe = std::max<size_t>(probe, 4);
    probe = std::min<size_t>(probe, 1024);
    probe = std::max<size_t>(1, std::min(probe, max_batch));
    AsxMemSet m(hip_mem); // the probe's pairs and results
    asx_plan::Staging d;
    std::string best;
    float best_ms = 0.f;
    EventPair ev;
    if (!m.take(&d.src, probe * 2 * N) && !m.take(&d.smp, probe * N) && !m.take(&d.lag, probe) && !m.take(&d.coef, probe) &&
        !m.take(&d.ret, probe) && hipEventCreate(&ev.e0) == hipSuccess && hipEventCreate(&ev.e1) == hipSuccess &&
        asx_synth_pairs_dev(12345, 0, probe, N, 1, d.src, d.smp, nullptr, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess) {
        for (const std::string &c : cands) {
            asx_plan *p = asx_plan_create_ex(N, probe, device, c.c_str());
            if (!p) continue;
            bool ok = asx_xcorr_batch_f32_dev(p, d.src, d.smp, probe, d.lag, d.coef, d.ret, nullptr) == 0; // warm-up
            float ms = 0.f;
            if (ok) {
                ok = hipEventRecord(ev.e0, p->stream) == hipSuccess;
                for (int r = 0; r < 2 && ok; r++) ok = asx_xcorr_batch_f32_dev(p, d.src, d.smp, probe, d.lag, d.coef, d.ret, nullptr) == 0;
                ok = ok && hipEventRecord(ev.e1, p->stream) == hipSuccess && hipEventSynchronize(ev.e1) == hipSuccess &&
                     hipEventElapsedTime(&ms, ev.e0, ev.e1) == hipSuccess;
            }
            asx_plan_destroy(p);
            if (ok && (best.empty() || ms < best_ms)) { best = c; best_ms = ms; }
        }
    }
    (void)hipGetLastError();
    return best;
}

extern "C" asx_plan *asx_plan_create_ex(size_t sample_len, size_t max_batch, int device, const char *split)
{
    if (!split || !*split) split = getenv("ASX_SPLIT");
    if (split && !strcmp(split, "measure")) {
        int prev = 0, ndev0 = 0;
        if (hipGetDeviceCount(&ndev0) != hipSuccess || ndev0 == 0) {
            fail("no usable HIP device; this library has no CPU fallback");
            return nullptr;
        }
        HIP_TRY_NULL(hipGetDevice(&prev));
        const int dev = device < 0 ? prev : device;
        if (dev >= ndev0) { fail("device %d out of range (%d devices)", dev, ndev0); return nullptr; }
        HIP_TRY_NULL(hipSetDevice(dev));
        const std::string best = measure_best_split(sample_len, max_batch ? max_batch : 1, dev);
        (void)hipSetDevice(prev);
        // an empty result (nothing could be timed) falls back to the planner's own choice
        asx_plan *mp = asx_plan_create_ex(sample_len, max_batch, device, best.empty() ? "auto" : best.c_str());
        if (mp) mp->tune_placement = true;
        return mp;
    }
    if (split && !strcmp(split, "auto")) split = "";
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        fail("no usable HIP device (%s); this library has no CPU fallback",
             e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0) HIP_TRY_NULL(hipGetDevice(&device));
    if (device >= ndev) {
        fail("device %d out of range (%d devices)", device, ndev);
        return nullptr;
    }
    int prev = 0;
    HIP_TRY_NULL(hipGetDevice(&prev));
    HIP_TRY_NULL(hipSetDevice(device));
    asx_plan *p = new asx_plan();
    p->device = device;
    int rc = plan_init(p, sample_len, max_batch, split);
    (void)hipSetDevice(prev);
    if (rc != 0) {
        asx_plan_destroy(p);
        return nullptr;
    }
    return p;
}

extern "C" asx_plan *asx_plan_create(size_t sample_len, size_t max_batch, int device)
{
    return asx_plan_create_ex(sample_len, max_batch, device, nullptr);
}

extern "C" void asx_plan_destroy(asx_plan *p)
{
    if (!p) return;
    DevGuard dg(p->device); // (until the plan's sets have given their device memory back)
    if (p->stream) { (void)hipStreamSynchronize(p->stream); (void)hipStreamDestroy(p->stream); }
    for (auto &ln : p->lanes) {
        if (ln.stream) { (void)hipStreamSynchronize(ln.stream); (void)hipStreamDestroy(ln.stream); }
        if (ln.done) (void)hipEventDestroy(ln.done);
    }
    if (p->fork) (void)hipEventDestroy(p->fork);
    for (auto &ring : p->evr)
        for (hipEvent_t ev : ring) (void)hipEventDestroy(ev);
    if (p->pin32) (void)hipHostFree(p->pin32);
    if (p->h_over_n) (void)hipHostFree((void *)p->h_over_n);
    delete p;
}

extern "C" size_t asx_plan_sample_len(const asx_plan *p) { return p ? p->host.N : 0; }
extern "C" size_t asx_plan_fft_len(const asx_plan *p) { return p ? p->host.F : 0; }
extern "C" size_t asx_plan_group(const asx_plan *p) { return p ? p->group : 0; }
extern "C" size_t asx_plan_workspace_bytes(const asx_plan *p) { return p ? p->mem.bytes() + p->cxy0.bytes() : 0; }
// diagnostic: copy back the k_rows phase clocks of the last group (needs ASX_STAMPS env + -DASX_STAMPS build)
extern "C" long asx_plan_debug_stamps(asx_plan *p, unsigned long long *out, size_t cap)
{
    if (!p || !p->dev.stamps) return -1;
    size_t n = p->stamp_blocks * 8;
    if (n > cap) n = cap;
    if (hipMemcpy(out, p->dev.stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long)n;
}

extern "C" int asx_plan_peak_overflows(asx_plan *p, uint64_t *count)
{
    if (!p || !count) return fail("asx_plan_peak_overflows: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    unsigned long long total = 0;
    for (int l = 0; l < p->nlanes; l++) {
        unsigned long long v = 0;
        HIP_TRY(hipStreamSynchronize(p->lanes[l].stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        HIP_TRY(hipMemcpy(&v, p->lanes[l].pk.overflows, sizeof(v), hipMemcpyDeviceToHost));
        total += v;
    }
    *count = total;
    return 0;
}

extern "C" int asx_plan_set_exact(asx_plan *p, int on)
{
    if (!p) return fail("asx_plan_set_exact: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    // whatever the asynchronous mode left on the list belongs to calls that have returned: start empty.  The whole
    // device is drained, not only the plan's own streams: an asynchronous batch may still be in flight on a stream the
    // CALLER supplied (asx_xcorr_batch_f32_dev's `stream`), and its k_finalize adds to the count this resets.
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(p->over_n, 0, sizeof(uint32_t)));
    *p->h_over_n = 0;
    p->exact = on != 0;
    return 0;
}

extern "C" int asx_plan_set_pearson(asx_plan *p, int spectral)
{
    if (!p) return fail("asx_plan_set_pearson: null argument");
    std::lock_guard<std::mutex> guard(p->lock);
    if (spectral && !p->dev.rlayout) return fail("asx_plan_set_pearson: the spectral form needs a real-column plan (the reference's six lengths)");
    p->spectral = spectral != 0;
    return 0;
}

extern "C" int asx_plan_pearson_modes(asx_plan *p, uint64_t counts[3])
{
    if (!p || !counts) return fail("asx_plan_pearson_modes: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    counts[0] = counts[1] = counts[2] = 0;
    if (!p->mode_count) return 0;
    // the whole device, as asx_plan_set_exact does: a batch on a caller-supplied stream (asx_xcorr_batch_f32_dev) is on none of the
    // plan's own streams, and its pairs would be missing from the counts
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[ASX_PM_NMODES];
    HIP_TRY(hipMemcpy(v, p->mode_count, sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; i++) counts[i] = v[i];
    return 0;
}

extern "C" int asx_plan_set_prune(asx_plan *p, int on)
{
    if (!p) return fail("asx_plan_set_prune: null argument");
    std::lock_guard<std::mutex> guard(p->lock);
    if (on && !p->prunable)
        return fail("asx_plan_set_prune: the pruned inverse pass needs a real-column plan (the reference's six lengths)");
    p->prune = on != 0;
    return 0;
}

extern "C" int asx_plan_prune_stats(asx_plan *p, uint64_t *tiles_transformed, uint64_t *tiles_total)
{
    if (!p || !tiles_transformed || !tiles_total) return fail("asx_plan_prune_stats: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    *tiles_transformed = *tiles_total = 0;
    if (!p->prune_stats) return 0;
    HIP_TRY(hipDeviceSynchronize()); // the whole device, as asx_plan_pearson_modes does
    unsigned long long v[2];
    HIP_TRY(hipMemcpy(v, p->prune_stats, sizeof v, hipMemcpyDeviceToHost));
    *tiles_transformed = v[0];
    *tiles_total = v[1];
    return 0;
}

extern "C" int asx_plan_set_qstore(asx_plan *p, int mode)
{
    if (!p) return fail("asx_plan_set_qstore: null argument");
    if (mode < 0 || mode > 2) return fail("asx_plan_set_qstore: mode %d (0 off, 1 auto, 2 always)", mode);
    std::lock_guard<std::mutex> guard(p->lock);
    p->qstore = mode;
    return 0;
}

extern "C" int asx_plan_qstore_stats(asx_plan *p, uint64_t out[4])
{
    if (!p || !out) return fail("asx_plan_qstore_stats: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!p->qstore_stats) return 0;
    HIP_TRY(hipDeviceSynchronize()); // the whole device, as asx_plan_pearson_modes does
    unsigned long long v[4];
    HIP_TRY(hipMemcpy(v, p->qstore_stats, sizeof v, hipMemcpyDeviceToHost));
    out[0] = v[0]; out[1] = v[1]; out[2] = p->qstore_redone; out[3] = v[3];
    return 0;
}

extern "C" int asx_plan_peak_repairs(asx_plan *p, uint64_t *count)
{
    if (!p || !count) return fail("asx_plan_peak_repairs: null argument");
    std::lock_guard<std::mutex> guard(p->lock);
    *count = p->repaired;
    return 0;
}

// diagnostic (not in the public header): the peak-search state of pair `pair` of the last group on lane 0
extern "C" int asx_plan_debug_peak(asx_plan *p, size_t pair, float *bound2, uint32_t *cand_n, uint32_t *refine_n,
                                   unsigned long long *pairmax, double *vals, uint32_t *idxs, size_t cap)
{
    if (!p || pair >= p->group) return -1;
    PlanCall c(p, nullptr, false);
    const AsxPeakWs &W = p->lanes[0].pk;
    (void)hipDeviceSynchronize();
    if (hipMemcpy(bound2, W.bound2 + pair, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(cand_n, W.cand_n + pair, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(refine_n, W.refine_n + pair, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(pairmax, W.pairmax + pair, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    size_t n = std::min<size_t>(cap, W.cap);
    if (vals && hipMemcpy(vals, W.refine_val + pair * (size_t)W.cap, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (idxs && hipMemcpy(idxs, W.refine_idx + pair * (size_t)W.cap, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

// diagnostic (not in the public header): what the spectral Pearson form (pearson_spectral.hip) built the coefficient of pair `pair`
// of the last group on lane 0 from.  Real-column plans only.
//   dims[4]   ntiles, nbands, band_rows, blocks of k_pearson_prep per pair
//   band      null, or [2][ntiles][nbands] {sum, sum of squares} (float pairs; band_cap = the floats it holds, at least
//             4 ntiles nbands): operand 0 the source, operand 1 the sample, whose bands past nbands / 2 were never written
//   hdr[4]    r[peak], the bound on its error, the direct flag, the mode k_pearson_partial recorded
//   seg[6]    lag, src_off, smp_off, len, peak, flags of the pair's AsxSeg
//   pick[8]   mode, n, Sx, Sxx, Sy, Syy, r, bound: asx_spec_pick evaluated ON THE DEVICE from that state (k_debug_spec_pick)
// Synchronises the device; what it allocates lives for the call alone.
extern "C" int asx_plan_debug_spectral(asx_plan *p, size_t pair, int *dims, float *band, size_t band_cap, double *hdr,
                                       long long *seg, double *pick)
{
    if (!p || pair >= p->group || !dims || !hdr || !seg || !pick) return -1;
    const asx_plan::Lane &W = p->lanes[0];
    if (!p->dev.rlayout || !W.pk.band || !W.spec.hdr) return -1;
    PlanCall c(p, nullptr, false);
    if (!c.dg.ok || hipDeviceSynchronize() != hipSuccess) return -1;
    const AsxDev &P = p->dev;
    const size_t cells = (size_t)P.ntiles * (size_t)P.nbands;
    if (band) {
        if (band_cap < 4 * cells) return -1;
        if (hipMemcpy(band, W.pk.band + pair * 2 * cells, 2 * cells * sizeof(float2), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    AsxSeg sg;
    if (hipMemcpy(hdr, W.spec.hdr + pair * ASX_SPEC_HDR, ASX_SPEC_HDR * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&sg, W.seg + pair, sizeof sg, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    seg[0] = sg.lag; seg[1] = sg.src_off; seg[2] = sg.smp_off; seg[3] = sg.len; seg[4] = sg.peak; seg[5] = sg.flags;
    AsxMemSet tmp(hip_mem);
    double *d_pick = nullptr;
    if (tmp.take(&d_pick, 8)) return -1;
    const int nb = asx_launch_debug_spec_pick(P, W.spec, W.seg, pair, d_pick, p->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess ||
        hipMemcpy(pick, d_pick, 8 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    dims[0] = P.ntiles; dims[1] = P.nbands; dims[2] = P.band_rows; dims[3] = nb;
    return 0;
}

// diagnostic (not in the public header): the pruned pass's bounds ub[0 .. n) and largest-bound tile of pair `pair` of the last pruned
// group on lane 0 (n <= the plan's tile count)
extern "C" int asx_plan_debug_prune(asx_plan *p, size_t pair, float *ub, int *best, size_t n)
{
    if (!p || pair >= p->group || !p->lanes[0].prune.ub || n > (size_t)p->host.ntiles) return -1;
    PlanCall c(p, nullptr, false);
    if (!c.dg.ok || hipDeviceSynchronize() != hipSuccess) return -1;
    const AsxPrune &U = p->lanes[0].prune;
    if (ub && hipMemcpy(ub, U.ub + pair * (size_t)p->host.ntiles, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (best && hipMemcpy(best, U.best + pair, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

// diagnostic (not in the public header): the plan's list of overflowed pairs as it stands -- the device's count and its host mirror --
// without emptying it (synchronises the device; asx_plan_set_exact would empty it)
extern "C" int asx_plan_debug_over_list(asx_plan *p, uint32_t *dev_n, uint32_t *host_n)
{
    if (!p || !dev_n || !host_n) return -1;
    PlanCall c(p, nullptr, false);
    if (!c.dg.ok || hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(dev_n, p->over_n, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    *host_n = *p->h_over_n;
    return 0;
}

extern "C" size_t asx_plan_peak_capacity(const asx_plan *p) { return p ? p->lanes[0].pk.cap : 0; }

// The window is plain host state under the plan's lock, read by run_group when it launches: no allocation, no synchronisation.
extern "C" int asx_plan_set_lag_window(asx_plan *p, int64_t lag_min, int64_t lag_max)
{
    if (!p) return fail("asx_plan_set_lag_window: null plan");
    const int64_t N = (int64_t)p->host.N;
    if (lag_min < -N || lag_max > N - 1 || lag_min > lag_max)
        return fail("asx_plan_set_lag_window: [%lld, %lld] is not a window inside [%lld, %lld] with lag_min <= lag_max",
                    (long long)lag_min, (long long)lag_max, (long long)-N, (long long)(N - 1));
    std::lock_guard<std::mutex> guard(p->lock);
    p->win_lo = lag_min;
    p->win_hi = lag_max;
    return 0;
}

extern "C" int asx_plan_lag_window(const asx_plan *p, int64_t *lag_min, int64_t *lag_max)
{
    if (!p || !lag_min || !lag_max) return fail("asx_plan_lag_window: null argument");
    std::lock_guard<std::mutex> guard(const_cast<asx_plan *>(p)->lock);
    *lag_min = p->win_lo;
    *lag_max = p->win_hi;
    return 0;
}

extern "C" int asx_plan_threads(const asx_plan *p, int *cols, int *rows)
{
    if (!p) return -1;
    if (cols) *cols = p->dev.threads_cols;
    if (rows) *rows = p->dev.threads_rows;
    return 0;
}

extern "C" int asx_plan_layout(const asx_plan *p) { return p ? p->dev.rlayout : -1; }

extern "C" int asx_plan_narrowed_calls(asx_plan *p, uint64_t *count)
{
    if (!p || !count) return fail("asx_plan_narrowed_calls: null argument");
    std::lock_guard<std::mutex> guard(p->lock);
    *count = p->narrowed;
    return 0;
}

extern "C" int asx_plan_split(const asx_plan *p, int *m1, int *m2, int *tile_cols)
{
    if (!p) return -1;
    if (m1) *m1 = p->host.M1;
    if (m2) *m2 = p->host.M2;
    if (tile_cols) *tile_cols = p->host.T;
    return 0;
}

// ---------------------------------------------------------------------------
// running groups
// ---------------------------------------------------------------------------
static void prof_begin_call(asx_plan *p)
{
    p->ev_groups = 0;
    if (!p->profiling) return;
    p->prof_ring = p->prof_calls % p->prof_depth;
    if (p->prof_groups.size() < p->prof_depth) p->prof_groups.resize(p->prof_depth, 0);
    if (p->evr.size() < p->prof_depth) p->evr.resize(p->prof_depth);
    p->prof_groups[p->prof_ring] = 0;
}
static void prof_end_call(asx_plan *p, size_t groups)
{
    if (!p->profiling) return;
    p->ev_groups = groups;
    p->prof_groups[p->prof_ring] = groups;
    p->prof_calls++;
}

// every launch group of a call is recorded: the ring slot's event list grows with the call
static int prof_mark(asx_plan *p, hipStream_t s, size_t slot)
{
    if (!p->profiling) return 0;
    std::vector<hipEvent_t> &ev = p->evr[p->prof_ring];
    while (ev.size() <= slot) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ev[slot], s));
    return 0;
}

// The pairs of a call, device resident: pair k is source src + k * src_step and sample smp + k * smp_step (elements).  The
// transforms read the float32 views, the exact passes (refine dots, Pearson, DC removal) the TIn views at the same steps: the
// caller's values when they are not float32, else the same buffers.  bc bit 0 / 1: the source / sample is the call's broadcast
// track (asx_xcorr_strided_f32_dev, real-column plans), whose forward column pass is already in the plan's slot.  win: null, or the
// per-pair lag windows of asx_xcorr_windowed_f32_dev -- pair k's row {lag_min, lag_max} is win + 2 k win_step (device memory) --
// which then replace the plan's window for these pairs.  pool: a pool call (asx_xcorr_pool_f32_dev) -- src / smp are the two pools,
// the steps their strides, and pair k is the call's pair first + k: {source a, sample b} from the caller's rows (or the implicit
// product), resolved on the device per group (k_pool_resolve); at() moves first and the window rows, not the pools.
struct PoolCall {
    const int32_t *rows;   // [batch][2] {a, b}, device memory; null: pair i = (i / nsmp, i % nsmp)
    size_t nsrc, nsmp;
};
template <typename TIn> struct Pairs {
    const float *src, *smp;
    const TIn *tsrc, *tsmp;
    size_t src_step, smp_step;
    int bc;
    const int64_t *win = nullptr;
    size_t win_step = 0;
    const PoolCall *pool = nullptr;
    size_t first = 0;
    // The shapes the entry points use.  staged: pair k at [k][2N] / [k][N], the transforms' float32 views apart from what the exact
    // passes read (the double ABI, the second look's source minus its mean); win: one pair's window row, or null.
    static Pairs staged(const float *src, const float *smp, const TIn *tsrc, const TIn *tsmp, size_t N, const int64_t *win = nullptr,
                        size_t win_step = 0)
    {
        return { .src = src, .smp = smp, .tsrc = tsrc, .tsmp = tsmp, .src_step = 2 * N, .smp_step = N, .bc = 0, .win = win, .win_step = win_step };
    }
    // contiguous float32 pairs, [batch][2N] and [batch][N]
    static Pairs contiguous(const float *src, const float *smp, size_t N) { return staged(src, smp, src, smp, N); }
    // float32 pairs src_step / smp_step apart (0: the call's broadcast track, whose bit of bc a real-column plan sets), per-pair windows or null
    static Pairs strided(const float *src, size_t src_step, const float *smp, size_t smp_step, int bc, const int64_t *win, size_t win_step)
    {
        return { .src = src, .smp = smp, .tsrc = src, .tsmp = smp, .src_step = src_step, .smp_step = smp_step, .bc = bc, .win = win, .win_step = win_step };
    }
    // the pairs of a pool call: the two pools and their strides, pair k = the call's pair k
    static Pairs pooled(const PoolCall *pool, const float *srcs, size_t src_stride, const float *smps, size_t smp_stride, const int64_t *win,
                        size_t win_step)
    {
        Pairs x = strided(srcs, src_stride, smps, smp_stride, 0, win, win_step);
        x.pool = pool;
        return x;
    }
    // one pair of a pool call on explicit pointers (the second look): source a against sample b, with this pair's window row
    Pairs pool_pair(size_t a, size_t b, size_t N) const
    {
        return staged(src + a * src_step, smp + b * smp_step, tsrc + a * src_step, tsmp + b * smp_step, N, win, win_step);
    }
    Pairs at(size_t k) const
    {
        Pairs x = *this;
        if (win) x.win += 2 * k * win_step;
        if (pool) { x.first += k; return x; }
        x.src += k * src_step; x.smp += k * smp_step; x.tsrc += k * src_step; x.tsmp += k * smp_step;
        return x;
    }
    // what the exact passes read (pl: the group's resolved records in a pool call, else null)
    AsxInputs<TIn> inputs(const AsxPoolPair *pl) const { return { tsrc, tsmp, src_step, smp_step, pl }; }
};

// Where pair k's results go (lag and ret may be null): entries step apart (the top-k calls: step = k, entry j of pair i at
// i * k + j; every other entry point: 1).  peak: the PHAT calls' peak heights, an entry each, null everywhere else.
struct Results {
    int64_t *lag;
    double *coef;
    int32_t *ret;
    size_t step = 1;
    double *peak = nullptr;
    Results at(size_t k) const
    {
        return { lag ? lag + k * step : nullptr, coef + k * step, ret ? ret + k * step : nullptr, step, peak ? peak + k * step : nullptr };
    }
};

// The top-k option of a call (asx_xcorr_topk_f32_dev, asx_xcorr_pool_topk_f32_dev): k passes over each group's Q, min_separation between the entries' lags.
// k = 1 is the strided / windowed call itself.
struct Topk {
    int k = 1;
    int64_t sep = 0;
};

// The peak's neighbourhood, which the sub-sample PHAT calls ask for (asx_xcorr_phat_sub_f32_dev): near, 2h + 1 values of r_phat / V
// per pair around its peak (may be null), and frac, the parabolic vertex of the three centre values.  frac null: not asked for.
struct Near {
    double *frac = nullptr;
    double *near = nullptr;
    int h = 0;
    Near at(size_t k) const { return { frac ? frac + k : nullptr, near ? near + k * (size_t)(2 * h + 1) : nullptr, h }; }
};

struct GroupOpts {
    static constexpr size_t no_marks = SIZE_MAX;
    size_t prof_group = 0;       // which group of the call the profiling events time (no_marks: none)
    int lane = 0;
    uint32_t pair_base = 0;      // the group's first pair in the caller's overflow window (what the overflow list records)
    // The caller reads the plan's overflow list behind this group (resolve_overflows).  A caller that does not (the asynchronous
    // mode) must not leave entries on it either: their indices count from ITS buffers, and the next synchronous call would take
    // a second look at its own staging buffers with them.  Marked and counted (ASX_SEG_INEXACT -> ret = 1,
    // asx_plan_peak_overflows) they still are.
    bool listed = true;
    // The group belongs to a float32 entry point's ordinary path, which has two effects (asx_group_form): the spectral Pearson form may
    // run, and the pruned inverse pass may.  Cleared, both are off -- the double ABI (it keeps the float64 reduction over the caller's
    // values even when its frames crossed PCIe as float32), the second look and the r dumps (they exist to see every lag's r and end
    // with the direct form).
    bool f32_abi = true;
    float *r_out = nullptr;      // r of every lag (asx_xcorr_debug_r_dev)
    int dot_blocks = 0;          // blocks per pair of the exact re-evaluation; 0: by the group size
    const AsxPeakWs *pk = nullptr; // the peak workspace instead of the lane's (the second look's lists for every lag)
    Topk topk{};                 // k > 1: passes 2..k over the group's Q (y's entry stride is k)
    // How the product spectrum is weighted (AsxWeight, asx_internal.h; real-column plans): a weighted group runs the row pass's
    // PHAT flavour and the PHAT tail -- k_phat_finalize, the direct Pearson form, k_invalid_rows.  In a pool group the Pearson form
    // reads the pairs' inputs through the group's records, and k_invalid_pairs gives a pair outside its pool a NaN peak too.
    // With topk.k > 1 (the PHAT top-k calls) passes 2..k search the resident Q', each ending in the same tail, and k_topk_peak
    // writes each entry's peak height in front of the step.
    // ASX_W_PHAT_BAND: only the bins of `fband` vote and the peak height is per voter (AsxBand::votes).  The entry points turn the
    // full band into ASX_W_PHAT (band_weight).
    AsxWeight weight = ASX_W_NONE;
    AsxBand fband{};
    bool qstore = true;          // partial storing of Q allowed (false: the second run of a pair whose stored set fell short)
    Near near{};                 // a PHAT group: the group's places for the peak's neighbourhood (k_phat_near behind the tail), or none
    // Not part of the ask: the group ends behind its inverse pass (asx_xcorr_ncc_f32_dev, with r_out) -- no finalize, no exact
    // re-evaluation, no Pearson pass, so no counter moves and y is not written -- and every lag's r is wanted whatever the plan's
    // window says: the search is the full one.
    bool transforms_only = false;
    // A pool group's spectra instead of the plan's bank (null: the bank): pass B of asx_xcorr_pool_ncc_full_f32_dev, whose source rows
    // are those of the staged x_lo tracks and whose sample rows are the bank's own.
    const AsxSpectra *bank = nullptr;
};

// One group: g <= plan->group pairs, the first g of x, results to the first g of y.
template <typename TIn>
static int run_group(asx_plan *p, const Pairs<TIn> &x, size_t g, const Results &y, hipStream_t s, const GroupOpts &o = {})
{
    const AsxDev &P = p->dev;
    asx_plan::Lane &W = p->lanes[o.lane];
    const AsxPeakWs &pk = o.pk ? *o.pk : W.pk;
    auto mark = [&](size_t k) { return o.prof_group != GroupOpts::no_marks && prof_mark(p, s, o.prof_group * 6 + k); };
    const AsxSearch call = o.transforms_only ? AsxSearch::of(-(int64_t)P.N, (int64_t)P.N - 1, P.N, nullptr, 0, W.tk, 0)
                                             : AsxSearch::of(p->win_lo, p->win_hi, P.N, x.win, x.win_step, W.tk, 0); // pass 1's search
    // what the group launches (plan_math.h): decided here, once, and only branched on below
    const AsxGroupForm form = asx_group_form(
        { .rlayout = P.rlayout != 0, .plan_prune = p->prune, .plan_spectral = p->spectral, .band_sums = pk.band != nullptr,
          .over_list = pk.over_list != nullptr, .f32_inputs = std::is_same<TIn, float>::value, .f32_abi = o.f32_abi, .listed = o.listed,
          .r_out = o.r_out != nullptr, .own_lists = o.pk != nullptr, .k = o.topk.k, .search = call.kind, .weight = o.weight,
          .pool = x.pool != nullptr, .bc = x.bc, .qstore = o.qstore });
    const AsxPeakWs fin = form.appends ? pk : asx_peak_unlisted(pk);                      // what k_finalize sees
    const AsxPeakWs tk = form.tail == ASX_TAIL_SPECTRAL ? pk : asx_peak_unbanded(pk);     // what the transform kernels see
    // The group's spectra (AsxSpectra): the lane's own forward passes -- but a broadcast operand's rows are in the plan's slot, and a
    // pool group's in the bank, found through its resolved records -- with the norm partials and band sums always in the lane's places.
    const AsxPoolPair *pl = x.pool ? W.pool : nullptr;
    const AsxSpectra &from = pl ? (o.bank ? *o.bank : p->bank.c) : p->bslot;
    const AsxSpectra C{ (pl || (x.bc & 1)) ? from.cx : W.zxa, (pl || (x.bc & 2)) ? from.cy : W.zya, pk.nrm_part, tk.band, form.bc, pl };
    // The pruned pass's kernels get a copy of the lane's AsxPrune that says whether Q is stored in part: q_rows predictor rows
    // (asx_qstore_rows: the row schedule has the kernel and the plan's switch lets a group of this size in), or 0 and list null = Q is whole.
    AsxPrune U = W.prune;
    U.q_rows = form.qstore ? asx_qstore_rows(P, (int)g, p->qstore) : 0;
    U.q_row_a = P.M1 / 3; // away from the real rows 0 and M1
    U.pair_base = o.pair_base;
    if (!U.q_rows) { U.list = nullptr; U.redo = nullptr; }
    if (mark(0)) return -1;
    if (form.fwd == ASX_FWD_POOL) {
        // pool calls: the bank holds every track's forward column pass; this group only resolves its pairs into slots and offsets
        const AsxPoolArgs A{ x.pool->rows, (uint64_t)x.first, (uint64_t)x.pool->nsrc, (uint64_t)x.pool->nsmp, (uint64_t)x.src_step,
                             (uint64_t)x.smp_step, from.nrm, from.band };
        asx_launch_pool_resolve(P, A, W.pool, C.nrm, C.band, (int)g, s);
    } else if (form.fwd == ASX_FWD_REAL) {
        // the operands that are not the call's broadcast track, whose pass is in the slot: only its norm partials and band sums are copied
        asx_launch_fwd_cols_r(P, (x.bc & 1) ? nullptr : x.src, x.src_step, (x.bc & 2) ? nullptr : x.smp, x.smp_step, 0, (int)g, C, false, s);
        for (unsigned which = 0; which < 2; which++)
            if (x.bc & (1 << which)) asx_launch_bcast_aux(P, from.nrm, from.band, C.nrm, C.band, (int)g, which, s);
    } else if (x.src_step == 2 * (size_t)P.N && x.smp_step == P.N) {
        asx_launch_fwd_cols(P, x.src, x.smp, W.zxa, W.zya, tk, (int)g, s);
    } else {
        // packed plans have no strided forward kernel: the contiguous one once per pair at the pair's own inputs (no broadcast
        // slot: every pair transforms its own copy of a shared track)
        for (size_t k = 0; k < g; k++) {
            AsxPeakWs one = tk;
            one.nrm_part = pk.nrm_part + k * 2 * (size_t)P.ntiles;
            asx_launch_fwd_cols(P, x.at(k).src, x.at(k).smp, W.zxa + k * (size_t)P.M, W.zya + k * (size_t)P.M, one, 1, s);
        }
    }
    if (mark(1)) return -1;
    float2 *q = W.ga;
    if (form.rows == ASX_ROWS_PACKED) asx_launch_rows(P, W.zxa, W.zya, q, tk, (int)g, s);
    else asx_launch_rows_r(P, C, form.rows, form.weight, o.fband, form.pruned ? &U : nullptr, q, tk, (int)g, s);
    if (mark(2)) return -1;
    // Top-k (o.topk.k > 1): every pass's results go to the lane's temporaries, and k_topk_step moves them to entry j of y
    const int K = o.topk.k;
    const Results out = K > 1 ? Results{ W.tk.lag, W.tk.coef, W.tk.ret } : y;
    const AsxInputs<TIn> in = x.inputs(pl);
    // Blocks per pair of the exact re-evaluation: a candidate is one whole block's work whatever the grid, so the count only
    // sets how many candidates of a pair are in flight.  Nearly every block of a batch finds no candidate and exits: with 1024
    // pairs, 128 blocks each were 131 072 empty blocks, 25 us of a 2 ms step.
    const int dot_blocks = o.dot_blocks ? o.dot_blocks : (int)std::min<size_t>(ASX_DOT_BLOCKS, std::max<size_t>(8, 16384 / g));
    // The search of pass j + 1 (AsxSearch).  Pass 1: the plan's lag window (asx_plan_set_lag_window) -- the second look at a pair runs
    // through here too, with the window of the call that listed it -- or the per-pair windows (asx_xcorr_windowed_f32_dev), which
    // replace it.  Later passes of a top-k call: each pair's window minus the zones around its earlier entries (the records
    // k_topk_step keeps).
    auto search = [&](int j) { return AsxSearch::of(p->win_lo, p->win_hi, P.N, x.win, x.win_step, W.tk, j); };
    // One pass over the group's Q: the inverse columns, finalize, the exact re-evaluation and Pearson, the lags of `find` competing.
    // first: pass 1, which the profiling marks time and whose r goes to o.r_out.
    const double votes = form.weight == ASX_W_PHAT_BAND ? o.fband.votes(P.N) : (double)P.F; // a PHAT group: the bins that voted
    auto pass = [&](const AsxSearch &find, bool first) -> int {
        float *const r_out = first ? o.r_out : nullptr;
        if (form.rows == ASX_ROWS_PACKED) asx_launch_inv_cols(P, q, tk, r_out, (int)g, s, find);
        else asx_launch_inv_cols_r(P, q, tk, r_out, (int)g, s, find, form.pruned ? &U : nullptr);
        if (first && mark(3)) return -1;
        if (o.transforms_only) return 0;
        if (form.tail == ASX_TAIL_PHAT) {
            // the PHAT tail: the float32 maximum stands (k_phat_finalize), then the reference's coefficient of the samples at that lag
            // (the peak height is per bin that voted; top-k: the step forms each entry's from the running maximum this leaves alone)
            asx_launch_phat_finalize(P, fin, W.seg, K > 1 ? nullptr : y.peak, votes, (int)g, s, find);
            if (first && mark(4)) return -1;
            asx_launch_pearson(in, P.N, W.seg, W.psums, out.lag, out.coef, out.ret, (int)g, s);
            // the peak's neighbourhood from the Q' this pass searched, around the index k_phat_finalize settled: it only reads
            if (o.near.frac)
                asx_launch_phat_near(P, q, W.seg, votes, o.near.h, find, pl, o.near.frac, o.near.near, (int)g, s);
            return 0;
        }
        asx_launch_finalize(P, fin, W.seg, (int)g, s, o.pair_base, find);
        // (the spectral form's first kernel applies the rule to the exact values itself: one launch less)
        asx_launch_refine(P, in, pk, W.seg, (int)g, s, dot_blocks, form.tail == ASX_TAIL_DIRECT, find);
        if (first && mark(4)) return -1;
        if (form.tail == ASX_TAIL_DIRECT)
            asx_launch_pearson(in, P.N, W.seg, W.psums, out.lag, out.coef, out.ret, (int)g, s);
        else if constexpr (std::is_same<TIn, float>::value)
            asx_launch_pearson_spectral_f32(P, in, find, tk, W.spec, W.seg, W.psums, out.lag, out.coef, out.ret, (int)g, s);
        return 0;
    };
    if (pass(call, true)) return -1;
    if (U.q_rows && form.takeback) asx_launch_qstore_takeback(U, W.spec, (int)g, s);
    // a pair whose row is not a window: (0, NaN, -2), the others untouched (top-k: k_topk_step writes it for every entry)
    // (a PHAT group: k_phat_finalize has given such a pair a NaN peak)
    if (call.kind == AsxSearch::ROWS && K == 1) asx_launch_invalid_rows(call.rows, P.N, y.lag, y.coef, y.ret, (int)g, s);
    // a pool pair with an index outside its pool: (0, NaN, -4), which takes precedence over -2 (a PHAT group: and a NaN peak over the 0
    // that k_phat_finalize wrote for its empty maximum)
    // (a pool group of an NCC call ends behind its inverse pass: ncc_batch writes that pair's entries behind its own last pass)
    if (pl && K == 1 && !o.transforms_only) asx_launch_invalid_pairs(pl, y.lag, y.coef, y.ret, y.peak, (int)g, s);
    // Passes 2..k over the same Q; the transforms are not run again.  In a pool group the passes read the pairs' inputs through the
    // group's records (the listed kernels), and an invalid pair -- whose Q is NaN and whose bound is zero, so that no pass finds or
    // lists anything for it -- gets (0, NaN, -4) in all k entries behind the last step, over the steps' -2 and -3.
    // A PHAT group's passes search the resident Q' and end in the PHAT tail; k_topk_peak takes the entry's peak height from the
    // pass's running maximum before the step zeroes it.
    for (int j = 0; K > 1 && j < K; j++) {
        if (j > 0 && pass(search(j), false)) return -1;
        if (form.tail == ASX_TAIL_PHAT && y.peak) asx_launch_topk_peak(W.tk, pk, call, P.N, (int)g, j, K, votes, y.peak, s);
        asx_launch_topk_step(W.tk, W.seg, pk, call, P.N, (int)g, j, K, o.topk.sep, y.lag, y.coef, y.ret, s);
    }
    if (pl && K > 1) asx_launch_invalid_pairs_k(pl, K, y.lag, y.coef, y.ret, y.peak, (int)g, s);
    if (mark(5)) return -1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// Second look at the pairs whose near-tie list overflowed (more lags inside the float32 error window than the
// per-pair list holds: a signal periodic in a few frames at a production length has hundreds of thousands of exactly
// tied peaks; an offset of hundreds of deviations in BOTH tracks makes every lag a near-tie).  k_finalize put their
// indices on the plan's list; every entry point reads it -- ONE host synchronisation per call (per window of
// `over_cap` pairs in a long device-resident batch), the price of a lag that is the reference's float64 argmax by
// construction (src/cross_correlation.c:52-67 has no candidate limit) -- and, only when the list is not empty, runs
// each listed pair again through run_group, as a group of one:
//   (i)  its transforms on (source - mean of source): the float32 error bound scales with both norms, and
//        r[k] = r'[k] + mean * sum(sample) exactly, a constant that k_inv_cols adds back when it forms the keys
//        (AsxPeakWs::shift, peak_key_shifted): with the offset gone from the source's norm the window shrinks by the
//        ratio offset / deviation;
//   (ii) into lists that hold all 2N lags; every listed lag is re-evaluated exactly (candidates x N double-double
//        multiply-adds: about 0.2 s for 400 000 candidates at N = 1 440 000, hence 2048 blocks) and the direct Pearson
//        pass is redone on the caller's values for the lag that wins.
// It runs on `s` behind everything the call has launched (the lanes have been joined), in the workspace slot 0 of
// lane 0 and the plan's one set of big lists: nothing else is in flight on this plan (one stream at a time per plan).
// xi is the listed pair itself (explicit pointers, no broadcast slot, no pool), yi its results.
template <typename TIn>
static int second_look(asx_plan *p, const Pairs<TIn> &xi, const Results &yi, hipStream_t s, const Topk &topk)
{
    const AsxDev &P = p->dev;
    const size_t N = p->host.N;
    asx_plan::BigPeak &B = p->big;
    if (!B.cand && asx_mem_whole(p->mem, B, [&](AsxMemSet &m, asx_plan::BigPeak &T) {
            T.cap = 2 * N;
            if (dev_alloc(m, &T.cand, T.cap) || dev_alloc(m, &T.refine_idx, T.cap) || dev_alloc(m, &T.refine_val, T.cap) ||
                dev_alloc(m, &T.cand_n, 1) || dev_alloc(m, &T.refine_n, 1) || dev_alloc(m, &T.overflows, 1) ||
                dev_alloc(m, &T.src_dc, 2 * N) || dev_alloc(m, &T.stats, ASX_DC_STATS_DOUBLES))
                return -1;
            HIP_TRY(hipMemsetAsync(T.overflows, 0, sizeof(unsigned long long), s));
            return 0;
        }))
        return -1;
    // slot 0's norms, bound and running maximum (k_rows recomputes all three); no overflow list and no band sums (the second look
    // ends with the direct Pearson reduction) ...
    AsxPeakWs K = asx_peak_unbanded(asx_peak_unlisted(p->lanes[0].pk));
    K.cand_n = B.cand_n; K.cand = B.cand; // ... with lists for all 2N lags: this look cannot overflow
    K.refine_n = B.refine_n; K.refine_idx = B.refine_idx; K.refine_val = B.refine_val;
    K.overflows = B.overflows;
    K.cap = (uint32_t)B.cap;
    HIP_TRY(hipMemsetAsync(B.cand_n, 0, sizeof(uint32_t), s));
    // r = r' + stats[2]
    asx_launch_dc_remove(xi.tsrc, xi.tsmp, P.N, (double)P.F, B.stats, B.src_dc, s);
    K.shift = B.stats + 2;
    if (run_group(p, Pairs<TIn>::staged(B.src_dc, xi.smp, xi.tsrc, xi.tsmp, N, xi.win, xi.win_step), 1, yi, s,
                  { .prof_group = GroupOpts::no_marks, .listed = false, .f32_abi = false, .dot_blocks = 2048, .pk = &K, .topk = topk }))
        return -1;
    p->repaired++;
    return 0;
}

// Returns -1 on error, else the number of pairs that took the second look.  Waits for everything the caller has enqueued
// on `s` (its result copies included): ONE synchronisation; the count is read from the page-locked mirror k_finalize adds to
// only when a pair overflows -- no device-to-host copy sits between the last kernel and the host.
template <typename TIn>
static int resolve_overflows(asx_plan *p, const Pairs<TIn> &x, const Results &y, hipStream_t s, const Topk &topk = {})
{
    // An entry with ASX_QSTORE_REDO is a pair whose partially stored Q fell short (k_prune_select): it runs again as a group of
    // one with partial storing off -- k_rows_re and the pruned pass over the whole of Q, in slot 0 of lane 0, into its own results,
    // listed as usual.  Such a run may overflow its near-tie list like any other: when one ran, the list is looked at once more
    // (that second round can hold no such entry).  Nothing here costs a call without entries anything new.
    int total = 0;
    for (int round = 0; round < 2; round++) {
        HIP_TRY(hipStreamSynchronize(s));
        if (p->lanes[0].pk.cap >= 2 * p->host.N) return total; // the ordinary list already holds every lag
        const uint32_t n = *p->h_over_n;
        if (n == 0) return total;
        if (n > p->over_cap) {
            // cannot happen (a window is at most over_cap pairs); if it ever does, the list must not stay poisoned
            (void)hipMemsetAsync(p->over_n, 0, sizeof(uint32_t), s);
            (void)hipStreamSynchronize(s);
            *p->h_over_n = 0;
            return fail("internal: %u overflowed pairs in a window of %zu", n, p->over_cap);
        }
        p->h_over.resize(n);
        HIP_TRY(hipMemcpyAsync(p->h_over.data(), p->over_list, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemsetAsync(p->over_n, 0, sizeof(uint32_t), s));
        // pool calls: the listed pairs' rows {a, b} (a small copy of those rows only), so that each pair's second look runs on explicit
        // pointers -- as the strided call's does
        std::vector<int32_t> ab;
        if (x.pool) {
            ab.resize(2 * (size_t)n);
            for (uint32_t k = 0; k < n; k++) {
                const size_t pi = x.first + (p->h_over[k] & ~ASX_QSTORE_REDO);
                if (x.pool->rows)
                    HIP_TRY(hipMemcpyAsync(&ab[2 * k], x.pool->rows + 2 * pi, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                else { ab[2 * k] = (int32_t)(pi / x.pool->nsmp); ab[2 * k + 1] = (int32_t)(pi % x.pool->nsmp); }
            }
        }
        HIP_TRY(hipStreamSynchronize(s));
        *p->h_over_n = 0;
        const std::vector<uint32_t> list = p->h_over; // (a second run appends to the plan's list: keep this round's)
        uint32_t redone = 0;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t i = list[k] & ~ASX_QSTORE_REDO;
            Pairs<TIn> xi = x.at(i);
            if (list[k] & ASX_QSTORE_REDO) {
                if (run_group(p, xi, 1, y.at(i), s, { .prof_group = GroupOpts::no_marks, .pair_base = i, .topk = topk, .qstore = false }))
                    return -1;
                p->qstore_redone++;
                redone++;
                continue;
            }
            if (x.pool) {
                const int64_t a = ab[2 * k], b = ab[2 * k + 1];
                if (a < 0 || (size_t)a >= x.pool->nsrc || b < 0 || (size_t)b >= x.pool->nsmp) continue; // (k_rows_rl never lets one overflow)
                xi = xi.pool_pair((size_t)a, (size_t)b, p->host.N);
            }
            if (second_look(p, xi, y.at(i), s, topk)) return -1;
        }
        total += (int)n;
        if (!redone) return total;
    }
    return total;
}

// Copies the results of the g pairs of one group of a host-side entry point (device d, host h) back to the host.  The copies go
// out with the one synchronisation that reads the overflow list, and once more behind the second look if any pair took it.
template <typename TIn>
static int fetch_results(asx_plan *p, const Pairs<TIn> &x, size_t g, const Results &d, const Results &h, hipStream_t s)
{
    for (int pass = 0; pass < 2; pass++) {
        HIP_TRY(hipMemcpyAsync(h.lag, d.lag, g * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.coef, d.coef, g * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h.ret, d.ret, g * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (pass == 1) { HIP_TRY(hipStreamSynchronize(s)); break; }
        const int looked = resolve_overflows(p, x, d, s);
        if (looked < 0) return -1;
        if (looked == 0) break;
    }
    return 0;
}

// The forward column kernel runs 2-5 % faster or slower with the PHYSICAL placement of the buffers it streams together (the
// caller's inputs read, C_x / C_y written): strictly alternating with every re-allocation of either side, whatever the
// allocator, and untouched by offsets inside an allocation (EXPERIMENTS.md, round 4 items 27-28).  Nothing the library lays
// out can steer that -- but a plan made with split = "measure" (FFTW_MEASURE's role) may spend a few milliseconds once: at its
// first device-resident batch it allocates C_x / C_y a second time, times k_fwd_cols against the caller's buffers on both sets
// and keeps the faster.  The default planning mode never does this.
static int tune_placement(asx_plan *p, const float *d_src, const float *d_smp, size_t g, hipStream_t s)
{
    // (It allocates, synchronises and frees: never inside a stream capture -- a capturing caller keeps the first set, and the next
    // un-captured batch of >= min(group, 8) pairs tunes.)
    if (stream_capturing(s)) return 0;
    p->placement_done = true;
    const AsxDev &P = p->dev;
    asx_plan::Lane &W = p->lanes[0];
    const size_t mz = asx_spectrum_len(P) * p->group;
    // whatever leaves this function gives back the set that lost and the events (a failing HIP call used to leak them)
    AsxMemSet second(hip_mem);
    float2 *set[2][2] = { { W.zxa, W.zya }, { nullptr, nullptr } };
    if (second.take(&set[1][0], mz) || second.take(&set[1][1], mz)) return 0; // no room for a second set: keep what there is
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    const AsxPeakWs tk = asx_peak_unbanded(W.pk);
    for (int k = 0; k < 2; k++) {
        float best = 0.f;
        for (int r = 0; r < 4; r++) { // the first launch warms the set up; the fastest of the other three counts
            HIP_TRY(hipEventRecord(ev.e0, s));
            if (P.rlayout) asx_launch_fwd_cols_r(P, d_src, 2 * (size_t)P.N, d_smp, P.N, 0, (int)g, { set[k][0], set[k][1], tk.nrm_part, tk.band }, false, s);
            else asx_launch_fwd_cols(P, d_src, d_smp, set[k][0], set[k][1], tk, (int)g, s);
            HIP_TRY(hipEventRecord(ev.e1, s));
            HIP_TRY(hipEventSynchronize(ev.e1));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
            if (r >= 1 && (best == 0.f || ms < best)) best = ms;
        }
        p->placement_ms[k] = best;
    }
    const int keep = p->placement_ms[1] < 0.995 * p->placement_ms[0] ? 1 : 0;
    p->placement_kept = keep;
    if (keep == 1) p->cxy0.swap(second); // (two sets of one size: asx_plan_workspace_bytes does not change)
    W.zxa = set[keep][0];
    W.zya = set[keep][1];
    return 0;
}

extern "C" int asx_plan_placement(asx_plan *p, double ms[2], int *kept)
{
    if (!p || !ms || !kept) return fail("asx_plan_placement: null argument");
    std::lock_guard<std::mutex> guard(p->lock);
    ms[0] = p->placement_ms[0]; ms[1] = p->placement_ms[1];
    *kept = p->placement_kept;
    return 0;
}

// A device-resident batch of float32 pairs, after the entry point's own checks.  A PHAT batch (weight) lists nothing, so it never reads
// the overflow list: asynchronous whatever asx_plan_set_exact says.
static int run_batch(asx_plan *p, const Pairs<float> &x, size_t batch, const Results &y, hipStream_t s, const Topk &topk = {},
                     AsxWeight weight = ASX_W_NONE, const AsxBand &band = {}, const Near &near = {})
{
    prof_begin_call(p);
    const bool exact = p->exact && weight == ASX_W_NONE;
    // chunking: groups of at most `group` pairs; with two lanes a batch is cut into at least two
    // chunks (when it is big enough to fill the chip twice) that alternate between the lanes
    const bool overlap = (p->nlanes == 2) && !p->profiling && batch >= 8;
    size_t chunk = p->group;
    if (overlap && batch < 2 * chunk) chunk = (batch + 1) / 2;
    // windows: the pairs between two looks at the list of overflowed pairs (asx_plan_set_exact, on by default); a
    // window is a whole number of chunks and at most `over_cap` pairs, i.e. the whole batch unless it is very long
    const size_t window = exact ? std::max<size_t>(chunk, p->over_cap / chunk * chunk) : batch;
    size_t gi = 0;
    for (size_t w0 = 0; w0 < batch; w0 += window) {
        const size_t wn = std::min(window, batch - w0);
        if (overlap) {
            HIP_TRY(hipEventRecord(p->fork, s));
            for (int l = 0; l < 2; l++) HIP_TRY(hipStreamWaitEvent(p->lanes[l].stream, p->fork, 0));
        }
        for (size_t done = w0; done < w0 + wn; done += chunk, gi++) {
            const size_t g = std::min(chunk, w0 + wn - done);
            const int lane = overlap ? (int)(gi & 1) : 0;
            hipStream_t ls = overlap ? p->lanes[lane].stream : s;
            if (run_group(p, x.at(done), g, y.at(done), ls,
                          { .prof_group = gi, .lane = lane, .pair_base = (uint32_t)(done - w0), .listed = exact, .topk = topk,
                            .weight = weight, .fband = band, .near = near.at(done) }))
                return -1;
        }
        if (overlap) {
            for (int l = 0; l < 2; l++) {
                HIP_TRY(hipEventRecord(p->lanes[l].done, p->lanes[l].stream));
                HIP_TRY(hipStreamWaitEvent(s, p->lanes[l].done, 0));
            }
        }
        // the second look, behind the window's last group (one host synchronisation per window)
        if (exact && resolve_overflows(p, x.at(w0), y.at(w0), s, topk) < 0) return -1;
    }
    prof_end_call(p, gi);
    return 0;
}

extern "C" int asx_xcorr_batch_f32_dev(asx_plan *p, const float *d_source, const float *d_sample,
                                       size_t batch, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                                       void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef) return fail("asx_xcorr_batch_f32_dev: null argument");
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    const size_t N = p->host.N;
    if (p->tune_placement && !p->placement_done && batch >= std::min<size_t>(p->group, 8) && // (lane 0's workspaces; a second lane keeps its own)
        tune_placement(p, d_source, d_sample, std::min(batch, p->group), c.s))
        return -1;
    return run_batch(p, Pairs<float>::contiguous(d_source, d_sample, N), batch, { d_lag, d_coef, d_ret }, c.s);
}

// ---------------------------------------------------------------------------
// strided batches: one track against many (asx_xcorr_strided_f32_dev)
// ---------------------------------------------------------------------------
// asx_xcorr_strided_f32_dev and asx_xcorr_windowed_f32_dev (fn: the entry point's name for the messages), after their own null checks.
// d_windows: null, or the per-pair windows (Pairs::win), window_stride rows apart.
// The layout rule of a strided call's inputs: 0, or -1 with the message.
static int strided_layout(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample,
                          size_t sample_stride)
{
    const AsxDev &P = p->dev;
    if (P.rlayout) {
        // k_fwd_cols_r reads every row of a pair's inputs as 16-byte loads from the pair's first frame
        if (((uintptr_t)d_source & 15u) || ((uintptr_t)d_sample & 15u))
            return fail("%s: real-column plans need 16-byte aligned inputs (source %p, sample %p)",
                        fn, (const void *)d_source, (const void *)d_sample);
        if ((source_stride & 3u) || (sample_stride & 3u))
            return fail("%s: real-column plans need strides that are multiples of 4 floats "
                        "(source_stride %zu, sample_stride %zu)", fn, source_stride, sample_stride);
    }
    return 0;
}

// The call's broadcast operands (bit 0: the source, bit 1: the sample; real-column plans): the slot, allocated at the first such call,
// and the shared track's forward column pass into it.  -> bc through *out; -1 with the message.
static int strided_broadcast(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample,
                             size_t sample_stride, hipStream_t s, int *out)
{
    const AsxDev &P = p->dev;
    const int bc = P.rlayout ? (source_stride == 0 ? 1 : 0) | (sample_stride == 0 ? 2 : 0) : 0;
    if (bc) {
        AsxSpectra &B = p->bslot;
        if (!B.cx) {
            if (stream_capturing(s))
                return fail("%s: the plan's broadcast workspace does not exist yet and cannot be allocated "
                            "during a stream capture; make one call with a stride of 0 outside the capture first", fn);
            if (asx_mem_whole(p->mem, B, [&](AsxMemSet &m, AsxSpectra &T) { return take_spectra(P, m, T, 1, 1); }))
                return fail("hipMalloc(&ptr, bytes) failed: %s (%s:%d)", hipGetErrorString(g_take_err), __FILE__, __LINE__);
        }
        // the shared track's forward column pass: once per call, on the caller's stream, before any lane forks
        asx_launch_fwd_cols_r(P, (bc & 1) ? d_source : nullptr, 0, (bc & 2) ? d_sample : nullptr, 0, 0, 1, B, true, s);
    }
    *out = bc;
    return 0;
}

static int strided_batch(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample,
                         size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch, const Results &y, void *stream,
                         const Topk &topk = {}, AsxWeight weight = ASX_W_NONE, const AsxBand &band = {}, const Near &near = {})
{
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    if (weight != ASX_W_NONE && p->dev.rlayout != 1) return fail("%s: PHAT calls need a real-column plan (asx_plan_layout() == 1)", fn);
    if (strided_layout(p, fn, d_source, source_stride, d_sample, sample_stride)) return -1;
    if (batch == 0) return 0;
    int bc = 0;
    if (strided_broadcast(p, fn, d_source, source_stride, d_sample, sample_stride, s, &bc)) return -1;
    return run_batch(p, Pairs<float>::strided(d_source, source_stride, d_sample, sample_stride, bc, d_windows, window_stride), batch, y, s,
                     topk, weight, band, near);
}

extern "C" int asx_xcorr_strided_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                         size_t sample_stride, size_t batch, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                                         void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef) return fail("asx_xcorr_strided_f32_dev: null argument");
    return strided_batch(p, "asx_xcorr_strided_f32_dev", d_source, source_stride, d_sample, sample_stride, nullptr, 0, batch,
                         { d_lag, d_coef, d_ret }, stream);
}

// Per-pair lag windows: the strided batch with each pair's row read on the device (run_group's per-pair kernels).  The plan's own
// window is neither used nor changed.
extern "C" int asx_xcorr_windowed_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                          size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                          int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream)
{
    if (!p || !d_source || !d_sample || !d_windows || !d_coef || !d_ret) return fail("asx_xcorr_windowed_f32_dev: null argument");
    return strided_batch(p, "asx_xcorr_windowed_f32_dev", d_source, source_stride, d_sample, sample_stride, d_windows, window_stride,
                         batch, { d_lag, d_coef, d_ret }, stream);
}

// GCC-PHAT: the strided / windowed batch with the whitened product spectrum (run_group: GroupOpts::weight).  The peak is the float32
// argmax of r_phat under the library's rule, the coefficient the reference's at that lag in the direct form, peak its height.
extern "C" int asx_xcorr_phat_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                      size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                      int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef || !d_ret) return fail("asx_xcorr_phat_f32_dev: null argument");
    return strided_batch(p, "asx_xcorr_phat_f32_dev", d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                         { d_lag, d_coef, d_ret, 1, d_peak }, stream, {}, ASX_W_PHAT);
}

// The weighting of a banded PHAT call: bins [bin_lo, bin_hi] of the F = 2N point transform, 0 <= bin_lo <= bin_hi <= N.  The full band
// is plain PHAT -- the kernels and the bits of asx_xcorr_phat_f32_dev, as the full lag window is no window.  false: not a band.
static bool band_weight(const asx_plan *p, int64_t bin_lo, int64_t bin_hi, AsxWeight &weight, AsxBand &band)
{
    const int64_t N = (int64_t)p->host.N;
    if (bin_lo < 0 || bin_lo > bin_hi || bin_hi > N) return false;
    const bool full = bin_lo == 0 && bin_hi == N;
    weight = full ? ASX_W_PHAT : ASX_W_PHAT_BAND;
    band = full ? AsxBand{} : AsxBand{ (uint32_t)bin_lo, (uint32_t)(bin_hi - bin_lo) };
    return true;
}

// GCC-PHAT in which only the bins of a band vote: asx_xcorr_phat_f32_dev with the banded row pass and the peak height per voter.
extern "C" int asx_xcorr_phat_band_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                           size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                           int64_t bin_lo, int64_t bin_hi, int64_t *d_lag, double *d_coef, double *d_peak,
                                           int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_phat_band_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_ret) return fail("%s: null argument", fn);
    AsxWeight weight;
    AsxBand band;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    return strided_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                         { d_lag, d_coef, d_ret, 1, d_peak }, stream, {}, weight, band);
}

// What the sub-sample PHAT calls add to their arguments: 1 <= half_width <= ASX_NEAR_MAX, d_frac not null (d_near may be), and a row
// long enough to hold the neighbourhood (every real-column plan's is; a packed plan is refused by the PHAT rule behind this).
static bool near_option(const asx_plan *p, const char *fn, int half_width, double *d_frac, double *d_near, Near &near)
{
    if (half_width < 1 || half_width > ASX_NEAR_MAX) { fail("%s: half_width = %d is not in [1, %d]", fn, half_width, ASX_NEAR_MAX); return false; }
    if (!d_frac) { fail("%s: null argument (d_frac)", fn); return false; }
    if (p->dev.rlayout == 1 && 2 * half_width + 1 > p->dev.M2) {
        fail("%s: half_width = %d needs rows of at least %d columns, the plan's have %d", fn, half_width, 2 * half_width + 1, p->dev.M2);
        return false;
    }
    near = Near{ d_frac, d_near, half_width };
    return true;
}

// Sub-sample GCC-PHAT: asx_xcorr_phat_band_f32_dev, and behind each group's tail k_phat_near, which reads r_phat around the peak from
// the group's Q' and writes d_near and d_frac.  The four other results are the banded call's: the same launches in front of it.
extern "C" int asx_xcorr_phat_sub_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                          size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                          int64_t bin_lo, int64_t bin_hi, int half_width, int64_t *d_lag, double *d_coef, double *d_peak,
                                          double *d_frac, double *d_near, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_phat_sub_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_ret) return fail("%s: null argument", fn);
    AsxWeight weight;
    AsxBand band;
    Near near;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    if (!near_option(p, fn, half_width, d_frac, d_near, near)) return -1;
    return strided_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                         { d_lag, d_coef, d_ret, 1, d_peak }, stream, {}, weight, band, near);
}

// one contiguous pair through a PHAT group (weight, band), r_phat of every lag (2N floats, unnormalised) to d_r; the plan's window
static int phat_debug_r(asx_plan *p, const char *fn, const float *d_source, const float *d_sample, float *d_r, const Results &y,
                        void *stream, AsxWeight weight, const AsxBand &band)
{
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    if (p->dev.rlayout != 1) return fail("%s: PHAT calls need a real-column plan (asx_plan_layout() == 1)", fn);
    if (((uintptr_t)d_source & 15u) || ((uintptr_t)d_sample & 15u))
        return fail("%s: real-column plans need 16-byte aligned inputs (source %p, sample %p)", fn, (const void *)d_source,
                    (const void *)d_sample);
    prof_begin_call(p);
    const size_t N = p->host.N;
    const int rc = run_group(p, Pairs<float>::contiguous(d_source, d_sample, N), 1, y, c.s,
                             { .listed = false, .f32_abi = false, .r_out = d_r, .weight = weight, .fband = band });
    prof_end_call(p, 1);
    return rc;
}

extern "C" int asx_xcorr_phat_debug_r_dev(asx_plan *p, const float *d_source, const float *d_sample, float *d_r, int64_t *d_lag,
                                          double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_phat_debug_r_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_ret || !d_r) return fail("%s: null argument", fn);
    return phat_debug_r(p, fn, d_source, d_sample, d_r, { d_lag, d_coef, d_ret, 1, d_peak }, stream, ASX_W_PHAT, {});
}

// the same for the banded call: d_r holds votes times what peak reports
extern "C" int asx_xcorr_phat_band_debug_r_dev(asx_plan *p, const float *d_source, const float *d_sample, int64_t bin_lo,
                                               int64_t bin_hi, float *d_r, int64_t *d_lag, double *d_coef, double *d_peak,
                                               int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_phat_band_debug_r_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_ret || !d_r) return fail("%s: null argument", fn);
    AsxWeight weight;
    AsxBand band;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    return phat_debug_r(p, fn, d_source, d_sample, d_r, { d_lag, d_coef, d_ret, 1, d_peak }, stream, weight, band);
}

// The bins of a frequency band, for the banded call: bin m of the F = 2N point transform is m * rate / (2N) Hz.  Host arithmetic only.
extern "C" int asx_band_bins(size_t sample_len, double sample_rate, double f_lo_hz, double f_hi_hz, int64_t *bin_lo, int64_t *bin_hi)
{
    // (every comparison with a NaN is false: written so that a NaN fails)
    if (!bin_lo || !bin_hi || sample_len == 0 || !(sample_rate > 0.0) || !(f_lo_hz >= 0.0) || !(f_lo_hz <= f_hi_hz)) return -1;
    const double n = (double)sample_len, per_hz = 2.0 * n / sample_rate;
    const double lo = std::ceil(f_lo_hz * per_hz), hi = std::min(n, std::floor(f_hi_hz * per_hz));
    if (!(lo <= hi)) return -1; // no bin inside (or an infinite rate or frequency made a NaN)
    *bin_lo = (int64_t)lo;
    *bin_hi = (int64_t)hi;
    return 0;
}

// The K strongest separated lags per pair: the strided / windowed batch with passes 2..k over each group's Q (run_group).  k = 1
// launches exactly what that call launches.
extern "C" int asx_xcorr_topk_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                      size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch, int k,
                                      int64_t min_separation, int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef || !d_ret) return fail("asx_xcorr_topk_f32_dev: null argument");
    if (k < 1 || k > ASX_TOPK_MAX) return fail("asx_xcorr_topk_f32_dev: k = %d is not in [1, %d]", k, ASX_TOPK_MAX);
    if (min_separation < 0) return fail("asx_xcorr_topk_f32_dev: min_separation = %lld is negative", (long long)min_separation);
    return strided_batch(p, "asx_xcorr_topk_f32_dev", d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                         { d_lag, d_coef, d_ret, (size_t)k }, stream, Topk{ k, min_separation });
}

// The K strongest separated lags per pair by the GCC-PHAT curve: the banded PHAT call with passes 2..k over each group's resident Q'
// (run_group).  k = 1 launches exactly asx_xcorr_phat_band_f32_dev.
extern "C" int asx_xcorr_phat_topk_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                           size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                           int64_t bin_lo, int64_t bin_hi, int k, int64_t min_separation, int64_t *d_lag, double *d_coef,
                                           double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_phat_topk_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_ret) return fail("%s: null argument", fn);
    if (k < 1 || k > ASX_TOPK_MAX) return fail("%s: k = %d is not in [1, %d]", fn, k, ASX_TOPK_MAX);
    if (min_separation < 0) return fail("%s: min_separation = %lld is negative", fn, (long long)min_separation);
    AsxWeight weight;
    AsxBand band;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    return strided_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                         { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, Topk{ k, min_separation }, weight, band);
}

// ---------------------------------------------------------------------------
// pool calls: listed pairs of two track pools (asx_xcorr_pool_f32_dev)
// ---------------------------------------------------------------------------
// The bank holds at least nsrc source and nsmp sample tracks.  Grown (everything reallocated, behind a device synchronisation: earlier
// calls may still read the old one) when a call names more; never inside a stream capture.
static int ensure_bank(asx_plan *p, const char *fn, size_t nsrc, size_t nsmp, hipStream_t s)
{
    asx_plan::Bank &B = p->bank;
    if (nsrc <= B.nsrc && nsmp <= B.nsmp) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's bank holds %zu x %zu tracks and cannot grow to %zu x %zu during a stream capture; make a call "
                    "with pools at least this large outside the capture first", fn, B.nsrc, B.nsmp, nsrc, nsmp);
    const AsxDev &P = p->dev;
    const size_t ns = std::max(nsrc, B.nsrc), nm = std::max(nsmp, B.nsmp);
    // the old bank goes before the new one comes: both at once would double the peak
    HIP_TRY(hipDeviceSynchronize());
    B.mem.clear(); B.c = AsxSpectra{}; B.nsrc = B.nsmp = 0;
    if (asx_mem_whole(B.mem, B.c, [&](AsxMemSet &m, AsxSpectra &T) { return take_spectra(P, m, T, ns, nm); }))
        return fail("%s: cannot allocate the plan's bank for %zu source and %zu sample tracks (%zu bytes per track)", fn, ns, nm,
                    asx_spectrum_len(P) * sizeof(float2));
    B.nsrc = ns; B.nsmp = nm;
    return 0;
}

// What every pool call checks of its pools and pairs behind its null checks; 0, or -1 with the message
static int pool_layout(asx_plan *p, const char *fn, const float *d_sources, size_t source_stride, size_t nsources, const float *d_samples,
                       size_t sample_stride, size_t nsamples, const int32_t *d_pairs, size_t batch)
{
    const AsxDev &P = p->dev;
    if (P.rlayout != 1) return fail("%s: pool calls need a real-column plan (asx_plan_layout() == 1)", fn);
    if (((uintptr_t)d_sources & 15u) || ((uintptr_t)d_samples & 15u))
        return fail("%s: the pools must be 16-byte aligned (sources %p, samples %p)", fn, (const void *)d_sources, (const void *)d_samples);
    if ((source_stride & 3u) || (sample_stride & 3u))
        return fail("%s: strides must be multiples of 4 floats (source_stride %zu, sample_stride %zu)", fn, source_stride, sample_stride);
    if (nsources > INT32_MAX || nsamples > INT32_MAX) return fail("%s: a pool of more than 2^31 - 1 tracks", fn);
    if (!d_pairs && batch != nsources * nsamples)
        return fail("%s: without pairs the batch is every combination, %zu x %zu, not %zu", fn, nsources, nsamples, batch);
    if (batch != 0 && (nsources == 0 || nsamples == 0))
        return fail("%s: an empty pool (%zu sources, %zu samples) for %zu pairs", fn, nsources, nsamples, batch);
    return 0;
}

// the bank fill: every track's forward column pass, once per call, on the caller's stream before any lane forks (grid.z: at most
// 65535 tracks per launch)
static void pool_fill(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources, const float *d_samples,
                      size_t sample_stride, size_t nsamples, hipStream_t s)
{
    const AsxDev &P = p->dev;
    for (int op = 0; op < 2; op++) {
        const size_t n = op ? nsamples : nsources;
        for (size_t c0 = 0; c0 < n; c0 += 65535)
            asx_launch_fwd_cols_r(P, op ? nullptr : d_sources, source_stride, op ? d_samples : nullptr, sample_stride, c0,
                                  (int)std::min<size_t>(65535, n - c0), p->bank.c, true, s);
    }
    p->bank.fills++;
}

// asx_xcorr_pool_f32_dev, asx_xcorr_pool_topk_f32_dev and asx_xcorr_pool_phat_f32_dev (fn: the entry point's name for the messages; y
// and topk: the top-k call's entry stride and option, after its own checks of k and min_separation; weight and band: the PHAT call's,
// after band_weight)
static int pool_batch(asx_plan *p, const char *fn, const float *d_sources, size_t source_stride, size_t nsources, const float *d_samples,
                      size_t sample_stride, size_t nsamples, const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride,
                      size_t batch, const Results &y, void *stream, const Topk &topk = {}, AsxWeight weight = ASX_W_NONE,
                      const AsxBand &band = {}, const Near &near = {})
{
    if (!p || !d_sources || !d_samples || !y.coef || !y.ret) return fail("%s: null argument", fn);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    if (pool_layout(p, fn, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, batch)) return -1;
    if (batch == 0) return 0;
    if (ensure_bank(p, fn, nsources, nsamples, s)) return -1;
    pool_fill(p, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, s);
    const PoolCall pool{ d_pairs, nsources, nsamples };
    return run_batch(p, Pairs<float>::pooled(&pool, d_sources, source_stride, d_samples, sample_stride, d_windows, window_stride), batch, y,
                     s, topk, weight, band, near);
}

extern "C" int asx_xcorr_pool_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                      const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                      const int64_t *d_windows, size_t window_stride, size_t batch, int64_t *d_lag, double *d_coef,
                                      int32_t *d_ret, void *stream)
{
    return pool_batch(p, "asx_xcorr_pool_f32_dev", d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs,
                      d_windows, window_stride, batch, { d_lag, d_coef, d_ret }, stream);
}

// The K strongest separated lags per pair of two pools: the pool call with passes 2..k over each group's Q (run_group); the bank is
// filled once per call whatever k is.  k = 1 launches exactly the pool call.
extern "C" int asx_xcorr_pool_topk_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                           const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                           const int64_t *d_windows, size_t window_stride, size_t batch, int k, int64_t min_separation,
                                           int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_topk_f32_dev";
    if (k < 1 || k > ASX_TOPK_MAX) return fail("%s: k = %d is not in [1, %d]", fn, k, ASX_TOPK_MAX);
    if (min_separation < 0) return fail("%s: min_separation = %lld is negative", fn, (long long)min_separation);
    return pool_batch(p, fn, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows, window_stride,
                      batch, { d_lag, d_coef, d_ret, (size_t)k }, stream, Topk{ k, min_separation });
}

// GCC-PHAT over two pools: the pool call's pairs through PHAT groups (run_group: GroupOpts::weight with a pool), the bank filled once per
// call.  The band is always given; the full band is plain PHAT (band_weight).
extern "C" int asx_xcorr_pool_phat_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                           const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                           const int64_t *d_windows, size_t window_stride, size_t batch, int64_t bin_lo, int64_t bin_hi,
                                           int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_phat_f32_dev";
    if (!p) return fail("%s: null argument", fn);
    AsxWeight weight;
    AsxBand band;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    return pool_batch(p, fn, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows, window_stride,
                      batch, { d_lag, d_coef, d_ret, 1, d_peak }, stream, {}, weight, band);
}

// The K strongest separated lags per pair of two pools by the GCC-PHAT curve: the pool PHAT call with passes 2..k over each group's
// resident Q' (run_group); the bank is filled once per call whatever k is.  k = 1 launches exactly asx_xcorr_pool_phat_f32_dev.
extern "C" int asx_xcorr_pool_phat_topk_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                                const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                                const int64_t *d_windows, size_t window_stride, size_t batch, int64_t bin_lo,
                                                int64_t bin_hi, int k, int64_t min_separation, int64_t *d_lag, double *d_coef,
                                                double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_phat_topk_f32_dev";
    if (!p) return fail("%s: null argument", fn);
    if (k < 1 || k > ASX_TOPK_MAX) return fail("%s: k = %d is not in [1, %d]", fn, k, ASX_TOPK_MAX);
    if (min_separation < 0) return fail("%s: min_separation = %lld is negative", fn, (long long)min_separation);
    AsxWeight weight;
    AsxBand band;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    return pool_batch(p, fn, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows, window_stride,
                      batch, { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, Topk{ k, min_separation }, weight, band);
}

// ... with the peak's neighbourhood: asx_xcorr_phat_sub_f32_dev's two outputs for the pool call's pairs
extern "C" int asx_xcorr_pool_phat_sub_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                               const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                               const int64_t *d_windows, size_t window_stride, size_t batch, int64_t bin_lo,
                                               int64_t bin_hi, int half_width, int64_t *d_lag, double *d_coef, double *d_peak,
                                               double *d_frac, double *d_near, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_phat_sub_f32_dev";
    if (!p) return fail("%s: null argument", fn);
    AsxWeight weight;
    AsxBand band;
    Near near;
    if (!band_weight(p, bin_lo, bin_hi, weight, band))
        return fail("%s: bins [%lld, %lld] are not a band inside [0, %zu]", fn, (long long)bin_lo, (long long)bin_hi, (size_t)p->host.N);
    if (!near_option(p, fn, half_width, d_frac, d_near, near)) return -1;
    return pool_batch(p, fn, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows, window_stride,
                      batch, { d_lag, d_coef, d_ret, 1, d_peak }, stream, {}, weight, band, near);
}

// ---------------------------------------------------------------------------
// the curve around given lags (asx_xcorr_curve_f32_dev, asx_xcorr_pool_curve_f32_dev): a consumer behind any call, on the lags it
// returned.  No transform, no group: r and frac from k_curve_dots over the tracks themselves, the coefficient curve from the direct
// Pearson kernels over one virtual pair per neighbour; both in slices of a launch group, in lane 0's records and psums.
// ---------------------------------------------------------------------------
// What the curve, track and warp calls share.  Before PlanCall, behind the caller's null check: the ranges of entries and of
// half_width, at most hmax (fn: the entry point's name for the messages).  0, or -1 with the message set.
static int entries_ranges(const char *fn, int entries, int half_width, int hmax)
{
    if (entries < 1 || entries > ASX_TOPK_MAX) return fail("%s: entries = %d is not in [1, %d]", fn, entries, ASX_TOPK_MAX);
    if (half_width < 1 || half_width > hmax) return fail("%s: half_width = %d is not in [1, %d]", fn, half_width, hmax);
    return 0;
}
// Behind PlanCall: the plan's layout against the inputs and the pools (pooled: nsrc, nsmp and d_pairs mean something), then E, the
// call's entries as the kernels take them.  1: go on; 0: nothing to do; -1 with the message set.
static int entries_of_call(const asx_plan *p, const char *fn, bool pooled, const float *d_src, size_t src_stride, size_t nsrc,
                           const float *d_smp, size_t smp_stride, size_t nsmp, const int32_t *d_pairs, size_t batch, int entries,
                           const int64_t *d_center, int half_width, AsxLagEntries &E)
{
    const AsxDev &P = p->dev;
    if (pooled && P.rlayout != 1) return fail("%s: pool calls need a real-column plan (asx_plan_layout() == 1)", fn);
    if (P.rlayout) {
        if (((uintptr_t)d_src & 15u) || ((uintptr_t)d_smp & 15u))
            return fail("%s: real-column plans need 16-byte aligned inputs (source %p, sample %p)", fn, (const void *)d_src,
                        (const void *)d_smp);
        if ((src_stride & 3u) || (smp_stride & 3u))
            return fail("%s: real-column plans need strides that are multiples of 4 floats (source_stride %zu, sample_stride %zu)", fn,
                        src_stride, smp_stride);
    }
    if (pooled) {
        if (nsrc > INT32_MAX || nsmp > INT32_MAX) return fail("%s: a pool of more than 2^31 - 1 tracks", fn);
        if (!d_pairs && batch != nsrc * nsmp)
            return fail("%s: without pairs the batch is every combination, %zu x %zu, not %zu", fn, nsrc, nsmp, batch);
    }
    if (batch == 0) return 0;
    if (pooled && (nsrc == 0 || nsmp == 0)) return fail("%s: an empty pool (%zu sources, %zu samples) for %zu pairs", fn, nsrc, nsmp, batch);
    E = AsxLagEntries{ d_center, P.N, entries, half_width, pooled ? d_pairs : nullptr, pooled ? (uint64_t)nsrc : 0u,
                       pooled ? (uint64_t)nsmp : 0u, (uint64_t)src_stride, (uint64_t)smp_stride };
    return 1;
}
// go(first, count) over [0, total) in slices of a launch group
template <class F> static void group_slices(const asx_plan *p, size_t total, F go)
{
    for (size_t e0 = 0; e0 < total; e0 += p->group) go(e0, (int)std::min(p->group, total - e0));
}

// both entry points
static int curve_call(asx_plan *p, const char *fn, bool pooled, const float *d_src, size_t src_stride, size_t nsrc, const float *d_smp,
                      size_t smp_stride, size_t nsmp, const int32_t *d_pairs, size_t batch, int entries, const int64_t *d_center,
                      int half_width, double *d_r, double *d_coef, double *d_frac, int32_t *d_ret, void *stream)
{
    if (!p || !d_src || !d_smp || !d_center || !d_r || !d_frac || !d_ret) return fail("%s: null argument", fn);
    if (entries_ranges(fn, entries, half_width, ASX_NEAR_MAX)) return -1;
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    AsxCurve A{ {}, d_r, d_frac, d_ret };
    const int go = entries_of_call(p, fn, pooled, d_src, src_stride, nsrc, d_smp, smp_stride, nsmp, d_pairs, batch, entries, d_center,
                                   half_width, A.E);
    if (go <= 0) return go;
    asx_plan::Lane &W = p->lanes[0];
    const size_t total = batch * (size_t)entries, n = 2 * (size_t)half_width + 1;
    group_slices(p, total, [&](size_t e0, int g) { asx_launch_curve_r(d_src, d_smp, A, e0, g, W.pool, W.psums, s); });
    if (d_coef) {
        // one direct Pearson pass per neighbour: the kernels, the chunks and the merge tree of a windowed call with the row [l, l]
        const AsxInputs<float> in{ d_src, d_smp, 0, 0, W.pool };
        group_slices(p, total * n, [&](size_t v0, int g) {
            asx_launch_curve_segs(A.E, v0, g, W.seg, W.pool, s);
            asx_launch_pearson(in, p->dev.N, W.seg, W.psums, (int64_t *)nullptr, d_coef + v0, (int32_t *)nullptr, g, s);
        });
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int asx_xcorr_curve_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                       size_t sample_stride, size_t batch, int entries, const int64_t *d_center, int half_width,
                                       double *d_r, double *d_coef, double *d_frac, int32_t *d_ret, void *stream)
{
    return curve_call(p, "asx_xcorr_curve_f32_dev", false, d_source, source_stride, 0, d_sample, sample_stride, 0, nullptr, batch,
                      entries, d_center, half_width, d_r, d_coef, d_frac, d_ret, stream);
}

extern "C" int asx_xcorr_pool_curve_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                            const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                            size_t batch, int entries, const int64_t *d_center, int half_width, double *d_r,
                                            double *d_coef, double *d_frac, int32_t *d_ret, void *stream)
{
    return curve_call(p, "asx_xcorr_pool_curve_f32_dev", true, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples,
                      d_pairs, batch, entries, d_center, half_width, d_r, d_coef, d_frac, d_ret, stream);
}

// ---------------------------------------------------------------------------
// the lag track (asx_xcorr_track_f32_dev, asx_xcorr_pool_track_f32_dev): the curve's sibling -- r per time segment over a wide lag
// range, each segment's peak and the drift line through the peaks.  No transform, no group: k_track_dots over the tracks themselves
// and k_track_fit behind it, in slices of a launch group, in lane 0's records and psums.
// ---------------------------------------------------------------------------
static int track_call(asx_plan *p, const char *fn, bool pooled, const float *d_src, size_t src_stride, size_t nsrc, const float *d_smp,
                      size_t smp_stride, size_t nsmp, const int32_t *d_pairs, size_t batch, int entries, const int64_t *d_center,
                      int half_width, int segments, double *d_r, double *d_seg, double *d_fit, int32_t *d_used, int32_t *d_ret,
                      void *stream)
{
    if (!p || !d_src || !d_smp || !d_center || !d_r || !d_fit || !d_used || !d_ret) return fail("%s: null argument", fn);
    if (entries_ranges(fn, entries, half_width, ASX_TRACK_HALF_MAX)) return -1;
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    if (segments < 1 || segments > ASX_TRACK_SEG_MAX || (uint64_t)segments > (uint64_t)p->dev.N)
        return fail("%s: segments = %d is not in [1, min(%d, N = %u)]", fn, segments, ASX_TRACK_SEG_MAX, (unsigned)p->dev.N);
    AsxTrack A{ {}, segments, d_r, d_seg, d_fit, d_used, d_ret };
    const int go = entries_of_call(p, fn, pooled, d_src, src_stride, nsrc, d_smp, smp_stride, nsmp, d_pairs, batch, entries, d_center,
                                   half_width, A.E);
    if (go <= 0) return go;
    asx_plan::Lane &W = p->lanes[0];
    group_slices(p, batch * (size_t)entries, [&](size_t e0, int g) { asx_launch_track(d_src, d_smp, A, e0, g, W.pool, W.psums, s); });
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int asx_xcorr_track_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                       size_t sample_stride, size_t batch, int entries, const int64_t *d_center, int half_width,
                                       int segments, double *d_r, double *d_seg, double *d_fit, int32_t *d_used, int32_t *d_ret,
                                       void *stream)
{
    return track_call(p, "asx_xcorr_track_f32_dev", false, d_source, source_stride, 0, d_sample, sample_stride, 0, nullptr, batch,
                      entries, d_center, half_width, segments, d_r, d_seg, d_fit, d_used, d_ret, stream);
}

extern "C" int asx_xcorr_pool_track_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                            const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                            size_t batch, int entries, const int64_t *d_center, int half_width, int segments,
                                            double *d_r, double *d_seg, double *d_fit, int32_t *d_used, int32_t *d_ret, void *stream)
{
    return track_call(p, "asx_xcorr_pool_track_f32_dev", true, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples,
                      d_pairs, batch, entries, d_center, half_width, segments, d_r, d_seg, d_fit, d_used, d_ret, stream);
}

// ---------------------------------------------------------------------------
// the warped correlation (asx_xcorr_warp_f32_dev, asx_xcorr_pool_warp_f32_dev): the curve's r, its frac and one Pearson coefficient
// along a drift line per entry, what the track call's fit feeds.  No transform, no group: k_warp_dots over the tracks themselves and
// k_warp_final behind it, in slices of a launch group, in lane 0's records and psums.
// ---------------------------------------------------------------------------
static int warp_call(asx_plan *p, const char *fn, bool pooled, const float *d_src, size_t src_stride, size_t nsrc, const float *d_smp,
                     size_t smp_stride, size_t nsmp, const int32_t *d_pairs, size_t batch, int entries, const int64_t *d_center,
                     const double *d_line, size_t line_stride, int half_width, double *d_r, double *d_frac, double *d_coef,
                     int64_t *d_len, int32_t *d_ret, void *stream)
{
    if (!p || !d_src || !d_smp || !d_center || !d_line || !d_r || !d_frac || !d_coef || !d_ret) return fail("%s: null argument", fn);
    if (entries_ranges(fn, entries, half_width, ASX_NEAR_MAX)) return -1;
    if (line_stride == 1) return fail("%s: line_stride = 1: a line is two doubles (0: one line for every entry)", fn);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    AsxWarp A{ {}, d_line, (uint64_t)line_stride, d_r, d_frac, d_coef, d_len, d_ret };
    const int go = entries_of_call(p, fn, pooled, d_src, src_stride, nsrc, d_smp, smp_stride, nsmp, d_pairs, batch, entries, d_center,
                                   half_width, A.E);
    if (go <= 0) return go;
    asx_plan::Lane &W = p->lanes[0];
    group_slices(p, batch * (size_t)entries, [&](size_t e0, int g) { asx_launch_warp(d_src, d_smp, A, e0, g, W.pool, W.psums, s); });
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int asx_xcorr_warp_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                      size_t sample_stride, size_t batch, int entries, const int64_t *d_center, const double *d_line,
                                      size_t line_stride, int half_width, double *d_r, double *d_frac, double *d_coef, int64_t *d_len,
                                      int32_t *d_ret, void *stream)
{
    return warp_call(p, "asx_xcorr_warp_f32_dev", false, d_source, source_stride, 0, d_sample, sample_stride, 0, nullptr, batch, entries,
                     d_center, d_line, line_stride, half_width, d_r, d_frac, d_coef, d_len, d_ret, stream);
}

extern "C" int asx_xcorr_pool_warp_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                           const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                           size_t batch, int entries, const int64_t *d_center, const double *d_line, size_t line_stride,
                                           int half_width, double *d_r, double *d_frac, double *d_coef, int64_t *d_len, int32_t *d_ret,
                                           void *stream)
{
    return warp_call(p, "asx_xcorr_pool_warp_f32_dev", true, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples,
                     d_pairs, batch, entries, d_center, d_line, line_stride, half_width, d_r, d_frac, d_coef, d_len, d_ret, stream);
}

// diagnostic (not in the public header): the bank's capacity in tracks and how many pool calls have filled it
extern "C" int asx_plan_debug_bank(asx_plan *p, uint64_t *nsrc, uint64_t *nsmp, uint64_t *fills)
{
    if (!p || !nsrc || !nsmp || !fills) return -1;
    std::lock_guard<std::mutex> guard(p->lock);
    *nsrc = p->bank.nsrc;
    *nsmp = p->bank.nsmp;
    *fills = p->bank.fills;
    return 0;
}

extern "C" int asx_xcorr_debug_r_dev(asx_plan *p, const float *d_source, const float *d_sample,
                                     float *d_r, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                                     void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef || !d_r) return fail("asx_xcorr_debug_r_dev: null argument");
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    prof_begin_call(p);
    // like every other entry point: listed and looked at again in the exact mode, only marked (ret = 1) otherwise
    // (the direct Pearson form: this entry point exists to compare decompositions and to dump r)
    const size_t N = p->host.N;
    const Pairs<float> x = Pairs<float>::contiguous(d_source, d_sample, N);
    const Results y{ d_lag, d_coef, d_ret };
    int rc = run_group(p, x, 1, y, c.s, { .listed = p->exact, .f32_abi = false, .r_out = d_r });
    prof_end_call(p, 1);
    if (rc == 0 && p->exact && resolve_overflows(p, x, y, c.s) < 0) rc = -1;
    return rc;
}

// ---------------------------------------------------------------------------
// normalised cross-correlation (asx_xcorr_ncc_f32_dev): a consumer behind ordinary launch groups
// ---------------------------------------------------------------------------
#define ASX_NCC_WS_BYTES ((size_t)1 << 30)
static_assert(ASX_NCC_MIN_ENERGY == 1e-6, "the header's floor");

// The plan's NCC set: r (8N bytes per pair) and the per-lag table (16N bytes per source track) of one NCC group, plus the chunk sums.
static int ensure_ncc(asx_plan *p, const char *fn, hipStream_t s)
{
    if (p->ncc.w.r) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's NCC workspace does not exist yet and cannot be allocated during a stream capture; make one call "
                    "outside the capture first", fn);
    const size_t N = p->host.N;
    const size_t g = std::max<size_t>(1, std::min(p->group, ASX_NCC_WS_BYTES / (24 * N)));
    const size_t chunks = g * ((size_t)asx_ncc_chunks((uint32_t)(2 * N)) + asx_ncc_chunks((uint32_t)N));
    if (asx_mem_whole(p->ncc.mem, p->ncc.w, [&](AsxMemSet &m, AsxNccWs &T) {
            return m.take(&T.r, g * 2 * N) || m.take(&T.table, g * N) || m.take(&T.raw, chunks) || m.take(&T.m1, chunks) ||
                           m.take(&T.m2, chunks) || m.take(&T.sstat, g * ASX_NCC_STAT) || m.take(&T.ystat, g * ASX_NCC_STAT) ||
                           m.take(&T.best, g) || m.take(&T.tk, g)
                       ? -1 : 0;
        }))
        return fail("%s: hipMalloc of the NCC workspace failed: %s", fn, hipGetErrorString(g_take_err));
    p->ncc.group = g;
    return 0;
}

// The plan's NCC track set holds at least nsrc source and nsmp sample tracks: 16N bytes of table per source track, three doubles per
// chunk of 2048 frames and four per track.  Grown as the bank is (ensure_bank): everything reallocated behind a device synchronisation,
// never inside a stream capture.
static int ensure_ncc_tracks(asx_plan *p, const char *fn, size_t nsrc, size_t nsmp, hipStream_t s)
{
    asx_plan::Ncc &C = p->ncc;
    if (nsrc <= C.nsrc && nsmp <= C.nsmp) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's NCC track set holds %zu x %zu tracks and cannot grow to %zu x %zu during a stream capture; make a "
                    "call with pools at least this large outside the capture first", fn, C.nsrc, C.nsmp, nsrc, nsmp);
    const size_t N = p->host.N, ns = std::max(nsrc, C.nsrc), nm = std::max(nsmp, C.nsmp);
    const size_t chunks = ns * asx_ncc_chunks((uint32_t)(2 * N)) + nm * asx_ncc_chunks((uint32_t)N);
    HIP_TRY(hipDeviceSynchronize());
    C.tmem.clear(); C.tracks = AsxNccWs{}; C.nsrc = C.nsmp = 0;
    if (asx_mem_whole(C.tmem, C.tracks, [&](AsxMemSet &m, AsxNccWs &T) {
            return m.take(&T.table, ns * N) || m.take(&T.raw, chunks) || m.take(&T.m1, chunks) || m.take(&T.m2, chunks) ||
                           m.take(&T.sstat, ns * ASX_NCC_STAT) || m.take(&T.ystat, nm * ASX_NCC_STAT)
                       ? -1 : 0;
        }))
        return fail("%s: cannot allocate the plan's NCC track set for %zu source and %zu sample tracks (%zu bytes per source track)", fn,
                    ns, nm, 16 * N);
    C.nsrc = ns; C.nsmp = nm;
    return 0;
}

// After the entry point's null checks and the top-k option's.  c_out: the debug call's curve (one contiguous pair), else null.
// pool: null (the strided forms: d_source and d_sample are pair 0's tracks), or the pool call's pairs (they are the two pools).
// topk.k > 1: y's entry stride is k.
static int ncc_batch(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample, size_t sample_stride,
                     const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy, float *c_out, const Results &y,
                     void *stream, const PoolCall *pool = nullptr, const Topk &topk = {})
{
    if (!(min_energy >= ASX_NCC_MIN_ENERGY && min_energy <= 1.0)) // (a NaN fails both)
        return fail("%s: min_energy %g is not in [%g, 1]", fn, min_energy, (double)ASX_NCC_MIN_ENERGY);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    const AsxDev &P = p->dev;
    if (pool ? pool_layout(p, fn, d_source, source_stride, pool->nsrc, d_sample, sample_stride, pool->nsmp, pool->rows, batch)
             : strided_layout(p, fn, d_source, source_stride, d_sample, sample_stride))
        return -1;
    if (batch == 0) return 0;
    if (pool && (ensure_bank(p, fn, pool->nsrc, pool->nsmp, s) || ensure_ncc_tracks(p, fn, pool->nsrc, pool->nsmp, s))) return -1;
    if (ensure_ncc(p, fn, s)) return -1;
    int bc = 0;
    if (!pool && strided_broadcast(p, fn, d_source, source_stride, d_sample, sample_stride, s, &bc)) return -1;
    if (pool) {
        // once per call, before the groups: every track's forward column pass into the bank and its moments into the track set
        pool_fill(p, d_source, source_stride, pool->nsrc, d_sample, sample_stride, pool->nsmp, s);
        asx_launch_ncc_pool_moments(p->ncc.tracks, d_source, source_stride, pool->nsrc, d_sample, sample_stride, pool->nsmp, P.N, s);
        p->ncc.built_src += pool->nsrc;
        p->ncc.built_smp += pool->nsmp;
    }
    // the transforms see no rows: every lag's r is wanted, and the rows are this call's own (0 <= lag_min <= lag_max <= N-1)
    const Pairs<float> x = pool ? Pairs<float>::pooled(pool, d_source, source_stride, d_sample, sample_stride, nullptr, 0)
                                : Pairs<float>::strided(d_source, source_stride, d_sample, sample_stride, bc, nullptr, 0);
    asx_plan::Lane &L = p->lanes[0];
    const AsxPoolPair *pl = pool ? L.pool : nullptr; // the group's records, which run_group resolves
    const int K = topk.k;
    prof_begin_call(p);
    size_t gi = 0;
    for (size_t done = 0; done < batch; done += p->ncc.group, gi++) {
        const size_t g = std::min(p->ncc.group, batch - done);
        const Pairs<float> xg = x.at(done);
        const Results yg = y.at(done);
        const int64_t *rows = d_windows ? d_windows + 2 * done * window_stride : nullptr;
        AsxNccWs W = p->ncc.w;
        if (pool) {
            // a pair's table and statistics: those of its slots in the track set
            W.table = p->ncc.tracks.table; W.sstat = p->ncc.tracks.sstat; W.ystat = p->ncc.tracks.ystat;
            W.nsrc = W.nsmp = 0;
            W.do_src = W.do_smp = false;
        } else {
            // a track every pair shares (a stride of 0, whatever the layout): its moments once per call, by the first group
            W.nsrc = source_stride == 0 ? 1u : (uint32_t)g;
            W.nsmp = sample_stride == 0 ? 1u : (uint32_t)g;
            W.do_src = source_stride != 0 || done == 0;
            W.do_smp = sample_stride != 0 || done == 0;
            if (W.do_src) p->ncc.built_src += W.nsrc;
            if (W.do_smp) p->ncc.built_smp += W.nsmp;
        }
        if (run_group(p, xg, g, yg, s, { .prof_group = gi, .listed = false, .f32_abi = false, .r_out = W.r, .transforms_only = true }))
            return -1;
        if (!pool) asx_launch_ncc_moments(W, xg.src, source_stride, xg.smp, sample_stride, P.N, s);
        asx_launch_ncc_peak(W, W.r, P.nout, P.N, (double)P.F, min_energy, rows, window_stride, c_out, L.seg, yg.peak, (int)g, s, pl, K);
        const AsxInputs<float> in = xg.inputs(pl);
        if (K == 1) {
            // the reference's coefficient of the samples at the winner, in the direct form
            asx_launch_pearson(in, P.N, L.seg, L.psums, yg.lag, yg.coef, yg.ret, (int)g, s);
            if (rows) asx_launch_ncc_invalid(P.N, rows, window_stride, yg.lag, yg.coef, yg.peak, yg.ret, (int)g, s);
            if (pl) asx_launch_invalid_pairs(pl, yg.lag, yg.coef, yg.ret, yg.peak, (int)g, s);
        } else {
            // Entry j: its lag from the pass's maximum (k_ncctop_step), the direct form at that lag into the lane's temporaries, which the
            // next step moves to the caller's arrays; pass j + 1 rescans the curve that k_ncc_peak left (k_ncctop_scan).
            for (int j = 0; j <= K; j++) {
                if (j > 0 && j < K) asx_launch_ncctop_scan(W, P.nout, P.N, rows, window_stride, topk.sep, j, (int)g, s);
                asx_launch_ncctop_step(W, P.N, rows, window_stride, topk.sep, j, K, L.seg, L.tk.lag, L.tk.coef, L.tk.ret, yg.lag, yg.coef,
                                       yg.peak, yg.ret, (int)g, s);
                if (j < K) asx_launch_pearson(in, P.N, L.seg, L.psums, L.tk.lag, L.tk.coef, L.tk.ret, (int)g, s);
            }
            if (pl) asx_launch_invalid_pairs_k(pl, K, yg.lag, yg.coef, yg.ret, yg.peak, (int)g, s);
        }
        HIP_TRY(hipGetLastError());
    }
    prof_end_call(p, gi);
    return 0;
}

static bool ncc_topk_option(const char *fn, int k, int64_t min_separation)
{
    if (k < 1 || k > ASX_TOPK_MAX) return fail("%s: k = %d is not in [1, %d]", fn, k, ASX_TOPK_MAX), false;
    if (min_separation < 0) return fail("%s: min_separation = %lld is negative", fn, (long long)min_separation), false;
    return true;
}

// The K strongest separated lags of the coefficient curve: k = 1 launches exactly asx_xcorr_ncc_f32_dev.
extern "C" int asx_xcorr_ncc_topk_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                          size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                          double min_energy, int k, int64_t min_separation, int64_t *d_lag, double *d_coef, double *d_peak,
                                          int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_topk_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    if (!ncc_topk_option(fn, k, min_separation)) return -1;
    return ncc_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch, min_energy, nullptr,
                     { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, nullptr, Topk{ k, min_separation });
}

// The NCC call over listed pairs of two pools: the bank filled and every track's moments formed once per call.
extern "C" int asx_xcorr_pool_ncc_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                          const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                          const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy, int64_t *d_lag,
                                          double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_ncc_f32_dev";
    if (!p || !d_sources || !d_samples || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    const PoolCall pool{ d_pairs, nsources, nsamples };
    return ncc_batch(p, fn, d_sources, source_stride, d_samples, sample_stride, d_windows, window_stride, batch, min_energy, nullptr,
                     { d_lag, d_coef, d_ret, 1, d_peak }, stream, &pool);
}

// ... with the K strongest separated lags per pair: k = 1 launches exactly asx_xcorr_pool_ncc_f32_dev.
extern "C" int asx_xcorr_pool_ncc_topk_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                               const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                               const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy, int k,
                                               int64_t min_separation, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret,
                                               void *stream)
{
    static const char *fn = "asx_xcorr_pool_ncc_topk_f32_dev";
    if (!p || !d_sources || !d_samples || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    if (!ncc_topk_option(fn, k, min_separation)) return -1;
    const PoolCall pool{ d_pairs, nsources, nsamples };
    return ncc_batch(p, fn, d_sources, source_stride, d_samples, sample_stride, d_windows, window_stride, batch, min_energy, nullptr,
                     { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, &pool, Topk{ k, min_separation });
}

// diagnostic: the NCC track set's capacity (sources, samples), and the source tables and sample moment sets built over the plan's life
extern "C" int asx_plan_debug_ncc(asx_plan *p, uint64_t out[4])
{
    if (!p || !out) return -1;
    out[0] = p->ncc.nsrc; out[1] = p->ncc.nsmp;
    out[2] = p->ncc.built_src; out[3] = p->ncc.built_smp;
    return 0;
}

// diagnostic (not in the public header): the float64 tables behind the coefficient, as the last call left them in one of the plan's
// sets.  which: 0 the NCC set (the tracks of the last NCC group; one track where the stride was 0), 1 the pool calls' track set,
// 2 the full-range set (as 0, plus the two tables of the negative lags), 3 the pool full-range calls' track set (the tracks of the
// last such call by pool index: table and statistics from the pool calls' track set, which that call filled, plus the two tables).
//   sstat[2]  the source track's mu and Vmax          ystat[3]  the sample track's mean, Sy, Vy
//   table     [N] {Sx' (mu-shifted), Vx} of the lags 0..N-1, as 2N doubles
//   ptab, ttab  which = 2 and 3 only, else ignored: [N] {P1[m], Vx of x[0, m)} and {T1[m], Vy of y[N - m, N)} as 2N doubles each; the
//             entries m = 1..N-1 are copied, entry 0 (which no kernel writes) is left as the caller had it
// An output may be null: it is not copied.  Synchronises the device; launches nothing and changes nothing.
extern "C" int asx_plan_debug_ncc_tables(asx_plan *p, int which, size_t source_track, size_t sample_track, double *sstat, double *ystat,
                                         double *table, double *ptab, double *ttab)
{
    static const char *fn = "asx_plan_debug_ncc_tables";
    if (!p) return fail("%s: null plan", fn);
    if (which < 0 || which > 3) return fail("%s: which = %d is not 0 (strided), 1 (pool), 2 (full) or 3 (pool full)", fn, which);
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    const bool pooled = which == 1 || which == 3;
    const AsxNccWs &W = which == 0 ? p->ncc.w : pooled ? p->ncc.tracks : p->nccfull.set.w;
    const size_t ns = which == 0 ? p->ncc.group : which == 1 ? p->ncc.nsrc : which == 2 ? p->nccfull.group : p->nccfull.nsrc;
    const size_t nm = which == 1 ? p->ncc.nsmp : which == 3 ? p->nccfull.nsmp : ns;
    if (!W.table || (which == 3 && !p->nccfull.pool.tracks.ptab))
        return fail("%s: the plan has no such set yet (which = %d): make a call that fills it first", fn, which);
    if (source_track >= ns || sample_track >= nm)
        return fail("%s: track (%zu, %zu) is outside the set's %zu source and %zu sample tracks", fn, source_track, sample_track, ns, nm);
    HIP_TRY(hipDeviceSynchronize());
    const size_t N = p->host.N;
    if (sstat) HIP_TRY(hipMemcpy(sstat, W.sstat + source_track * ASX_NCC_STAT, 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (ystat) {
        double st[ASX_NCC_STAT];
        HIP_TRY(hipMemcpy(st, W.ystat + sample_track * ASX_NCC_STAT, sizeof st, hipMemcpyDeviceToHost));
        ystat[0] = st[0]; ystat[1] = st[2]; ystat[2] = st[3];
    }
    if (table) HIP_TRY(hipMemcpy(table, W.table + source_track * N, N * sizeof(double2), hipMemcpyDeviceToHost));
    if (which >= 2 && N > 1) {
        const AsxNccFullWs &F = which == 2 ? p->nccfull.set.f : p->nccfull.pool.tracks;
        if (ptab) HIP_TRY(hipMemcpy(ptab + 2, F.ptab + source_track * N + 1, (N - 1) * sizeof(double2), hipMemcpyDeviceToHost));
        if (ttab) HIP_TRY(hipMemcpy(ttab + 2, F.ttab + sample_track * N + 1, (N - 1) * sizeof(double2), hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int asx_xcorr_ncc_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                     size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                     double min_energy, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("asx_xcorr_ncc_f32_dev: null argument");
    return ncc_batch(p, "asx_xcorr_ncc_f32_dev", d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch,
                     min_energy, nullptr, { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

extern "C" int asx_xcorr_ncc_debug_c_dev(asx_plan *p, const float *d_source, const float *d_sample, double min_energy, float *d_c,
                                         int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    if (!p || !d_source || !d_sample || !d_c || !d_coef || !d_peak || !d_ret) return fail("asx_xcorr_ncc_debug_c_dev: null argument");
    const size_t N = p->host.N;
    return ncc_batch(p, "asx_xcorr_ncc_debug_c_dev", d_source, 2 * N, d_sample, N, nullptr, 0, 1, min_energy, d_c,
                     { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

// ---------------------------------------------------------------------------
// full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev): the lags -(N-1)..N-1, two transform passes per group
// ---------------------------------------------------------------------------
// The plan's full-range set, per pair of one group: two r buffers (16N bytes; a top-k group keeps the curve in the halves that nothing
// reads), per source track the staged x_lo (8N) and the tables of the lags >= 0 and < 0 (16N each), per sample track the suffix table
// (16N): ASX_NCCFULL_PAIR_BYTES * N bytes where every pair has tracks of its own, plus the chunk sums.
#define ASX_NCCFULL_PAIR_BYTES 72
static int ensure_ncc_full(asx_plan *p, const char *fn, hipStream_t s)
{
    if (p->nccfull.set.w.r) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's full-range NCC workspace does not exist yet and cannot be allocated during a stream capture; make "
                    "one call outside the capture first", fn);
    const size_t N = p->host.N, pitch = (2 * N + 3) & ~(size_t)3;
    const size_t g = std::max<size_t>(1, std::min(p->group, ASX_NCC_WS_BYTES / (ASX_NCCFULL_PAIR_BYTES * N)));
    const size_t chunks = g * ((size_t)asx_ncc_chunks((uint32_t)(2 * N)) + asx_ncc_chunks((uint32_t)N));
    if (asx_mem_whole(p->nccfull.mem, p->nccfull.set, [&](AsxMemSet &m, asx_plan::NccFull::Set &T) {
            T.f.pitch = pitch;
            return m.take(&T.w.r, g * 2 * N) || m.take(&T.w.table, g * N) || m.take(&T.w.raw, chunks) || m.take(&T.w.m1, chunks) ||
                           m.take(&T.w.m2, chunks) || m.take(&T.w.sstat, g * ASX_NCC_STAT) || m.take(&T.w.ystat, g * ASX_NCC_STAT) ||
                           m.take(&T.w.best, g) || m.take(&T.w.tk, g) || m.take(&T.f.rlo, g * 2 * N) || m.take(&T.f.stage, g * pitch) ||
                           m.take(&T.f.ptab, g * N) || m.take(&T.f.ttab, g * N)
                       ? -1 : 0;
        }))
        return fail("%s: hipMalloc of the full-range NCC workspace failed: %s", fn, hipGetErrorString(g_take_err));
    p->nccfull.group = g;
    return 0;
}

// ncc_batch's sibling for the strided full-range calls, after the entry point's null checks and the top-k option's.  c_out: the debug
// call's curve (one contiguous pair, 2N - 1 floats), else null.  topk.k > 1: y's entry stride is k.
static int ncc_full_batch(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample,
                          size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy,
                          int64_t min_overlap, float *c_out, const Results &y, void *stream, const Topk &topk = {})
{
    if (!(min_energy >= ASX_NCC_MIN_ENERGY && min_energy <= 1.0)) // (a NaN fails both)
        return fail("%s: min_energy %g is not in [%g, 1]", fn, min_energy, (double)ASX_NCC_MIN_ENERGY);
    if (min_overlap < 1 || min_overlap > (int64_t)p->host.N)
        return fail("%s: min_overlap %lld is not in [1, %zu]", fn, (long long)min_overlap, p->host.N);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    const AsxDev &P = p->dev;
    if (strided_layout(p, fn, d_source, source_stride, d_sample, sample_stride)) return -1;
    if (batch == 0) return 0;
    if (ensure_ncc_full(p, fn, s)) return -1;
    int bc = 0;
    if (strided_broadcast(p, fn, d_source, source_stride, d_sample, sample_stride, s, &bc)) return -1;
    const Pairs<float> x = Pairs<float>::strided(d_source, source_stride, d_sample, sample_stride, bc, nullptr, 0);
    asx_plan::Lane &L = p->lanes[0];
    const AsxNccFullWs &F = p->nccfull.set.f;
    const int K = topk.k;
    // the slot holds one source spectrum: the shared source's for pass A, its x_lo's for pass B
    auto slot_source = [&](const float *track) { asx_launch_fwd_cols_r(P, track, 0, nullptr, 0, 0, 1, p->bslot, true, s); };
    prof_begin_call(p);
    size_t gi = 0;
    for (size_t done = 0; done < batch; done += p->nccfull.group, gi++) {
        const size_t g = std::min(p->nccfull.group, batch - done);
        const Pairs<float> xg = x.at(done);
        const Results yg = y.at(done);
        const int64_t *rows = d_windows ? d_windows + 2 * done * window_stride : nullptr;
        AsxNccWs W = p->nccfull.set.w;
        // a track every pair shares (a stride of 0, whatever the layout): its moments, x_lo and tables once per call, by the first group
        W.nsrc = source_stride == 0 ? 1u : (uint32_t)g;
        W.nsmp = sample_stride == 0 ? 1u : (uint32_t)g;
        W.do_src = source_stride != 0 || done == 0;
        W.do_smp = sample_stride != 0 || done == 0;
        if (W.do_src) p->ncc.built_src += W.nsrc;
        if (W.do_smp) p->ncc.built_smp += W.nsmp;
        // pass A: the NCC call's own group on the caller's tracks -> r of the lags >= 0, then that call's moment kernels
        if ((bc & 1) && done > 0) slot_source(d_source);
        if (run_group(p, xg, g, yg, s, { .prof_group = gi, .listed = false, .f32_abi = false, .r_out = W.r, .transforms_only = true }))
            return -1;
        asx_launch_ncc_moments(W, xg.src, source_stride, xg.smp, sample_stride, P.N, s);
        // pass B: the same samples against x_lo -> r of the lags < 0 without the products that wrap around
        if (W.do_src) asx_launch_nccfull_stage(F, xg.src, source_stride, W.nsrc, P.N, s);
        if (bc & 1) slot_source(F.stage);
        const Pairs<float> xlo = Pairs<float>::strided(F.stage, source_stride == 0 ? 0 : F.pitch, xg.smp, sample_stride, bc, nullptr, 0);
        if (run_group(p, xlo, g, yg, s, { .prof_group = GroupOpts::no_marks, .listed = false, .f32_abi = false, .r_out = F.rlo,
                                          .transforms_only = true }))
            return -1;
        asx_launch_nccfull_prefix(W, F, xg.src, source_stride, xg.smp, sample_stride, P.N, s);
        asx_launch_nccfull_peak(W, F, P.nout, P.N, (double)P.F, min_energy, min_overlap, rows, window_stride, c_out, L.seg, yg.peak, (int)g,
                                s, K);
        const AsxInputs<float> in = xg.inputs(nullptr);
        if (K == 1) {
            // the reference's coefficient of the samples at the winner, in the direct form
            asx_launch_pearson(in, P.N, L.seg, L.psums, yg.lag, yg.coef, yg.ret, (int)g, s);
            if (rows) asx_launch_nccfull_invalid(P.N, rows, window_stride, yg.lag, yg.coef, yg.peak, yg.ret, (int)g, s);
        } else {
            // ncc_batch's passes over the signed curve
            for (int j = 0; j <= K; j++) {
                if (j > 0 && j < K) asx_launch_nccfull_scan(W, F, P.nout, P.N, rows, window_stride, topk.sep, j, (int)g, s);
                asx_launch_nccfull_step(W, P.N, rows, window_stride, topk.sep, j, K, L.seg, L.tk.lag, L.tk.coef, L.tk.ret, yg.lag, yg.coef,
                                        yg.peak, yg.ret, (int)g, s);
                if (j < K) asx_launch_pearson(in, P.N, L.seg, L.psums, L.tk.lag, L.tk.coef, L.tk.ret, (int)g, s);
            }
        }
        HIP_TRY(hipGetLastError());
    }
    prof_end_call(p, gi);
    return 0;
}

extern "C" int asx_xcorr_ncc_full_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                          size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                          double min_energy, int64_t min_overlap, int64_t *d_lag, double *d_coef, double *d_peak,
                                          int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_full_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    return ncc_full_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch, min_energy,
                          min_overlap, nullptr, { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

// The K strongest separated lags of the full-range curve: k = 1 launches exactly asx_xcorr_ncc_full_f32_dev.
extern "C" int asx_xcorr_ncc_full_topk_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                               size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch,
                                               double min_energy, int64_t min_overlap, int k, int64_t min_separation, int64_t *d_lag,
                                               double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_full_topk_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    if (!ncc_topk_option(fn, k, min_separation)) return -1;
    return ncc_full_batch(p, fn, d_source, source_stride, d_sample, sample_stride, d_windows, window_stride, batch, min_energy,
                          min_overlap, nullptr, { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, Topk{ k, min_separation });
}

extern "C" int asx_xcorr_ncc_full_debug_c_dev(asx_plan *p, const float *d_source, const float *d_sample, double min_energy,
                                              int64_t min_overlap, float *d_c, int64_t *d_lag, double *d_coef, double *d_peak,
                                              int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_full_debug_c_dev";
    if (!p || !d_source || !d_sample || !d_c || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    const size_t N = p->host.N;
    return ncc_full_batch(p, fn, d_source, 2 * N, d_sample, N, nullptr, 0, 1, min_energy, min_overlap, d_c,
                          { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

// ---------------------------------------------------------------------------
// ragged NCC (asx_xcorr_ncc_ragged_f32_dev): the full-range curve for pairs whose tracks hold Ls <= 2N and Lm <= N frames
// ---------------------------------------------------------------------------
// The plan's ragged set, per pair of one group: the staged x', x_lo' (8N bytes each) and y' (4N), two r buffers (16N), the prefix
// tables of 2N + 1 and N + 1 double2 (32N + 16N): ASX_NCCRAG_PAIR_BYTES * N bytes, plus the chunk sums.  Every pair has all of it,
// a broadcast track's too.
#define ASX_NCCRAG_PAIR_BYTES 84
static int ensure_ncc_ragged(asx_plan *p, const char *fn, hipStream_t s)
{
    if (p->nccrag.w.r) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's ragged NCC workspace does not exist yet and cannot be allocated during a stream capture; make "
                    "one call outside the capture first", fn);
    const size_t N = p->host.N, xpitch = (2 * N + 3) & ~(size_t)3, ypitch = (N + 3) & ~(size_t)3;
    const size_t g = std::max<size_t>(1, std::min(p->group, ASX_NCC_WS_BYTES / (ASX_NCCRAG_PAIR_BYTES * N)));
    const size_t chunks = g * ((size_t)asx_ncc_chunks((uint32_t)(2 * N)) + asx_ncc_chunks((uint32_t)N));
    if (asx_mem_whole(p->nccrag.mem, p->nccrag.w, [&](AsxMemSet &m, AsxNccRagWs &T) {
            T.xpitch = xpitch; T.ypitch = ypitch;
            return m.take(&T.xs, g * xpitch) || m.take(&T.xlo, g * xpitch) || m.take(&T.ys, g * ypitch) || m.take(&T.r, g * 2 * N) ||
                           m.take(&T.rlo, g * 2 * N) || m.take(&T.pa, g * (2 * N + 1)) || m.take(&T.pb, g * (N + 1)) ||
                           m.take(&T.raw, chunks) || m.take(&T.m1, chunks) || m.take(&T.m2, chunks) ||
                           m.take(&T.stat, g * ASX_NCC_STAT) || m.take(&T.best, g) || m.take(&T.tk, g)
                       ? -1 : 0;
        }))
        return fail("%s: hipMalloc of the ragged NCC workspace failed: %s", fn, hipGetErrorString(g_take_err));
    p->nccrag.group = g;
    return 0;
}

// ncc_full_batch's sibling for the ragged calls, after the entry point's null checks and the top-k option's.  lens: where a pair's
// {Ls, Lm} is read (AsxRagLens: device rows, or one pair of values).  c_out: the debug call's curve (one contiguous pair, 2N - 1
// floats), else null.  topk.k > 1: y's entry stride is k.  The transforms read the staged copies only, with no broadcast slot: a
// shared track is cut per pair.
static int ncc_ragged_batch(asx_plan *p, const char *fn, const float *d_source, size_t source_stride, const float *d_sample,
                            size_t sample_stride, const AsxRagLens &lens, const int64_t *d_windows, size_t window_stride, size_t batch,
                            double min_energy, int64_t min_overlap, float *c_out, const Results &y, void *stream, const Topk &topk = {})
{
    if (!(min_energy >= ASX_NCC_MIN_ENERGY && min_energy <= 1.0)) // (a NaN fails both)
        return fail("%s: min_energy %g is not in [%g, 1]", fn, min_energy, (double)ASX_NCC_MIN_ENERGY);
    if (min_overlap < 1 || min_overlap > (int64_t)p->host.N)
        return fail("%s: min_overlap %lld is not in [1, %zu]", fn, (long long)min_overlap, p->host.N);
    if (!lens.rows && lens.step != 0)
        return fail("%s: length_stride %zu without lengths (d_lengths is null)", fn, lens.step);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    const AsxDev &P = p->dev;
    if (strided_layout(p, fn, d_source, source_stride, d_sample, sample_stride)) return -1;
    if (batch == 0) return 0;
    if (ensure_ncc_ragged(p, fn, s)) return -1;
    asx_plan::Lane &L = p->lanes[0];
    const AsxNccRagWs &R = p->nccrag.w;
    // what k_nccfull_scan and k_nccfull_step take of a group: the two r buffers that keep the curve, the maxima and the records
    AsxNccWs W{};
    W.r = R.r; W.best = R.best; W.tk = R.tk;
    AsxNccFullWs F{};
    F.rlo = R.rlo;
    const int K = topk.k;
    const Pairs<float> x = Pairs<float>::strided(d_source, source_stride, d_sample, sample_stride, 0, nullptr, 0);
    const Pairs<float> xa = Pairs<float>::strided(R.xs, R.xpitch, R.ys, R.ypitch, 0, nullptr, 0);
    const Pairs<float> xb = Pairs<float>::strided(R.xlo, R.xpitch, R.ys, R.ypitch, 0, nullptr, 0);
    prof_begin_call(p);
    size_t gi = 0;
    for (size_t done = 0; done < batch; done += p->nccrag.group, gi++) {
        const size_t g = std::min(p->nccrag.group, batch - done);
        const Pairs<float> xg = x.at(done);
        const Results yg = y.at(done);
        const int64_t *rows = d_windows ? d_windows + 2 * done * window_stride : nullptr;
        AsxRagLens lg = lens;
        if (lg.rows) lg.rows += 2 * done * lg.step;
        asx_launch_nccrag_tracks(R, lg, xg.src, source_stride, xg.smp, sample_stride, P.N, (int)g, s);
        // pass A: (x', y') -> r of the lags >= 0; pass B: (x_lo', y') -> r of the lags < 0
        if (run_group(p, xa, g, yg, s, { .prof_group = gi, .listed = false, .f32_abi = false, .r_out = R.r, .transforms_only = true }))
            return -1;
        if (run_group(p, xb, g, yg, s, { .prof_group = GroupOpts::no_marks, .listed = false, .f32_abi = false, .r_out = R.rlo,
                                         .transforms_only = true }))
            return -1;
        asx_launch_nccrag_peak(R, lg, P.N, (double)P.F, min_energy, min_overlap, rows, window_stride, c_out, L.seg, yg.peak, (int)g, s, K);
        // the reference's coefficient over the overlap, in the direct form, from the caller's tracks
        const AsxInputs<float> in = xg.inputs(nullptr);
        if (K == 1) {
            asx_launch_pearson(in, P.N, L.seg, L.psums, yg.lag, yg.coef, yg.ret, (int)g, s);
            if (rows) asx_launch_nccfull_invalid(P.N, rows, window_stride, yg.lag, yg.coef, yg.peak, yg.ret, (int)g, s);
        } else {
            // ncc_full_batch's passes; behind each step the entry's segment by the pair's lengths
            for (int j = 0; j <= K; j++) {
                if (j > 0 && j < K) asx_launch_nccfull_scan(W, F, P.nout, P.N, rows, window_stride, topk.sep, j, (int)g, s);
                asx_launch_nccfull_step(W, P.N, rows, window_stride, topk.sep, j, K, L.seg, L.tk.lag, L.tk.coef, L.tk.ret, yg.lag, yg.coef,
                                        yg.peak, yg.ret, (int)g, s);
                if (j < K) {
                    asx_launch_nccrag_seg(R, lg, P.N, j, L.seg, (int)g, s);
                    asx_launch_pearson(in, P.N, L.seg, L.psums, L.tk.lag, L.tk.coef, L.tk.ret, (int)g, s);
                }
            }
        }
        if (lg.rows || !(1 <= lg.ls && lg.ls <= 2 * (int64_t)P.N && 1 <= lg.lm && lg.lm <= (int64_t)P.N))
            asx_launch_nccrag_invalid(lg, P.N, K, yg.lag, yg.coef, yg.peak, yg.ret, (int)g, s); // -5 takes precedence over -2 and -3
        HIP_TRY(hipGetLastError());
    }
    prof_end_call(p, gi);
    return 0;
}

extern "C" int asx_xcorr_ncc_ragged_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                            size_t sample_stride, const int64_t *d_lengths, size_t length_stride,
                                            const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy,
                                            int64_t min_overlap, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret,
                                            void *stream)
{
    static const char *fn = "asx_xcorr_ncc_ragged_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    const int64_t N = (int64_t)p->host.N;
    return ncc_ragged_batch(p, fn, d_source, source_stride, d_sample, sample_stride, { d_lengths, length_stride, 2 * N, N }, d_windows,
                            window_stride, batch, min_energy, min_overlap, nullptr, { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

// The K strongest separated lags of the ragged curve: k = 1 launches exactly asx_xcorr_ncc_ragged_f32_dev.
extern "C" int asx_xcorr_ncc_ragged_topk_f32_dev(asx_plan *p, const float *d_source, size_t source_stride, const float *d_sample,
                                                 size_t sample_stride, const int64_t *d_lengths, size_t length_stride,
                                                 const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy,
                                                 int64_t min_overlap, int k, int64_t min_separation, int64_t *d_lag, double *d_coef,
                                                 double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_ragged_topk_f32_dev";
    if (!p || !d_source || !d_sample || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    if (!ncc_topk_option(fn, k, min_separation)) return -1;
    const int64_t N = (int64_t)p->host.N;
    return ncc_ragged_batch(p, fn, d_source, source_stride, d_sample, sample_stride, { d_lengths, length_stride, 2 * N, N }, d_windows,
                            window_stride, batch, min_energy, min_overlap, nullptr, { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream,
                            Topk{ k, min_separation });
}

extern "C" int asx_xcorr_ncc_ragged_debug_c_dev(asx_plan *p, const float *d_source, const float *d_sample, int64_t source_len,
                                                int64_t sample_len, double min_energy, int64_t min_overlap, float *d_c, int64_t *d_lag,
                                                double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_ncc_ragged_debug_c_dev";
    if (!p || !d_source || !d_sample || !d_c || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    const size_t N = p->host.N;
    return ncc_ragged_batch(p, fn, d_source, 2 * N, d_sample, N, { nullptr, 0, source_len, sample_len }, nullptr, 0, 1, min_energy,
                            min_overlap, d_c, { d_lag, d_coef, d_ret, 1, d_peak }, stream);
}

// diagnostic: the ragged set's pairs per group and its bytes (0, 0 until the plan's first ragged call)
extern "C" int asx_plan_debug_ncc_ragged(asx_plan *p, uint64_t out[2])
{
    if (!p || !out) return -1;
    out[0] = p->nccrag.group;
    out[1] = p->nccrag.mem.bytes();
    return 0;
}

// ---------------------------------------------------------------------------
// full-range NCC over track pools (asx_xcorr_pool_ncc_full_f32_dev): the per-track work once per call, two transform passes per group
// ---------------------------------------------------------------------------
// The plan's full-range track set holds at least nsrc source and nsmp sample tracks: per source track x_lo (8N bytes), its spectrum
// (a bank row) and the prefix table (16N), per sample track the suffix table (16N), and the norm partials and band sums of a bank.
// Grown as the bank is (ensure_bank): everything reallocated behind a device synchronisation, never inside a stream capture.
static int ensure_ncc_full_tracks(asx_plan *p, const char *fn, size_t nsrc, size_t nsmp, hipStream_t s)
{
    asx_plan::NccFull &C = p->nccfull;
    if (nsrc <= C.nsrc && nsmp <= C.nsmp) return 0;
    if (stream_capturing(s))
        return fail("%s: the plan's full-range NCC track set holds %zu x %zu tracks and cannot grow to %zu x %zu during a stream "
                    "capture; make a call with pools at least this large outside the capture first", fn, C.nsrc, C.nsmp, nsrc, nsmp);
    const AsxDev &P = p->dev;
    const size_t N = p->host.N, ns = std::max(nsrc, C.nsrc), nm = std::max(nsmp, C.nsmp), pitch = (2 * N + 3) & ~(size_t)3;
    const size_t na = std::max(ns, nm), nt = P.ntiles, nb = nt * (size_t)P.nbands;
    HIP_TRY(hipDeviceSynchronize());
    C.pmem.clear(); C.pool = asx_plan::NccFull::Tracks{}; C.nsrc = C.nsmp = 0;
    if (asx_mem_whole(C.pmem, C.pool, [&](AsxMemSet &m, asx_plan::NccFull::Tracks &T) {
            T.tracks.pitch = pitch;
            return m.take(&T.tracks.stage, ns * pitch) || m.take(&T.tracks.ptab, ns * N) || m.take(&T.tracks.ttab, nm * N) ||
                           m.take(&T.bank.cx, ns * asx_spectrum_len(P)) || m.take(&T.bank.nrm, na * 2 * nt) ||
                           (nb && m.take(&T.bank.band, na * 2 * nb))
                       ? -1 : 0;
        }))
        return fail("%s: cannot allocate the plan's full-range NCC track set for %zu source and %zu sample tracks (%zu bytes per "
                    "source track, %zu per sample track)", fn, ns, nm, 24 * N + asx_spectrum_len(P) * sizeof(float2), 16 * N);
    C.nsrc = ns; C.nsmp = nm;
    return 0;
}

// ncc_full_batch's sibling for the pool calls, after the entry point's null checks and the top-k option's: ncc_batch's pools and
// ncc_full_batch's curve.  topk.k > 1: y's entry stride is k.  The per-group buffers (two r buffers per pair, best, tk) are the
// strided full-range set's, so a group of this call is that set's: min(the plan's group, one gibibyte / 72N) pairs.
static int ncc_full_pool_batch(asx_plan *p, const char *fn, const float *d_sources, size_t source_stride, const float *d_samples,
                               size_t sample_stride, const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy,
                               int64_t min_overlap, const Results &y, void *stream, const PoolCall &pool, const Topk &topk = {})
{
    if (!(min_energy >= ASX_NCC_MIN_ENERGY && min_energy <= 1.0)) // (a NaN fails both)
        return fail("%s: min_energy %g is not in [%g, 1]", fn, min_energy, (double)ASX_NCC_MIN_ENERGY);
    if (min_overlap < 1 || min_overlap > (int64_t)p->host.N)
        return fail("%s: min_overlap %lld is not in [1, %zu]", fn, (long long)min_overlap, p->host.N);
    PlanCall c(p, stream);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    hipStream_t s = c.s;
    const AsxDev &P = p->dev;
    if (pool_layout(p, fn, d_sources, source_stride, pool.nsrc, d_samples, sample_stride, pool.nsmp, pool.rows, batch)) return -1;
    if (batch == 0) return 0;
    if (ensure_bank(p, fn, pool.nsrc, pool.nsmp, s) || ensure_ncc_tracks(p, fn, pool.nsrc, pool.nsmp, s) ||
        ensure_ncc_full_tracks(p, fn, pool.nsrc, pool.nsmp, s) || ensure_ncc_full(p, fn, s))
        return -1;
    // Once per call, before the groups.  What ncc_batch does for its pools: every track's forward column pass into the bank and its
    // moments into the NCC track set ...
    pool_fill(p, d_sources, source_stride, pool.nsrc, d_samples, sample_stride, pool.nsmp, s);
    asx_launch_ncc_pool_moments(p->ncc.tracks, d_sources, source_stride, pool.nsrc, d_samples, sample_stride, pool.nsmp, P.N, s);
    p->ncc.built_src += pool.nsrc;
    p->ncc.built_smp += pool.nsmp;
    // ... and what the negative lags add: x_lo of every source track and the prefix and suffix tables, then the forward column pass
    // of every x_lo into the second bank, whose sample side is the first bank's (the samples are the same in both passes: their norm
    // partials and band sums are copied, their spectra shared)
    AsxNccFullWs F = p->nccfull.pool.tracks;
    AsxSpectra B = p->nccfull.pool.bank;
    asx_launch_nccfull_pool_tracks(p->ncc.tracks, F, d_sources, source_stride, pool.nsrc, d_samples, sample_stride, pool.nsmp, P.N, s);
    p->nccfull.staged += pool.nsrc;
    p->nccfull.suffixed += pool.nsmp;
    {
        const size_t na = std::max(pool.nsrc, pool.nsmp), nt = P.ntiles, nb = nt * (size_t)P.nbands;
        HIP_TRY(hipMemcpyAsync(B.nrm, p->bank.c.nrm, na * 2 * nt * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (nb) HIP_TRY(hipMemcpyAsync(B.band, p->bank.c.band, na * 2 * nb * sizeof(float2), hipMemcpyDeviceToDevice, s));
        B.cy = p->bank.c.cy;
        for (size_t c0 = 0; c0 < pool.nsrc; c0 += 65535)
            asx_launch_fwd_cols_r(P, F.stage, F.pitch, nullptr, 0, c0, (int)std::min<size_t>(65535, pool.nsrc - c0), B, true, s);
    }
    // the transforms see no rows: every lag's r is wanted, and the rows are this call's own (-(N-1) <= lag_min <= lag_max <= N-1)
    const Pairs<float> x = Pairs<float>::pooled(&pool, d_sources, source_stride, d_samples, sample_stride, nullptr, 0);
    asx_plan::Lane &L = p->lanes[0];
    const AsxPoolPair *pl = L.pool; // the group's records, which run_group resolves
    F.rlo = p->nccfull.set.f.rlo;
    const int K = topk.k;
    prof_begin_call(p);
    size_t gi = 0;
    for (size_t done = 0; done < batch; done += p->nccfull.group, gi++) {
        const size_t g = std::min(p->nccfull.group, batch - done);
        const Pairs<float> xg = x.at(done);
        const Results yg = y.at(done);
        const int64_t *rows = d_windows ? d_windows + 2 * done * window_stride : nullptr;
        // the group's r buffers, best and tk; a pair's tables and statistics: those of its slots in the two track sets
        AsxNccWs W = p->nccfull.set.w;
        W.table = p->ncc.tracks.table; W.sstat = p->ncc.tracks.sstat; W.ystat = p->ncc.tracks.ystat;
        W.nsrc = W.nsmp = 0;
        W.do_src = W.do_smp = false;
        // pass A: the bank's rows -> r of the lags >= 0; pass B: the same samples against the rows of x_lo -> r of the lags < 0
        if (run_group(p, xg, g, yg, s, { .prof_group = gi, .listed = false, .f32_abi = false, .r_out = W.r, .transforms_only = true }))
            return -1;
        if (run_group(p, xg, g, yg, s, { .prof_group = GroupOpts::no_marks, .listed = false, .f32_abi = false, .r_out = F.rlo,
                                         .transforms_only = true, .bank = &B }))
            return -1;
        asx_launch_nccfp_peak(W, F, P.nout, P.N, (double)P.F, min_energy, min_overlap, rows, window_stride, L.seg, yg.peak, (int)g, s, pl, K);
        const AsxInputs<float> in = xg.inputs(pl);
        if (K == 1) {
            // the reference's coefficient of the samples at the winner, in the direct form
            asx_launch_pearson(in, P.N, L.seg, L.psums, yg.lag, yg.coef, yg.ret, (int)g, s);
            if (rows) asx_launch_nccfull_invalid(P.N, rows, window_stride, yg.lag, yg.coef, yg.peak, yg.ret, (int)g, s);
            asx_launch_invalid_pairs(pl, yg.lag, yg.coef, yg.ret, yg.peak, (int)g, s);
        } else {
            // ncc_full_batch's passes over the signed curve
            for (int j = 0; j <= K; j++) {
                if (j > 0 && j < K) asx_launch_nccfull_scan(W, F, P.nout, P.N, rows, window_stride, topk.sep, j, (int)g, s);
                asx_launch_nccfull_step(W, P.N, rows, window_stride, topk.sep, j, K, L.seg, L.tk.lag, L.tk.coef, L.tk.ret, yg.lag, yg.coef,
                                        yg.peak, yg.ret, (int)g, s);
                if (j < K) asx_launch_pearson(in, P.N, L.seg, L.psums, L.tk.lag, L.tk.coef, L.tk.ret, (int)g, s);
            }
            asx_launch_invalid_pairs_k(pl, K, yg.lag, yg.coef, yg.ret, yg.peak, (int)g, s);
        }
        HIP_TRY(hipGetLastError());
    }
    prof_end_call(p, gi);
    return 0;
}

// The full-range NCC call over listed pairs of two pools.
extern "C" int asx_xcorr_pool_ncc_full_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                               const float *d_samples, size_t sample_stride, size_t nsamples, const int32_t *d_pairs,
                                               const int64_t *d_windows, size_t window_stride, size_t batch, double min_energy,
                                               int64_t min_overlap, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret,
                                               void *stream)
{
    static const char *fn = "asx_xcorr_pool_ncc_full_f32_dev";
    if (!p || !d_sources || !d_samples || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    return ncc_full_pool_batch(p, fn, d_sources, source_stride, d_samples, sample_stride, d_windows, window_stride, batch, min_energy,
                               min_overlap, { d_lag, d_coef, d_ret, 1, d_peak }, stream, PoolCall{ d_pairs, nsources, nsamples });
}

// ... with the K strongest separated lags per pair: k = 1 launches exactly asx_xcorr_pool_ncc_full_f32_dev.
extern "C" int asx_xcorr_pool_ncc_full_topk_f32_dev(asx_plan *p, const float *d_sources, size_t source_stride, size_t nsources,
                                                    const float *d_samples, size_t sample_stride, size_t nsamples,
                                                    const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride, size_t batch,
                                                    double min_energy, int64_t min_overlap, int k, int64_t min_separation,
                                                    int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream)
{
    static const char *fn = "asx_xcorr_pool_ncc_full_topk_f32_dev";
    if (!p || !d_sources || !d_samples || !d_coef || !d_peak || !d_ret) return fail("%s: null argument", fn);
    if (!ncc_topk_option(fn, k, min_separation)) return -1;
    return ncc_full_pool_batch(p, fn, d_sources, source_stride, d_samples, sample_stride, d_windows, window_stride, batch, min_energy,
                               min_overlap, { d_lag, d_coef, d_ret, (size_t)k, d_peak }, stream, PoolCall{ d_pairs, nsources, nsamples },
                               Topk{ k, min_separation });
}

// diagnostic: the full-range track set's capacity (sources, samples), and the sources staged and the suffix tables built by the pool
// full-range calls over the plan's life
extern "C" int asx_plan_debug_ncc_full(asx_plan *p, uint64_t out[4])
{
    if (!p || !out) return -1;
    out[0] = p->nccfull.nsrc; out[1] = p->nccfull.nsmp;
    out[2] = p->nccfull.staged; out[3] = p->nccfull.suffixed;
    return 0;
}

static int ensure_staging(asx_plan *p, bool with64 = false) // with64: one pair's float64 inputs too (asx_xcorr_f64)
{
    const size_t N = p->host.N, g = p->group;
    if (!p->st.src && asx_mem_whole(p->mem, p->st, [&](AsxMemSet &m, asx_plan::Staging &T) {
            return dev_alloc(m, &T.src, g * 2 * N) || dev_alloc(m, &T.smp, g * N) || dev_alloc(m, &T.lag, g) || dev_alloc(m, &T.coef, g) ||
                   dev_alloc(m, &T.ret, g);
        }))
        return -1;
    if (with64 && !p->st64.src && asx_mem_whole(p->mem, p->st64, [&](AsxMemSet &m, asx_plan::Staging64 &T) {
            return dev_alloc(m, &T.src, 2 * N) || dev_alloc(m, &T.smp, N);
        }))
        return -1;
    return 0;
}

extern "C" int asx_xcorr_batch_f32(asx_plan *p, const float *source, const float *sample, size_t batch,
                                   int64_t *lag, double *coef, int32_t *ret)
{
    if (!p || !source || !sample || !lag || !coef || !ret) return fail("asx_xcorr_batch_f32: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    if (ensure_staging(p)) return -1;
    const size_t N = p->host.N;
    hipStream_t s = c.s;
    const Pairs<float> x = Pairs<float>::contiguous(p->st.src, p->st.smp, N);
    const Results d{ p->st.lag, p->st.coef, p->st.ret };
    prof_begin_call(p);
    for (size_t done = 0; done < batch; done += p->group) {
        const size_t g = std::min(p->group, batch - done);
        HIP_TRY(hipMemcpyAsync(p->st.src, source + done * 2 * N, g * 2 * N * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(p->st.smp, sample + done * N, g * N * sizeof(float), hipMemcpyHostToDevice, s));
        if (run_group(p, x, g, d, s) || fetch_results(p, x, g, d, { lag + done, coef + done, ret + done }, s)) return -1;
    }
    return 0;
}

// Several plans (normally one per GPU of the node) in ONE process: the batch is block-partitioned over
// them (the first batch % nplans plans get one pair more), every block runs on its plan's device from
// its own host thread, and the results land in the caller's arrays in pair order -- the "gather" of a
// single process is the D2H copy.  No data-path exchange between devices.
extern "C" int asx_xcorr_batch_multi(asx_plan *const *plans, int nplans, const float *source, const float *sample,
                                     size_t batch, int64_t *lag, double *coef, int32_t *ret)
{
    if (!plans || nplans < 1 || !source || !sample || !lag || !coef || !ret) return fail("asx_xcorr_batch_multi: bad argument");
    const size_t N = plans[0] ? plans[0]->host.N : 0;
    for (int i = 0; i < nplans; i++)
        if (!plans[i] || plans[i]->host.N != N) return fail("asx_xcorr_batch_multi: plans must share one sample_len");
    std::vector<int> rc((size_t)nplans, 0);
    std::vector<std::string> err((size_t)nplans);
    std::vector<std::thread> workers;
    const size_t base = batch / (size_t)nplans, extra = batch % (size_t)nplans;
    size_t start = 0;
    for (int i = 0; i < nplans; i++) {
        const size_t count = base + ((size_t)i < extra ? 1 : 0);
        if (count) {
            workers.emplace_back([=, &rc, &err]() {
                rc[(size_t)i] = asx_xcorr_batch_f32(plans[i], source + start * 2 * N, sample + start * N, count,
                                                    lag + start, coef + start, ret + start);
                if (rc[(size_t)i] != 0) err[(size_t)i] = asx_last_error(); // the worker thread's message
            });
        }
        start += count;
    }
    for (std::thread &t : workers) t.join();
    for (int i = 0; i < nplans; i++)
        if (rc[(size_t)i] != 0) return fail("asx_xcorr_batch_multi: plan %d: %s", i, err[(size_t)i].c_str());
    return 0;
}

// ---------------------------------------------------------------------------
// device-resident shards + RCCL result gather.  RCCL is dlopen()ed: seven entry points by name.
// ---------------------------------------------------------------------------
extern "C" int asx_shard_range(size_t total, int nshards, int shard, size_t *start, size_t *count)
{
    if (nshards < 1 || shard < 0 || shard >= nshards || !start || !count) return fail("asx_shard_range: bad argument");
    const size_t base = total / (size_t)nshards, extra = total % (size_t)nshards;
    *count = base + ((size_t)shard < extra ? 1 : 0);
    *start = (size_t)shard * base + std::min((size_t)shard, extra);
    return 0;
}

extern "C" size_t asx_result_bytes(size_t width) { return asx_shard_record_bytes(width); }

namespace {
typedef void *nccl_comm_t;
struct Rccl {
    void *handle = nullptr;
    int (*CommInitAll)(nccl_comm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int /* ncclDataType_t */, nccl_comm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*GetVersion)(int *) = nullptr;
};
std::mutex g_rccl_lock;
Rccl g_rccl;
const Rccl *rccl_load()
{
    std::lock_guard<std::mutex> g(g_rccl_lock);
    if (g_rccl.handle) return &g_rccl;
    void *h = nullptr;
    for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
        h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) { fail("cannot load librccl.so.1: %s", dlerror()); return nullptr; }
    Rccl r;
    r.handle = h;
    r.CommInitAll = (int (*)(nccl_comm_t *, int, const int *))dlsym(h, "ncclCommInitAll");
    r.CommDestroy = (int (*)(nccl_comm_t))dlsym(h, "ncclCommDestroy");
    r.AllGather = (int (*)(const void *, void *, size_t, int, nccl_comm_t, hipStream_t))dlsym(h, "ncclAllGather");
    r.GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
    r.GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
    r.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    r.GetVersion = (int (*)(int *))dlsym(h, "ncclGetVersion");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllGather || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
        fail("librccl.so.1 lacks an entry point this library binds");
        dlclose(h);
        return nullptr;
    }
    g_rccl = r;
    return &g_rccl;
}
} // namespace

struct asx_comm {
    std::vector<asx_plan *> plans;
    std::vector<int> devices;      // the plans' devices, kept here: destroy must not need the plans (they may be gone)
    std::vector<nccl_comm_t> comms;
    AsxShardState state;           // the shards' result records and the width they are sized for (shard_driver.h)
};

// the ops table of csrc/shard_driver.cpp bound to HIP + RCCL
namespace {
int shard_alloc(void *ctx, int i, size_t bytes, void **out, std::string *err)
{
    asx_comm *c = (asx_comm *)ctx;
    DevGuard dg(c->devices[(size_t)i]);
    if (!dg.ok) { *err = "cannot select the device"; return -1; }
    const hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) { *out = nullptr; *err = hipGetErrorString(e); return -1; }
    return 0;
}
void shard_free(void *ctx, int i, void *rec)
{
    asx_comm *c = (asx_comm *)ctx;
    DevGuard dg(c->devices[(size_t)i]);
    (void)hipFree(rec);
}
int shard_run(void *ctx, int i, void *record, size_t width, size_t count, const float *d_src, const float *d_smp, std::string *err)
{
    asx_comm *c = (asx_comm *)ctx;
    asx_plan *p = c->plans[(size_t)i];
    if (hipSetDevice(p->device) != hipSuccess) { *err = "hipSetDevice failed"; return -1; }
    char *base = (char *)record;
    int64_t *lag = (int64_t *)base;
    double *coef = (double *)(base + width * sizeof(int64_t));
    int32_t *ret = (int32_t *)(base + width * (sizeof(int64_t) + sizeof(double)));
    if (hipMemsetAsync(base, 0, asx_shard_record_bytes(width), p->stream) != hipSuccess) { *err = "hipMemsetAsync failed"; return -1; }
    if (count && asx_xcorr_batch_f32_dev(p, d_src, d_smp, count, lag, coef, ret, p->stream) != 0) { *err = asx_last_error(); return -1; }
    return 0;
}
int shard_gather(void *ctx, int n, void *const *records, void *const *gathered, size_t rec, std::string *err)
{
    asx_comm *c = (asx_comm *)ctx;
    const Rccl *R = rccl_load();
    if (!R) { *err = asx_last_error(); return -1; }
    int grc = R->GroupStart();
    for (int i = 0; i < n && grc == 0; i++) {
        asx_plan *p = c->plans[(size_t)i];
        DevGuard dg(p->device);
        grc = R->AllGather(records[i], gathered[i], rec, 0 /* ncclInt8 / ncclChar */, c->comms[(size_t)i], p->stream);
    }
    const int erc = R->GroupEnd();
    if (grc == 0) grc = erc;
    if (grc != 0) { *err = R->GetErrorString(grc); return -1; }
    return 0;
}
int shard_sync(void *ctx, int i, std::string *err)
{
    asx_comm *c = (asx_comm *)ctx;
    asx_plan *p = c->plans[(size_t)i];
    DevGuard dg(p->device);
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) { *err = hipGetErrorString(e); return -1; }
    return 0;
}
AsxShardOps shard_ops(asx_comm *c) { return AsxShardOps{ c, shard_alloc, shard_free, shard_run, shard_gather, shard_sync }; }
} // namespace

extern "C" void asx_comm_destroy(asx_comm *c)
{
    if (!c) return;
    const Rccl *R = g_rccl.handle ? &g_rccl : nullptr;
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (size_t i = 0; i < c->devices.size(); i++) {
        (void)hipSetDevice(c->devices[i]);
        if (i < c->comms.size() && c->comms[i] && R) (void)R->CommDestroy(c->comms[i]);
    }
    (void)hipSetDevice(prev);
    asx_shard_release(shard_ops(c), c->state); // frees by device id: the plans are not touched
    delete c;
}

extern "C" asx_comm *asx_comm_create(asx_plan *const *plans, int nplans)
{
    if (!plans || nplans < 1) { fail("asx_comm_create: bad argument"); return nullptr; }
    for (int i = 0; i < nplans; i++) {
        if (!plans[i] || plans[i]->host.N != plans[0]->host.N) { fail("asx_comm_create: plans must share one sample_len"); return nullptr; }
        for (int j = 0; j < i; j++)
            if (plans[j]->device == plans[i]->device) { fail("asx_comm_create: one plan per device (device %d twice)", plans[i]->device); return nullptr; }
    }
    const Rccl *R = rccl_load();
    if (!R) return nullptr;
    asx_comm *c = new asx_comm();
    c->plans.assign(plans, plans + nplans);
    c->comms.assign((size_t)nplans, nullptr);
    c->devices.resize((size_t)nplans);
    for (int i = 0; i < nplans; i++) c->devices[(size_t)i] = plans[i]->device;
    const int rc = R->CommInitAll(c->comms.data(), nplans, c->devices.data());
    if (rc != 0) {
        fail("ncclCommInitAll over %d device(s) failed: %s", nplans, R->GetErrorString(rc));
        c->comms.assign((size_t)nplans, nullptr);
        asx_comm_destroy(c);
        return nullptr;
    }
    return c;
}

extern "C" int asx_xcorr_batch_multi_dev(asx_comm *c, const float *const *d_source, const float *const *d_sample,
                                         const size_t *counts, size_t width, void *const *d_gathered)
{
    if (!c) return fail("asx_xcorr_batch_multi_dev: bad argument");
    if (!rccl_load()) return -1;
    std::string err;
    if (asx_shard_drive(shard_ops(c), c->state, (int)c->plans.size(), d_source, d_sample, counts, width, d_gathered, &err) != 0)
        return fail("asx_xcorr_batch_multi_dev: %s", err.c_str());
    return 0;
}

// Frames that are exactly float32 cross PCIe as float32 (csrc/host_narrow.h): the conversion runs on the host pool into
// page-locked staging, every finished run of chunks is uploaded while later ones are still being converted.
namespace {
struct NarrowUp {
    hipStream_t s;
    const float *pin;
    float *dev;
    hipError_t err;
};
void narrow_upload(size_t first, size_t count, void *user)
{
    NarrowUp *u = (NarrowUp *)user;
    if (u->err != hipSuccess) return;
    u->err = hipMemcpyAsync(u->dev + first, u->pin + first, count * sizeof(float), hipMemcpyHostToDevice, u->s);
}
bool narrow_enabled()
{
    static const bool on = !(getenv("ASX_NARROW") && atoi(getenv("ASX_NARROW")) == 0); // ASX_NARROW=0: always 8 bytes per frame (A/B)
    return on;
}
// 1: dev[0..n) holds the frames as float32 (enqueued on s); 0: not every frame is a float32 (nothing usable was left); -1: error
int upload_narrowed(hipStream_t s, const double *host, size_t n, float *pin, float *dev)
{
    NarrowUp u{ s, pin, dev, hipSuccess };
    const int exact = asx_narrow_exact(host, pin, n, narrow_upload, &u);
    if (u.err != hipSuccess) return fail("hipMemcpyAsync of narrowed frames failed: %s", hipGetErrorString(u.err));
    return exact;
}
} // namespace

// One pair of asx_xcorr_f64 in the plan's staging buffers: the transforms read the float32 copy, the exact passes tsrc / tsmp
// (the float32 copy itself when the frames were narrowed); the direct Pearson form, see GroupOpts::f32_abi.
template <typename TIn>
static int staged_pair(asx_plan *p, const TIn *tsrc, const TIn *tsmp, const Results &h, hipStream_t s)
{
    const size_t N = p->host.N;
    const Pairs<TIn> x = Pairs<TIn>::staged(p->st.src, p->st.smp, tsrc, tsmp, N);
    const Results d{ p->st.lag, p->st.coef, p->st.ret };
    return run_group(p, x, 1, d, s, { .f32_abi = false }) || fetch_results(p, x, 1, d, h, s) ? -1 : 0;
}

extern "C" int asx_xcorr_f64(asx_plan *p, const double *source, const double *sample, long *lag,
                             double *coefficient)
{
    if (!p || !source || !sample || !lag || !coefficient) return fail("asx_xcorr_f64: null argument");
    PlanCall c(p);
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    if (ensure_staging(p, true)) return -1;
    const size_t N = p->host.N;
    hipStream_t s = c.s;
    prof_begin_call(p);
    // What ffmpeg decodes from 16-bit or float audio is exactly representable in float32 (src/capture/linux_capture.c:370
    // asks for f64le all the same): then 4 bytes per frame cross PCIe, and the float64 passes (exact re-evaluation, Pearson)
    // read the float32 copy widened in registers -- the same values, the same operations, the same bits.
    int narrow = 0;
    if (narrow_enabled()) {
        if (!p->pin32) {
            void *pin = nullptr;
            if (hipHostMalloc(&pin, 3 * N * sizeof(float), hipHostMallocDefault) == hipSuccess) p->pin32 = (float *)pin;
            else (void)hipGetLastError(); // no staging: the 8-byte path below
        }
        if (p->pin32) {
            narrow = upload_narrowed(s, source, 2 * N, p->pin32, p->st.src);
            if (narrow == 1) narrow = upload_narrowed(s, sample, N, p->pin32 + 2 * N, p->st.smp);
            if (narrow < 0) return -1;
        }
    }
    int64_t h_lag = 0;
    double h_coef = 0;
    int32_t h_ret = -1;
    const Results h{ &h_lag, &h_coef, &h_ret };
    if (narrow == 1) {
        p->narrowed++;
        if (staged_pair(p, p->st.src, p->st.smp, h, s)) return -1;
    } else {
        HIP_TRY(hipMemcpyAsync(p->st64.src, source, 2 * N * sizeof(double), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(p->st64.smp, sample, N * sizeof(double), hipMemcpyHostToDevice, s));
        asx_launch_cvt_f64_f32(p->st64.src, p->st.src, 2 * N, s);
        asx_launch_cvt_f64_f32(p->st64.smp, p->st.smp, N, s);
        if (staged_pair(p, p->st64.src, p->st64.smp, h, s)) return -1;
    }
    *lag = (long)h_lag;
    *coefficient = h_coef;
    return h_ret;
}

// pearson_coefficient() is called on its own by the reference's tests and may be called often: its
// device buffers are kept per device and only ever grow (the reference allocates nothing here).
struct PearsonScratch {
    std::mutex lock;
    size_t cap = 0;              // doubles per array
    double *a = nullptr, *b = nullptr;
    struct Fixed { double *ps = nullptr, *c = nullptr; AsxSeg *seg = nullptr; } f;
    AsxMemSet ab{ hip_mem }, fixed{ hip_mem }; // a / b: replaced on growth; the rest: whole or absent
    hipStream_t stream = nullptr;
};
static std::mutex g_pearson_lock;
static std::vector<PearsonScratch *> g_pearson; // by device id, created on first use, kept for the life of the process

extern "C" int asx_pearson_f64(const double *a, const double *b, size_t n, int device, double *out)
{
    if (!a || !b || !out) return fail("asx_pearson_f64: null argument");
    if (n > 0xFFFFFFFFull) return fail("asx_pearson_f64: range too long");
    const int ndev = asx_device_count();
    if (ndev == 0) return fail("no usable HIP device; this library has no CPU fallback");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail("asx_pearson_f64: device %d out of range (%d devices)", device, ndev);
    DevGuard dg(device);
    if (!dg.ok) return fail("cannot select device %d", device);
    PearsonScratch *Sp = nullptr;
    {
        std::lock_guard<std::mutex> g(g_pearson_lock);
        if (g_pearson.size() <= (size_t)device) g_pearson.resize((size_t)device + 1, nullptr);
        if (!g_pearson[(size_t)device]) g_pearson[(size_t)device] = new PearsonScratch();
        Sp = g_pearson[(size_t)device];
    }
    PearsonScratch &S = *Sp;
    std::lock_guard<std::mutex> guard(S.lock);
    if (!S.stream) {
        if (!S.f.ps && asx_mem_whole(S.fixed, S.f, [](AsxMemSet &m, PearsonScratch::Fixed &T) {
                return m.take(&T.ps, ASX_PEARSON_BLOCKS_MAX * 6) || m.take(&T.c, 1) || m.take(&T.seg, 1);
            }))
            return fail("asx_pearson_f64: scratch allocation failed: %s", hipGetErrorString(g_take_err));
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess)
            return fail("asx_pearson_f64: scratch allocation failed: %s", hipGetErrorString(hipGetLastError()));
        S.stream = st;
    }
    if (n > S.cap) {
        S.ab.clear();
        S.a = S.b = nullptr; S.cap = 0;
        const size_t want = std::max<size_t>(n, 4096);
        AsxMemSet grown(hip_mem);
        double *na = nullptr, *nb = nullptr;
        if (grown.take(&na, want) || grown.take(&nb, want)) return fail("asx_pearson_f64: hipMalloc failed: %s", hipGetErrorString(g_take_err));
        S.ab.swap(grown);
        S.a = na; S.b = nb; S.cap = want;
    }
    AsxSeg seg{};
    seg.lag = 0; seg.src_off = 0; seg.smp_off = 0; seg.len = (uint32_t)n; seg.peak = 0;
    HIP_TRY(hipMemcpyAsync(S.a, a, n * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIP_TRY(hipMemcpyAsync(S.b, b, n * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIP_TRY(hipMemcpyAsync(S.f.seg, &seg, sizeof(seg), hipMemcpyHostToDevice, S.stream));
    asx_launch_pearson(AsxInputs<double>{ S.a, S.b, 0, 0, nullptr }, (uint32_t)n, S.f.seg, S.f.ps, nullptr, S.f.c, nullptr, 1, S.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, S.f.c, sizeof(double), hipMemcpyDeviceToHost, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    return 0;
}

// ---------------------------------------------------------------------------
// result consumers
// ---------------------------------------------------------------------------
extern "C" int asx_results_to_ms_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret, size_t batch,
                                     double min_confidence, double sample_rate, int64_t *d_lag_ms,
                                     int32_t *d_accept, void *stream)
{
    if (!d_lag || !d_coef || !d_ret || !d_lag_ms) return fail("asx_results_to_ms_dev: null argument");
    if (!(sample_rate > 0.0)) return fail("asx_results_to_ms_dev: bad sample rate");
    asx_launch_results_to_ms(d_lag, d_coef, d_ret, batch, min_confidence, sample_rate, d_lag_ms, d_accept,
                             (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The entry of each pair a caller of the top-k calls keeps (k_topk_best): one launch on `stream`, nothing allocated.
extern "C" int asx_topk_best_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret, size_t batch, int k,
                                 int64_t *d_best_lag, double *d_best_coef, int32_t *d_best_ret, int32_t *d_best_entry, void *stream)
{
    if (!d_lag || !d_coef || !d_ret || !d_best_coef || !d_best_ret) return fail("asx_topk_best_dev: null argument");
    if (k < 1 || k > ASX_TOPK_MAX) return fail("asx_topk_best_dev: k = %d is not in [1, %d]", k, ASX_TOPK_MAX);
    asx_launch_topk_best(d_lag, d_coef, d_ret, batch, k, d_best_lag, d_best_coef, d_best_ret, d_best_entry, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Each pair's entry by triangle closure over one pool's all-pairs tables, and the clips' offsets from the picks (k_closure_votes,
// k_closure_confirm, k_closure_root, k_closure_offsets): four launches on `stream`, nothing allocated, no workspace -- every kernel
// reads required outputs of those before it.
static_assert(ASX_CLOSURE_LAG_MAX == ASX_CLOSURE_LAG_LIMIT, "the header's limit of a valid lag and the kernels' copy of it differ");
extern "C" int asx_pool_closure_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret, size_t nclips, int k,
                                    int64_t tolerance, int min_confirm, int root, int32_t *d_votes, int64_t *d_best_lag,
                                    double *d_best_coef, int32_t *d_best_ret, int32_t *d_best_entry, int32_t *d_confirm,
                                    int32_t *d_root, int64_t *d_offset, int32_t *d_support, int32_t *d_placed, void *stream)
{
    if (!d_lag || !d_coef || !d_ret || !d_best_lag || !d_best_coef || !d_best_ret || !d_best_entry || !d_confirm || !d_root ||
        !d_offset || !d_support || !d_placed)
        return fail("asx_pool_closure_dev: null argument");
    if (k < 1 || k > ASX_TOPK_MAX) return fail("asx_pool_closure_dev: k = %d is not in [1, %d]", k, ASX_TOPK_MAX);
    if (nclips == 0) return fail("asx_pool_closure_dev: no clips");
    // (nclips > 65535 first: it is what keeps the 64-bit product below from wrapping, at nclips = 2^33 for instance)
    if (nclips > 65535 || (uint64_t)nclips * nclips * (uint64_t)k > (uint64_t)INT32_MAX)
        return fail("asx_pool_closure_dev: %zu clips with k = %d are more than INT32_MAX entries", nclips, k);
    if (tolerance < 0 || tolerance > ASX_CLOSURE_LAG_MAX)
        return fail("asx_pool_closure_dev: tolerance = %lld is not in [0, 2^40]", (long long)tolerance);
    if (min_confirm < 0) return fail("asx_pool_closure_dev: min_confirm = %d is negative", min_confirm);
    if (root < -1 || (root >= 0 && (size_t)root >= nclips))
        return fail("asx_pool_closure_dev: root = %d is neither -1 nor one of the %zu clips", root, nclips);
    asx_launch_pool_closure(d_lag, d_coef, d_ret, (uint32_t)nclips, k, tolerance, min_confirm, root, d_votes, d_best_lag, d_best_coef,
                            d_best_ret, d_best_entry, d_confirm, d_root, d_offset, d_support, d_placed, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Every clip that a chain of usable pairs reaches from the root, and a verdict per pair, from closure's picked tables (k_place_init,
// k_place_layer, k_place_sweep, k_place_verdict: place.hip): 2 + max_hops + sweeps launches on `stream`, nothing allocated; the root
// is read on the device.
extern "C" int asx_pool_place_dev(const int64_t *d_lag, const int32_t *d_ret, const int32_t *d_confirm, size_t nclips,
                                  int64_t tolerance, int min_confirm, const int32_t *d_root, int max_hops, int sweeps,
                                  int64_t *d_scratch, int64_t *d_offset, int32_t *d_hops, int32_t *d_support, int32_t *d_degree,
                                  int64_t *d_step, int64_t *d_resid, int32_t *d_state, void *stream)
{
    if (!d_lag || !d_ret || !d_confirm || !d_root || !d_offset || !d_hops || !d_support || !d_degree || !d_step || !d_resid || !d_state)
        return fail("asx_pool_place_dev: null argument");
    if (nclips == 0) return fail("asx_pool_place_dev: no clips");
    if (nclips > 65535 || (uint64_t)nclips * nclips > (uint64_t)INT32_MAX)
        return fail("asx_pool_place_dev: %zu clips are more than INT32_MAX pairs", nclips);
    if (tolerance < 0 || tolerance > ASX_CLOSURE_LAG_MAX)
        return fail("asx_pool_place_dev: tolerance = %lld is not in [0, 2^40]", (long long)tolerance);
    if (min_confirm < 0) return fail("asx_pool_place_dev: min_confirm = %d is negative", min_confirm);
    if (max_hops < 1 || max_hops > ASX_PLACE_HOPS_MAX)
        return fail("asx_pool_place_dev: max_hops = %d is not in [1, %d]", max_hops, ASX_PLACE_HOPS_MAX);
    if (sweeps < 0 || sweeps > ASX_PLACE_SWEEPS_MAX)
        return fail("asx_pool_place_dev: sweeps = %d is not in [0, %d]", sweeps, ASX_PLACE_SWEEPS_MAX);
    if (sweeps > 0 && !d_scratch) return fail("asx_pool_place_dev: sweeps = %d need d_scratch", sweeps);
    asx_launch_pool_place(d_lag, d_ret, d_confirm, (uint32_t)nclips, tolerance, min_confirm, d_root, max_hops, sweeps, d_scratch,
                          d_offset, d_hops, d_support, d_degree, d_step, d_resid, d_state, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// growing-window streams (BASELINE config 5)
// ---------------------------------------------------------------------------
struct asx_stream {
    int device = 0;
    size_t cap = 0;                 // max sample frames (source capacity = 2*cap)
    size_t n_src = 0, n_smp = 0;    // frames resident
    asx_plan::Staging f32;          // the tracks as float32, one result
    asx_plan::Staging64 f64;        // the tracks as they came
    AsxMemSet mem{ hip_mem };       // the seven buffers of the two
    std::vector<asx_plan *> plans;  // one per prefix length seen
    int64_t win_lo = INT64_MIN, win_hi = INT64_MAX; // asx_stream_set_lag_window, in frames: clamped to [-n, n-1] per prefix length n
    hipStream_t s = nullptr;        // uploads and conversions of new frames
    std::mutex lock;
};

extern "C" void asx_stream_destroy(asx_stream *st)
{
    if (!st) return;
    DevGuard dg(st->device); // (until the stream's set has given its buffers back)
    for (asx_plan *p : st->plans) asx_plan_destroy(p);
    if (st->s) { (void)hipStreamSynchronize(st->s); (void)hipStreamDestroy(st->s); }
    delete st;
}

extern "C" asx_stream *asx_stream_create(size_t max_sample_len, int device)
{
    if (max_sample_len == 0) { fail("asx_stream_create: max_sample_len must be > 0"); return nullptr; }
    if (asx_device_count() == 0) { fail("no usable HIP device; this library has no CPU fallback"); return nullptr; }
    if (device < 0) HIP_TRY_NULL(hipGetDevice(&device));
    DevGuard dg(device);
    if (!dg.ok) { fail("cannot select device %d", device); return nullptr; }
    asx_stream *st = new asx_stream();
    st->device = device;
    st->cap = max_sample_len;
    const size_t n = max_sample_len;
    AsxMemSet &m = st->mem;
    const bool took = !(m.take(&st->f64.src, 2 * n) || m.take(&st->f64.smp, n) || m.take(&st->f32.src, 2 * n) || m.take(&st->f32.smp, n) ||
                        m.take(&st->f32.lag, 1) || m.take(&st->f32.coef, 1) || m.take(&st->f32.ret, 1));
    if (!took || hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking) != hipSuccess) {
        fail("asx_stream_create: hipMalloc failed: %s", hipGetErrorString(took ? hipGetLastError() : g_take_err));
        asx_stream_destroy(st);
        return nullptr;
    }
    return st;
}

extern "C" int asx_stream_lengths(const asx_stream *st, size_t *n_source, size_t *n_sample)
{
    if (!st) return -1;
    if (n_source) *n_source = st->n_src;
    if (n_sample) *n_sample = st->n_smp;
    return 0;
}

extern "C" int asx_stream_reset(asx_stream *st)
{
    if (!st) return -1;
    std::lock_guard<std::mutex> guard(st->lock);
    st->n_src = st->n_smp = 0;
    return 0;
}

extern "C" int asx_stream_append_f64(asx_stream *st, const double *source_frames, size_t n_source,
                                     const double *sample_frames, size_t n_sample)
{
    if (!st || (n_source && !source_frames) || (n_sample && !sample_frames))
        return fail("asx_stream_append_f64: null argument");
    std::lock_guard<std::mutex> guard(st->lock);
    if (st->n_src + n_source > 2 * st->cap || st->n_smp + n_sample > st->cap)
        return fail("asx_stream_append_f64: capacity exceeded");
    DevGuard dg(st->device);
    if (!dg.ok) return fail("cannot select device %d", st->device);
    // Both tracks' new frames go up on the stream's own HIP stream -- from page-locked memory (asx_host_malloc) by DMA,
    // both copies and both conversions in flight together -- and one synchronisation orders them before the plans'
    // streams, which only start after this function has returned.
    // (No float32 narrowing here, unlike asx_xcorr_f64: the frames come from page-locked memory and go by DMA as they are;
    //  a CPU pass over them to save PCIe bytes measured SLOWER, 1.98 against 1.76 ms for the six intervals.)
    if (n_source) {
        HIP_TRY(hipMemcpyAsync(st->f64.src + st->n_src, source_frames, n_source * sizeof(double), hipMemcpyHostToDevice, st->s));
        asx_launch_cvt_f64_f32(st->f64.src + st->n_src, st->f32.src + st->n_src, n_source, st->s);
    }
    if (n_sample) {
        HIP_TRY(hipMemcpyAsync(st->f64.smp + st->n_smp, sample_frames, n_sample * sizeof(double), hipMemcpyHostToDevice, st->s));
        asx_launch_cvt_f64_f32(st->f64.smp + st->n_smp, st->f32.smp + st->n_smp, n_sample, st->s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st->s));
    st->n_src += n_source;
    st->n_smp += n_sample;
    return 0;
}

extern "C" int asx_stream_set_lag_window(asx_stream *st, int64_t lag_min, int64_t lag_max)
{
    if (!st) return fail("asx_stream_set_lag_window: null stream");
    if (lag_min > lag_max) return fail("asx_stream_set_lag_window: lag_min %lld > lag_max %lld", (long long)lag_min, (long long)lag_max);
    std::lock_guard<std::mutex> guard(st->lock);
    st->win_lo = lag_min;
    st->win_hi = lag_max;
    return 0;
}

extern "C" int asx_stream_xcorr(asx_stream *st, size_t sample_len, long *lag, double *coefficient)
{
    if (!st || !lag || !coefficient || sample_len == 0) return fail("asx_stream_xcorr: bad argument");
    std::lock_guard<std::mutex> guard(st->lock);
    if (st->n_smp < sample_len || st->n_src < 2 * sample_len)
        return fail("asx_stream_xcorr: only %zu/%zu frames resident, %zu/%zu needed", st->n_src, st->n_smp,
                    2 * sample_len, sample_len);
    asx_plan *p = nullptr;
    for (asx_plan *q : st->plans)
        if (q->host.N == sample_len) p = q;
    if (!p) {
        p = asx_plan_create(sample_len, 1, st->device);
        if (!p) return -1;
        st->plans.push_back(p);
    }
    PlanCall c(p); // (the plan was made on the stream's device)
    if (!c.dg.ok) return fail("cannot select device %d", p->device);
    // the stream's window on this prefix length (both ends clamped to [-n, n-1]: lo <= hi stays true)
    const int64_t n = (int64_t)sample_len;
    p->win_lo = std::min(std::max(st->win_lo, -n), n - 1);
    p->win_hi = std::min(std::max(st->win_hi, -n), n - 1);
    prof_begin_call(p);
    int64_t h_lag = 0;
    double h_coef = 0;
    int32_t h_ret = -1;
    const Pairs<double> x = Pairs<double>::staged(st->f32.src, st->f32.smp, st->f64.src, st->f64.smp, sample_len);
    const Results d{ st->f32.lag, st->f32.coef, st->f32.ret };
    if (run_group(p, x, 1, d, c.s) || fetch_results(p, x, 1, d, { &h_lag, &h_coef, &h_ret }, c.s)) return -1;
    *lag = (long)h_lag;
    *coefficient = h_coef;
    return h_ret;
}

// ---------------------------------------------------------------------------
// synthetic inputs, timing, raw memory helpers
// ---------------------------------------------------------------------------
extern "C" int asx_synth_pairs_dev(uint64_t seed, uint64_t first_pair, size_t count, size_t sample_len,
                                   int noise_shift, float *d_source, float *d_sample,
                                   int64_t *d_true_lag, void *stream)
{
    if (!d_source || !d_sample) return fail("asx_synth_pairs_dev: null argument");
    if (sample_len == 0 || sample_len > (1u << 30)) return fail("asx_synth_pairs_dev: bad sample_len");
    for (size_t done = 0; done < count; done += 32768) {
        const size_t c = std::min((size_t)32768, count - done);
        asx_launch_synth(seed, first_pair + done, c, (uint32_t)sample_len, noise_shift,
                         d_source + done * 2 * sample_len, d_sample + done * sample_len,
                         d_true_lag ? d_true_lag + done : nullptr, (hipStream_t)stream);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int asx_plan_set_profiling(asx_plan *p, int depth)
{
    if (!p) return -1;
    std::lock_guard<std::mutex> guard(p->lock);
    p->profiling = depth > 0;
    p->prof_depth = depth > 0 ? (size_t)depth : 1;
    p->prof_calls = 0;
    p->prof_groups.assign(p->prof_depth, 0);
    if (p->evr.size() < p->prof_depth) p->evr.resize(p->prof_depth);
    p->ev_groups = 0;
    return 0;
}

// timings of the batch call `calls_back` calls ago (0 = the latest) of the profiling ring
extern "C" int asx_plan_timings_ms(asx_plan *p, int calls_back, float out[6])
{
    if (!p || !out) return -1;
    std::lock_guard<std::mutex> guard(p->lock);
    for (int i = 0; i < 6; i++) out[i] = 0.f;
    if (!p->profiling || calls_back < 0 || (size_t)calls_back >= p->prof_depth || (size_t)calls_back >= p->prof_calls)
        return fail("no profiled call recorded %d calls back", calls_back);
    const size_t ring = (p->prof_calls - 1 - (size_t)calls_back) % p->prof_depth;
    const size_t groups = p->prof_groups[ring];
    if (groups == 0) return fail("no profiled call recorded");
    if (p->evr.size() <= ring || p->evr[ring].size() < groups * 6) return fail("no profiled call recorded");
    const hipEvent_t *ev = p->evr[ring].data();
    DevGuard dg(p->device);
    for (size_t g = 0; g < groups; g++) {
        HIP_TRY(hipEventSynchronize(ev[g * 6 + 5]));
        for (int k = 0; k < 5; k++) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[g * 6 + k], ev[g * 6 + k + 1]));
            out[k] += ms;
        }
    }
    float total = 0.f;
    HIP_TRY(hipEventElapsedTime(&total, ev[0], ev[(groups - 1) * 6 + 5]));
    out[5] = total;
    return 0;
}

extern "C" int asx_plan_last_timings_ms(asx_plan *p, float out[6]) { return asx_plan_timings_ms(p, 0, out); }

extern "C" void *asx_device_malloc(size_t bytes, int device)
{
    int prev = 0;
    if (device >= 0) {
        HIP_TRY_NULL(hipGetDevice(&prev));
        HIP_TRY_NULL(hipSetDevice(device));
    }
    void *ptr = nullptr;
    hipError_t e = hipMalloc(&ptr, bytes ? bytes : 1);
    if (device >= 0) (void)hipSetDevice(prev);
    if (e != hipSuccess) {
        fail("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return ptr;
}

extern "C" int asx_device_free(void *ptr)
{
    HIP_TRY(hipFree(ptr));
    return 0;
}

extern "C" void *asx_host_malloc(size_t bytes)
{
    void *ptr = nullptr;
    hipError_t e = hipHostMalloc(&ptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        fail("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return ptr;
}

extern "C" int asx_host_free(void *ptr)
{
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return 0;
}

extern "C" int asx_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int asx_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int asx_stream_sync(asx_plan *p, void *stream)
{
    if (!p) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return 0;
    }
    PlanCall c(p, stream, false);
    HIP_TRY(hipStreamSynchronize(c.s));
    return 0;
}

// ---------------------------------------------------------------------------
// planning arithmetic exposed for the CPU test-suite (no HIP calls)
// ---------------------------------------------------------------------------
// the kernels the plan of (sample_len, split) would run under the current environment (AsxKernelChoice): out = {real-column,
// entry of the column list, of the row list, block size of the packed column kernels, of the row kernels, band_rows, prunable};
// cols / rows: the two entries spelled out (asx_kernel_table_spell), ASX_KERNEL_ENTRY_CAP ints each
static void choice_out(const AsxKernelChoice &k, int *out, int *cols, int *rows)
{
    const int v[7] = { k.rlayout, k.cols, k.rows, k.threads_cols, k.threads_rows, k.band_rows, k.prunable };
    memcpy(out, v, sizeof v);
    asx_kernel_table_spell(k.rlayout ? 0 : 2, k.cols, cols);
    asx_kernel_table_spell(k.rlayout ? 1 : 3, k.rows, rows);
}
// entry `index` of list 0 .. 3 of kernel_table.h (AsxRCols, AsxRRows, AsxPCols, AsxPRows) into out; 1: the list ends before it
extern "C" int asx_planmath_kernel_table(int list, int index, int *out)
{
    if (!out) return fail("asx_planmath_kernel_table: null argument");
    return asx_kernel_table_spell(list, index, out) ? 0 : 1;
}
extern "C" int asx_planmath_kernels(size_t sample_len, const char *split, int *out, int *cols, int *rows)
{
    if (!out || !cols || !rows) return fail("asx_planmath_kernels: null argument");
    AsxHostPlan h;
    std::string err = asx_host_plan_build(sample_len, split, &h);
    if (!err.empty()) return fail("%s", err.c_str());
    choice_out(h.kernels, out, cols, rows);
    return 0;
}
// the same of a live plan: the record it holds
extern "C" int asx_plan_debug_kernels(const asx_plan *p, int *out, int *cols, int *rows)
{
    if (!p || !out || !cols || !rows) return fail("asx_plan_debug_kernels: null argument");
    choice_out(p->host.kernels, out, cols, rows);
    return 0;
}

// asx_group_form of an ask given as ASX_GROUP_ASK_INTS ints (plan_math.h states both orders), into ASX_GROUP_FORM_INTS ints
extern "C" int asx_planmath_group_form(const int *ask, int nask, int *out, int nout)
{
    if (!ask || !out || nask != ASX_GROUP_ASK_INTS || nout != ASX_GROUP_FORM_INTS)
        return fail("asx_planmath_group_form: %d and %d ints, not %d and %d", nask, nout, ASX_GROUP_ASK_INTS, ASX_GROUP_FORM_INTS);
    AsxGroupAsk a;
    a.rlayout = ask[0]; a.plan_prune = ask[1]; a.plan_spectral = ask[2]; a.band_sums = ask[3]; a.over_list = ask[4];
    a.f32_inputs = ask[5]; a.f32_abi = ask[6]; a.listed = ask[7]; a.r_out = ask[8]; a.own_lists = ask[9]; a.k = ask[10];
    a.search = ask[11]; a.weight = (AsxWeight)ask[12]; a.pool = ask[13]; a.bc = ask[14]; a.qstore = ask[15];
    const AsxGroupForm f = asx_group_form(a);
    const int v[ASX_GROUP_FORM_INTS] = { f.fwd, f.rows, f.weight, f.bc, f.pruned, f.tail, f.appends, f.qstore, f.takeback };
    memcpy(out, v, sizeof v);
    return 0;
}

extern "C" int asx_planmath_describe(size_t sample_len, const char *split, uint32_t *F, uint32_t *src_valid,
                                     int *M1, int *M2, int *T, int *nst1, int *radix1, int *nst2,
                                     int *radix2)
{
    AsxHostPlan h;
    std::string err = asx_host_plan_build(sample_len, split, &h);
    if (!err.empty()) return fail("%s", err.c_str());
    *F = h.F; *src_valid = h.src_valid; *M1 = h.M1; *M2 = h.M2; *T = h.T;
    *nst1 = h.st1.nstages; *nst2 = h.st2.nstages;
    for (int i = 0; i < h.st1.nstages; i++) radix1[i] = h.st1.radix[i];
    for (int i = 0; i < h.st2.nstages; i++) radix2[i] = h.st2.radix[i];
    return 0;
}

// candidates of the measured mode, newline-separated "M1xM2xT" strings; returns their number
extern "C" int asx_planmath_candidates(size_t sample_len, size_t max_count, char *out, size_t cap)
{
    const std::vector<std::string> c = asx_host_plan_candidates(sample_len, max_count);
    std::string joined;
    for (const std::string &x : c) { joined += x; joined += '\n'; }
    if (joined.size() + 1 > cap) return fail("candidate list larger than buffer");
    memcpy(out, joined.c_str(), joined.size() + 1);
    return (int)c.size();
}

// tables: which = 0 pos1_of_k1 (M1 ints), 1 k1_of_pos1 (M1), 2 pos2_of_k2 (M2)
extern "C" int asx_planmath_table(size_t sample_len, const char *split, int which, int *out, size_t cap)
{
    AsxHostPlan h;
    std::string err = asx_host_plan_build(sample_len, split, &h);
    if (!err.empty()) return fail("%s", err.c_str());
    const std::vector<int> &t = which == 0 ? h.pos1_of_k1 : which == 1 ? h.k1_of_pos1 : h.pos2_of_k2;
    if (t.size() > cap) return fail("table larger than buffer");
    memcpy(out, t.data(), t.size() * sizeof(int));
    return (int)t.size();
}

// twiddle tables: which = 0 tw1, 1 tw2, 2 tw_lo, 3 tw_hi ; out = interleaved re,im floats
extern "C" int asx_planmath_twiddles(size_t sample_len, const char *split, int which, float *out, size_t cap)
{
    AsxHostPlan h;
    std::string err = asx_host_plan_build(sample_len, split, &h);
    if (!err.empty()) return fail("%s", err.c_str());
    const std::vector<float2> &t =
        which == 0 ? h.tw1 : which == 1 ? h.tw2 : which == 2 ? h.tw_lo : h.tw_hi;
    if (t.size() > cap) return fail("table larger than buffer");
    memcpy(out, t.data(), t.size() * sizeof(float2));
    return (int)t.size();
}
