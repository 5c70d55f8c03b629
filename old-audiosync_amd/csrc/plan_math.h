// csrc/plan_math.h — host-only planning arithmetic (no HIP calls): transform
// length selection, the M = M1*M2 split, radix schedules, twiddle and index
// tables.  Kept separate so the CPU test-suite can exercise it without a GPU
// (tests/test_plan_math.py through the asx_planmath_* C entry points).
#pragma once

#include "asx_internal.h"

#include <string>
#include <vector>

// Which compiled-in kernels a plan's transforms run (kernel_table.h): decided once, by asx_host_plan_build, from the host plan and
// the environment alone.  The launchers look the indices up; nothing matches a schedule again.
struct AsxKernelChoice {
    bool rlayout = false;               // the real-column kernels (rlayout.hip); else the packed-sample kernels (xcorr_kernels.hip)
    int cols = -1, rows = -1;           // entry of AsxRCols / AsxRRows, or of AsxPCols / AsxPRows; -1 (packed only): run-time schedule
    int threads_cols = 0, threads_rows = 0; // block sizes of the packed kernels ($ASX_THREADS_COLS / _ROWS override them)
    int band_rows = 0;                  // real-column: rows of the [2 M1][M2] sample matrix one lane group of k_fwd_cols_r loads
    bool prunable = false;              // real-column: the pruned inverse pass can run on this plan
};

struct AsxHostPlan {
    size_t N = 0;
    uint32_t F = 0, M = 0, src_valid = 0;
    int M1 = 0, M2 = 0, T = 0, logT = 0, ntiles = 0;
    AsxStages st1{}, st2{};
    std::vector<float2> tw1, tw2, tw2s, tw_lo, tw_hi;
    std::vector<int> k1_of_pos1, pos1_of_k1, pos2_of_k2;
    std::vector<int4> row_tasks;
    // real-column decomposition (rlayout.hip): possible when M1 is even, the length is not embedded and tiles are whole
    bool rlayout = false;
    std::vector<int4> col_pairs;    // [M1/2 + 1] {u, slot of u, slot of M1 - u, 0}, ordered by the slot of u
    std::vector<float2> col_tw;     // w_{2 M1}^u in the same order
    AsxKernelChoice kernels;
};

// LDS budgets that bound the split (bytes per workgroup).
constexpr size_t ASX_LDS_COLS_MAX = 80 * 1024;  // M1 * T * 8  (two blocks per CU)
constexpr size_t ASX_LDS_ROWS_MAX = 64 * 1024;  // 4 * M2 * 8
constexpr size_t ASX_LDS_HW_MAX = 160 * 1024;   // what one gfx950 workgroup may declare (overrides only)

bool asx_is_smooth(uint64_t n);                 // only factors 2, 3, 5
uint64_t asx_next_smooth_even(uint64_t n);
// Fills *plan for sample_len N. `split_override` may be "" or "M1xM2xT".  Reads $ASX_LAYOUT (packed: never the real-column
// kernels), $ASX_GENERIC (packed, and never a compiled-in schedule), $ASX_THREADS_COLS / _ROWS and $ASX_STAGE_ORDER.
// Returns "" on success, else an error message.
std::string asx_host_plan_build(size_t N, const char *split_override, AsxHostPlan *plan);
// The `max_count` cheapest splits of sample_len N by the planner's cost model, every feasible tile
// width included ("M1xM2xT" strings, cheapest first): the candidates of the measured mode
// (asx_plan_create_ex(..., "measure") times them on the device and keeps the fastest).
std::vector<std::string> asx_host_plan_candidates(size_t N, size_t max_count);
bool asx_make_stages(int n, AsxStages *st);
std::vector<int> asx_position_table(const AsxStages &st); // pos[k] = slot of X[k] after the DIF transform
// Entry `index` of a list of kernel_table.h spelled out for the diagnostics (asx_entry_spell: at most ASX_ENTRY_INTS ints) -- list 0
// AsxRCols, 1 AsxRRows, 2 AsxPCols, 3 AsxPRows; false, and a first int of -1: the list has no such entry
bool asx_kernel_table_spell(int list, int index, int *out);
constexpr int ASX_KERNEL_ENTRY_CAP = 32; // ints per entry a caller of the diagnostic exports provides (hipxcorr.py: KERNEL_ENTRY_CAP)

// The form of a launch group: what run_group (asx_api.hip) launches for it, decided once from values alone ("The form
// of a launch group"; tabled without a device by tests/test_group_form.py through asx_planmath_group_form).
// The ask: what run_group knows before it launches anything.
struct AsxGroupAsk {
    // the plan
    bool rlayout = false;        // a real-column plan (else packed)
    bool plan_prune = false;     // asx_plan_set_prune
    bool plan_spectral = false;  // asx_plan_set_pearson
    bool band_sums = false;      // the peak workspace in use has band sums (AsxPeakWs::band)
    bool over_list = false;      // ... and an overflow list (AsxPeakWs::over_list)
    // the call
    bool f32_inputs = false;     // the exact passes read float32 (TIn)
    bool f32_abi = false;        // GroupOpts::f32_abi
    bool listed = false;         // GroupOpts::listed
    bool r_out = false;          // r of every lag is asked for
    bool own_lists = false;      // the group runs on lists of its own (GroupOpts::pk: the second look)
    int k = 1;                   // top-k passes
    int search = AsxSearch::ALL; // pass 1's AsxSearch::Kind
    AsxWeight weight = ASX_W_NONE;
    bool pool = false;           // a pool group
    int bc = 0;                  // broadcast operands (bit 0: source, bit 1: sample)
    bool qstore = false;         // GroupOpts::qstore
};
enum AsxFwdForm { ASX_FWD_POOL, ASX_FWD_REAL, ASX_FWD_PACKED }; // pool resolve; k_fwd_cols_r (+ k_bcast_aux per bit of bc); k_fwd_cols
enum AsxTail { ASX_TAIL_PHAT, ASX_TAIL_DIRECT, ASX_TAIL_SPECTRAL };
struct AsxGroupForm {
    AsxFwdForm fwd;
    AsxRowFlavour rows;
    AsxWeight weight;            // beside the row flavour: PHAT and pruning exclude each other
    int bc;                      // the form of the plain row flavour
    bool pruned;                 // the pruned pair of passes in place of the inverse column pass (rows == ASX_ROWS_ENERGY on a real-column plan)
    AsxTail tail;
    bool appends;                // k_finalize may append to the overflow list
    // Partial storing of Q may be asked for: asx_qstore_rows, which asks the device, then says how many predictor rows -- more than
    // none: k_rows_rm in place of k_rows_re, and k_qstore_takeback behind the Pearson kernels when `takeback`
    bool qstore;
    bool takeback;
};
AsxGroupForm asx_group_form(const AsxGroupAsk &a);
// the diagnostic export's arrays: the ask's fields in the order above as ints, and {fwd, rows, weight, bc, pruned, tail, appends,
// qstore, takeback}
constexpr int ASX_GROUP_ASK_INTS = 16, ASX_GROUP_FORM_INTS = 9;
