/* include/audiosync/xcorr_hip.h — the C-ABI of the MI355X (gfx950) layer.
 *
 * This is the drop-in boundary for ONE path of vidify/old-audiosync: the FFT
 * cross-correlation of src/cross_correlation.c.  Plain C, plain pointers and
 * sizes; no C++/torch types.  The library behind it (libaudiosync_hip.so) is
 * hand-written HIP for gfx950 and has no CPU fallback: every entry point
 * fails (-1 / NULL, message in asx_last_error()) when no HIP device works.
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *
 *   asx_xcorr_f64            the body of cross_correlation()
 *                            src/cross_correlation.c:133-307, called from
 *                            src/audiosync.c:246 and tests/test_cross_correlation.c:25..109.
 *                            include/audiosync/cross_correlation.h:24-25 is the signature
 *                            the host-side wrapper (host/cross_correlation.c) keeps.
 *   asx_pearson_f64          pearson_coefficient(), src/cross_correlation.c:74-116,
 *                            include/audiosync/cross_correlation.h:10-11
 *   asx_plan_create/destroy  the per-call fftw_plan_dft_r2c_1d / _c2r_1d / fftw_alloc_*
 *                            / fftw_free of src/cross_correlation.c:33-36,159,187-201,
 *                            237-239,300-304, hoisted into a reusable object
 *   asx_xcorr_batch_f32      many independent cross_correlation() calls on float32 data
 *   asx_xcorr_batch_f32_dev  (BASELINE.json north_star: batched many-pair variant);
 *                            no reference equivalent beyond a loop over :133-307
 *   asx_synth_pairs_dev      synthetic 48 kHz mono float32 pairs for benchmarks
 *                            (stands in for the producers src/ffmpeg_pipe.c:68-81)
 *
 * Return convention everywhere: 0 = ok, -1 = error (asx_last_error() says why).
 * Per-pair result convention (the reference's, src/cross_correlation.c:140,276,298):
 *   ret[i] = 0 on success, -1 when the Pearson coefficient is NaN (lag[i] and
 *   coef[i] are still written, exactly as the reference leaves them).
 *   ret[i] = -2 (asx_xcorr_windowed_f32_dev, and asx_xcorr_phat_f32_dev with rows): pair i's lag
 *   window was not a window inside [-N, N-1]; lag[i] = 0 and coef[i] = NaN.  (asx_xcorr_curve_f32_dev and
 *   asx_xcorr_pool_curve_f32_dev: an entry's centre was not a lag inside [-N, N-1]; NaN in all its values.  The same in
 *   asx_xcorr_track_f32_dev and asx_xcorr_pool_track_f32_dev, with used = 0.  asx_xcorr_ncc_f32_dev with rows: the row was not a
 *   window inside [0, N-1]; peak[i] = NaN too.  The same in asx_xcorr_ncc_topk_f32_dev, asx_xcorr_pool_ncc_f32_dev and
 *   asx_xcorr_pool_ncc_topk_f32_dev, in all k entries.  asx_xcorr_ncc_full_f32_dev, asx_xcorr_ncc_full_topk_f32_dev and their pool
 *   forms asx_xcorr_pool_ncc_full_f32_dev and asx_xcorr_pool_ncc_full_topk_f32_dev: the row was not a window inside [-(N-1), N-1].)
 *   ret = -3 (asx_xcorr_topk_f32_dev, asx_xcorr_pool_topk_f32_dev, asx_xcorr_phat_topk_f32_dev and
 *   asx_xcorr_pool_phat_topk_f32_dev only): no lag is left for
 *   this entry of the pair (its window minus the zones around the earlier entries is empty);
 *   lag = 0 and coef = NaN.  (asx_xcorr_ncc_topk_f32_dev, asx_xcorr_pool_ncc_topk_f32_dev, asx_xcorr_ncc_full_topk_f32_dev and
 *   asx_xcorr_pool_ncc_full_topk_f32_dev too: peak = NaN as well.)
 *   ret = -4 (asx_xcorr_pool_f32_dev, asx_xcorr_pool_topk_f32_dev, asx_xcorr_pool_phat_f32_dev,
 *   asx_xcorr_pool_phat_sub_f32_dev and asx_xcorr_pool_phat_topk_f32_dev only): a pair's source or sample index is outside its pool; lag = 0 and coef = NaN (the top-k
 *   form: in all k entries of the pair).  It takes precedence over -2 and -3.  (asx_xcorr_pool_curve_f32_dev: NaN in all
 *   the values of the pair's entries.  asx_xcorr_pool_track_f32_dev: the same, with used = 0.  asx_xcorr_pool_ncc_f32_dev,
 *   asx_xcorr_pool_ncc_topk_f32_dev, asx_xcorr_pool_ncc_full_f32_dev and asx_xcorr_pool_ncc_full_topk_f32_dev: lag = 0, coef = NaN
 *   and peak = NaN, in all k entries.)
 *   ret = -5 (asx_xcorr_warp_f32_dev and asx_xcorr_pool_warp_f32_dev only): an entry's drift line is not valid; NaN in all its
 *   values and len = 0.  In these two calls -4 and -2 mean what they mean in the calls around given lags and take precedence, in
 *   that order.  (asx_xcorr_ncc_ragged_f32_dev and asx_xcorr_ncc_ragged_topk_f32_dev: a pair's row of lengths is not valid; lag = 0,
 *   coef = NaN and peak = NaN in all k entries.  There it takes precedence over -2 and -3, which mean what they mean in
 *   asx_xcorr_ncc_full_f32_dev.)
 */
#ifndef AUDIOSYNC_XCORR_HIP_H
#define AUDIOSYNC_XCORR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct asx_plan asx_plan;

/* ---- library / device ------------------------------------------------- */

/* Number of usable HIP devices (0 when there is none or the runtime fails). */
int asx_device_count(void);
/* The calling thread's current HIP device (-1 when the runtime fails): what device < 0 means below. */
int asx_current_device(void);
/* Last error message of the calling thread ("" if none). Never NULL. */
const char *asx_last_error(void);
/* ABI version of this header (bumped on any signature change). */
int asx_abi_version(void);

/* ---- plans ------------------------------------------------------------ */

/* A plan fixes sample_len (N frames; source is 2N frames) and owns twiddle
 * tables, index tables and HBM workspaces for up to `max_batch` pairs per
 * launch group (larger batches are processed in groups).  device < 0 means
 * "the current HIP device".  Returns NULL on error.
 * Supported N: any N >= 1 whose transform length splits into two factors that
 * fit the LDS kernels (N up to about 4,000,000).  Lengths 2N that are not
 * {2,3,5}-smooth are embedded in a longer smooth transform (same r[k]). */
asx_plan *asx_plan_create(size_t sample_len, size_t max_batch, int device);
/* Same, with the transform split chosen by the caller: "M1xM2xT" (M1*M2 = F/2, T = tile
 * columns, a power of two <= 64) forces it; "measure" times the planner's best candidates
 * on the device (synthetic pairs, a fraction of a second) and keeps the fastest -- what
 * FFTW_MEASURE is to the FFTW_ESTIMATE of src/cross_correlation.c:187-201; NULL, "" or
 * "auto" = the planner's cost model (tuned table for the reference's six lengths).
 * $ASX_SPLIT supplies the value when the argument is NULL or "". */
asx_plan *asx_plan_create_ex(size_t sample_len, size_t max_batch, int device, const char *split);
/* "measure" plans only, once, at their first asx_xcorr_batch_f32_dev call of at least min(group, 8) pairs: the forward column
 * kernel is timed against the caller's buffers on two allocations of its output workspaces (those of the plan's first stream
 * lane) and the faster set is kept (the kernel runs 2-5 % apart with the physical placement of the buffers it streams
 * together; offsets inside an allocation change nothing).  That call allocates, SYNCHRONISES with the device (events on the
 * caller's stream) and frees: a few milliseconds and, transiently, a second set of workspaces; a call made while its stream is
 * being captured into a graph does not tune (the next one outside a capture does).  asx_plan_placement: the two times in ms (0 = not measured)
 * and which set was kept (0 = the first, 1 = the second, -1 = not measured).  Plans of every other mode never do this. */
int asx_plan_placement(asx_plan *plan, double ms[2], int *kept);
void asx_plan_destroy(asx_plan *plan);

/* Peak search exactness (replaces max_abs_index(), src/cross_correlation.c:52-67, a float64 scan).
 * The transforms run in float32; every lag whose float32 value is within the float32 error bound of
 * the float32 maximum is re-evaluated exactly and the reference's rule is applied to the exact values,
 * for up to asx_plan_peak_capacity() such lags per pair (2048..16384 by sample_len; all 2N lags for
 * short tracks).  A pair with more near-ties than that (a signal periodic in that many lags, an offset
 * of hundreds of deviations in both tracks) is marked on the device, counted -- asx_plan_peak_overflows():
 * *count = number of such pairs since the plan was created -- and EVERY entry point, the device-resident
 * asx_xcorr_batch_f32_dev included, takes a second look at it before it returns: the pair's transforms
 * again on the mean-removed source, into lists that hold all 2N lags, so that no candidate limit remains
 * and the lag is the reference's float64 argmax by construction (asx_plan_peak_repairs() counts these;
 * slow: candidates x N multiply-adds).  The price: one host synchronisation of the call's stream per call
 * (per window of >= 1024 pairs of a very long batch), behind the last launch group; the second look itself
 * only runs when the list of marked pairs is not empty.
 * asx_plan_set_exact(plan, 0) trades that for a fully asynchronous asx_xcorr_batch_f32_dev: no host
 * synchronisation, and a marked pair comes back with ret[i] = 1 ("inexact: lag[i] is the float32 argmax,
 * submit the pair again on an exact plan") -- never silently.  ret[i] = 1 cannot occur in the default mode.
 * Both getters synchronise the plan's streams. */
int asx_plan_peak_overflows(asx_plan *plan, uint64_t *count);
int asx_plan_peak_repairs(asx_plan *plan, uint64_t *count);
/* on != 0 (the default): see above.  Synchronises the plan's streams. */
int asx_plan_set_exact(asx_plan *plan, int on);
size_t asx_plan_peak_capacity(const asx_plan *plan);

/* Lag window of the peak search ("maxlag" of MATLAB's xcorr, max_tau of GCC-PHAT tools): only the lags lag_min..lag_max,
 * -N <= lag_min <= lag_max <= N-1, compete for the peak; the default [-N, N-1] is every lag.  Lag l >= 0 is index l of the
 * reference's results[], lag l < 0 index 2N + l (the inverse of the wrap at src/cross_correlation.c:256-263), so the window
 * is one or two ranges of [0, 2N).  The windowed peak is max_abs_index() (src/cross_correlation.c:52-67) run over the
 * in-window elements in ascending index order: the first of them (the smallest in-window index, the "seed") starts the
 * running maximum with its SIGNED value, as arr[0] does at :56, every later one competes with fabs and the strict '>' of :60.
 * So the smallest index wins ties; a digitally silent pair returns the seed's lag; a negative r at the seed loses to any
 * larger |r| in the window, as a negative r[0] does without one.  Everything after the peak is unchanged: the lag wrap and
 * segments (:256-271), the Pearson coefficient in both forms, ret = -1 for a NaN, ret = 1 in the asynchronous mode, the
 * near-tie lists and the second look (which runs with the window of the call that listed the pair).  When the windowed peak
 * is the unwindowed one, every output is bit for bit the unwindowed call's.  The full window runs exactly the kernels of a
 * plan that never had one; any other window runs the inverse column pass in its windowed form (csrc/rlayout.hip
 * k_inv_cols_r<..., AsxWin>, csrc/xcorr_kernels.hip k_inv_cols<..., AsxWin>).  The window does not prune work: the call costs what it costs.
 * Every entry point on the plan honours it (asx_xcorr_debug_r_dev still returns the whole of r; asx_xcorr_batch_multi /
 * _multi_dev: set it on each plan).  Setting it neither allocates nor synchronises: it is safe between captured calls.
 * asx_plan_set_lag_window returns -1 and leaves the window unchanged when lag_min < -N, lag_max > N-1 or
 * lag_min > lag_max. */
int asx_plan_set_lag_window(asx_plan *plan, int64_t lag_min, int64_t lag_max);
int asx_plan_lag_window(const asx_plan *plan, int64_t *lag_min, int64_t *lag_max);

/* The Pearson coefficient of src/cross_correlation.c:74-116 (pearson_coefficient(), :272) in the batched float32 entry
 * points.  Two forms, the same formula:
 *   direct    the reference's reduction over both segments (one streaming pass with the accuracy of its two);
 *   spectral  (the default on plans for the reference's six lengths, asx_plan_layout() == 1) the cross term is r[peak] --
 *             exactly the sum the transforms have just computed (minus, for a negative lag, the |lag| products that did not
 *             wrap around) -- and the four window sums come from per-band sums the forward pass keeps of the samples it
 *             loads anyway; the inputs are not read a second time.  r[peak] carries the float32 transforms' error; its
 *             bound (the one that guards the lag) and that of the float32 band sums are turned into a bound on the
 *             coefficient's error PER PAIR, and a pair whose bound exceeds 1e-5 (quiet windows of a loud track, large
 *             offsets, short segments) takes the direct form by itself.  So: |coefficient - reference's| <= 1e-5 either
 *             way (the bound is first order in the rounding errors it adds up; measured worst case over the parity and
 *             fuzz runs: 5e-7); the spectral form's value is not bit-identical to the direct form's.
 *             ONE OBSERVABLE DIFFERENCE: identical (or exactly negated) segments give exactly +-1.0 only in the direct form
 *             (the reference's own test asserts `coefficient == 1.0`, tests/test_cross_correlation.c:29); the spectral form
 *             returns a value clamped to [-1, 1] within 1e-5 of +-1.0 (tests/test_gpu_pearson_spectral.py::
 *             test_identical_segments_on_the_spectral_path).  asx_plan_set_pearson(plan, 0) restores the reference's bits.
 * cross_correlation(double*) / asx_xcorr_f64 / asx_stream_xcorr always use the direct form on the caller's doubles.
 * asx_plan_pearson_modes: pairs so far that took {spectral, spectral + wrap-around correction, direct} under the spectral
 * setting (synchronises the DEVICE: batches submitted on a caller's stream are counted too). */
int asx_plan_set_pearson(asx_plan *plan, int spectral);
int asx_plan_pearson_modes(asx_plan *plan, uint64_t counts[3]);

/* The pruned inverse pass (real-column plans; on by default there, $ASX_PRUNE=0 = the initial value off).  The row pass of a group
 * also leaves the energy of every row of Q per column tile; by Parseval no |r| of a tile exceeds sqrt(4 M1 x the tile's energy), and
 * a tile whose bound lies under the near-maximum window of the pair's running maximum is not transformed: it can hold neither the
 * peak nor a lag the exact re-evaluation would look at.  The tile with the largest bound and the tile of lag 0 go first, the others
 * only if their bound allows; a tile too quiet for its float32 energies to be trusted (underflow) has no bound and is transformed.
 * Lag, ret and coefficient are what the unpruned pass returns, bit for bit; only
 * asx_plan_peak_overflows may come out smaller (fewer stale near-tie entries).  Taken by the float32 batch and strided calls without
 * a broadcast track when every lag competes (the plan's full window, no per-pair windows, k = 1, no pools); every other call, the
 * second look and asx_xcorr_debug_r_dev run the unpruned kernels whatever the setting.  asx_plan_set_prune(plan, 1) fails on a
 * packed-sample plan.
 * asx_plan_prune_stats: column tiles the pruned groups transformed, and the tiles those groups had in all, over the plan's life
 * (synchronises the DEVICE, as asx_plan_pearson_modes does). */
int asx_plan_set_prune(asx_plan *plan, int on);
int asx_plan_prune_stats(asx_plan *plan, uint64_t *tiles_transformed, uint64_t *tiles_total);

/* Partial storing of Q in the pruned inverse pass (the two longest lengths, N = 960 000 and 1 440 000; $ASX_QSTORE = the initial
 * mode).  The pruned pass reads about two of a pair's column tiles of Q, so the row pass of a group need not store the others: it
 * runs a few rows first, which store everything; from their tile energies each pair's tile 0 and up to three outstanding tiles are
 * predicted -- or none, for unrelated tracks, and the pair stores everything -- and the other rows store only those.  The exact
 * bounds then decide, as ever, which tiles the result needs; a pair that needs a tile that was not stored is run again through the
 * full-store kernels when the call reads its overflow list.  Lag, ret, coefficient and every counter are what mode 0 returns, bit
 * for bit.  Exact mode only (asx_plan_set_exact): the asynchronous mode never reads the list and keeps the full-store row pass.
 *   mode 0  off
 *   mode 1  auto, the default: groups of at least eight generations of row blocks (14 pairs at N = 1 440 000 on 256 compute units);
 *           smaller groups and single pairs launch exactly what mode 0 launches
 *   mode 2  always (any group size, eight predictor rows): for tests
 * asx_plan_qstore_stats: pairs given a list, pairs that stored everything, pairs run again, tiles stored, over the plan's life
 * (synchronises the DEVICE, as asx_plan_pearson_modes does). */
int asx_plan_set_qstore(asx_plan *plan, int mode);
int asx_plan_qstore_stats(asx_plan *plan, uint64_t out[4]);

/* Introspection (used by tests, bench and DESIGN.md's numbers). */
size_t asx_plan_sample_len(const asx_plan *plan);
size_t asx_plan_fft_len(const asx_plan *plan);        /* F, real transform length */
int asx_plan_split(const asx_plan *plan, int *m1, int *m2, int *tile_cols);
/* Which decomposition the plan runs: 1 = the real-column kernels (csrc/rlayout.hip: r2c / c2r column transforms with the
 * untangling inside the tile, one independent row problem per k1; the reference's six lengths), 0 = the packed-sample
 * kernels (csrc/xcorr_kernels.hip: any length; forced by $ASX_LAYOUT=packed), -1 = NULL plan.  Same results either way. */
int asx_plan_layout(const asx_plan *plan);
int asx_plan_threads(const asx_plan *plan, int *threads_cols, int *threads_rows); /* block sizes */
size_t asx_plan_group(const asx_plan *plan);          /* pairs per launch group */
size_t asx_plan_workspace_bytes(const asx_plan *plan);

/* ---- the hot path ------------------------------------------------------ */

/* One pair, host double buffers: the reference's own calling convention.
 * source: 2N doubles (read only), sample: N doubles.  Copies to the device,
 * converts to float32 there, runs the transforms in float32 and the Pearson
 * reduction in float64 on the ORIGINAL doubles.  Returns 0, or -1 exactly
 * where the reference does (device/allocation failure: outputs untouched;
 * NaN coefficient: outputs written). */
int asx_xcorr_f64(asx_plan *plan, const double *source, const double *sample, long *lag,
                  double *coefficient);
/* When EVERY double of both buffers is exactly a float32 -- true of whatever ffmpeg decodes from 16-bit or float audio,
 * although the reference asks it for f64le (src/capture/linux_capture.c:370) -- asx_xcorr_f64 moves 4 bytes per frame across PCIe instead of 8: the check and the conversion run on a small host thread pool
 * ($ASX_HOST_THREADS, default 12 or the cgroup's CPU quota) into page-locked staging, overlapped with the uploads, and the float64 passes read the
 * float32 copy widened on the device: the same values, the same operations, the same bits.  Anything else (a NaN, a value
 * with more than 24 significant bits) takes the 8-byte route.  $ASX_NARROW=0 switches the check off.
 * asx_plan_narrowed_calls(): how many asx_xcorr_f64 calls on this plan went the 4-byte way. */
int asx_plan_narrowed_calls(asx_plan *plan, uint64_t *count);

/* `batch` pairs, host float32 buffers laid out pair after pair:
 * source[batch][2N], sample[batch][N].  lag/coef/ret: `batch` entries each. */
int asx_xcorr_batch_f32(asx_plan *plan, const float *source, const float *sample, size_t batch,
                        int64_t *lag, double *coef, int32_t *ret);

/* Same with everything already resident in this plan's device memory space.
 * All pointers are DEVICE pointers; `stream` is a hipStream_t (NULL = the
 * plan's own stream).  Results are valid after the stream is synchronised (the
 * call itself waits once for its kernels to look at the list of overflowed pairs,
 * see asx_plan_set_exact; what it enqueues after that is asynchronous).
 * source pairs are 2N floats apart, sample pairs N floats.
 * A plan's workspaces are shared by all its calls: use ONE stream at a time per plan
 * (calls on different streams must be ordered by the caller, e.g. with events);
 * concurrent work belongs on separate plans. */
int asx_xcorr_batch_f32_dev(asx_plan *plan, const float *d_source, const float *d_sample,
                            size_t batch, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                            void *stream);

/* Strided batches: one track against many.  Pair i (0 <= i < batch) is source = d_source + i*source_stride (2N floats),
 * sample = d_sample + i*sample_stride (N floats); strides are in floats.  A stride of 0 broadcasts one track to every pair
 * (one source against many samples, one sample against many sources; both 0 is legal); on real-column plans
 * (asx_plan_layout() == 1) its forward column transform then runs ONCE per call, into a plan-owned workspace that every launch
 * group reads, not once per pair or per launch group.  Strides below the track length are allowed (overlapping windows of one
 * long recording: source_stride = hop, sample_stride = 0): the inputs are only read.
 *   Results: per pair, bit for bit what asx_xcorr_batch_f32_dev returns on the materialised contiguous pairs on the same plan --
 * lag, coef and ret, both Pearson forms, exact mode on or off (the second look at overflowed pairs, ret = 1 in the asynchronous
 * mode), and the overflow, repair and Pearson-mode counters, which count every pair as that call would.  d_lag and d_ret may
 * be NULL.  Same stream rule as asx_xcorr_batch_f32_dev; this call never tunes placement ("measure" plans).
 *   Layout rule.  Real-column plans read every row of a pair's inputs with 16-byte float4 loads starting at the pair's first
 * frame, so both base pointers must be 16-byte aligned and every NONZERO stride a multiple of 4 floats; otherwise the call
 * returns -1 (asx_last_error() says which) before anything is launched and the outputs are untouched.  Packed plans (every
 * other length, or $ASX_LAYOUT=packed) take any float-aligned pointer and any stride: their loads fall back to 4-byte loads
 * where a pair's inputs are not 16-byte aligned; they transform each pair's inputs, a broadcast track included.
 *   The broadcast workspace ((M1+1)*M2 complex values per operand, plus norm and band partials) is allocated at the first call
 * with a stride of 0 and kept with the plan.  That first call must not be made while `stream` is being captured into a graph:
 * it returns -1 instead of allocating. */
int asx_xcorr_strided_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                              const float *d_sample, size_t sample_stride, size_t batch,
                              int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream);

/* Strided batches with a lag window per pair (asx_plan_set_lag_window's rule, one window per pair instead of one per plan).
 * Pair i's inputs are exactly those of asx_xcorr_strided_f32_dev (strides, broadcast, layout rule, stream rule).  Its window is
 * d_windows[2*i*window_stride] (lag_min) and d_windows[2*i*window_stride + 1] (lag_max), int64 in DEVICE memory, read when the
 * kernels run: window_stride counts rows of two int64s (1 = one row per pair, 0 = one row for every pair).  So a call captured
 * into a graph (asx_plan_set_exact(plan, 0), as any capture) follows rows that change between replays.
 *   A valid row (-N <= lag_min <= lag_max <= N-1) follows asx_plan_set_lag_window's rule in full, the second look included (it
 * runs with that pair's row): per pair, the results are bit for bit what asx_xcorr_strided_f32_dev returns for that pair alone
 * on the same plan with asx_plan_set_lag_window(plan, lag_min, lag_max).  A full row [-N, N-1] gives the unwindowed bits.
 *   Any other row (an empty one, lag_min > lag_max, included) cannot be refused before launch without a host copy: that pair
 * returns lag = 0, coef = NaN, ret = -2, and is never listed for the second look, so the overflow and repair counters never
 * count it; the Pearson-mode counter (asx_plan_pearson_modes) counts it once as a direct reduction.  The other pairs of the call
 * are unaffected, bit for bit.  Every valid pair counts as the strided call would count it.
 *   d_windows, d_coef and d_ret must not be NULL (d_lag may be); otherwise, or when the layout rule fails, the call returns -1
 * before anything is launched and the outputs are untouched.  The plan's own window is ignored by this call and left as it is.
 * Costs what the strided call costs: the window does not prune work. */
int asx_xcorr_windowed_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                               const float *d_sample, size_t sample_stride,
                               const int64_t *d_windows, size_t window_stride,
                               size_t batch, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                               void *stream);

/* The K strongest separated lags per pair, each with its own Pearson coefficient.  The peak of r is not normalised: its argmax
 * favours lags with a long overlap, and repeated bars, choruses, echoes and reverb give several near-equal peaks, so the true
 * offset can be the runner-up -- with the higher coefficient.  This call returns the runner-ups too, and how close they are.
 *   Inputs.  Strides, broadcast (stride 0), the layout rule of real-column plans and the stream rule are exactly those of
 * asx_xcorr_strided_f32_dev.  d_windows == NULL: the plan's window (asx_plan_set_lag_window) applies to every pair.  Otherwise
 * d_windows holds per-pair rows with the rule of asx_xcorr_windowed_f32_dev, and the plan's window is ignored and left as it is.
 * 1 <= k <= ASX_TOPK_MAX (8) and min_separation >= 0; otherwise, or when d_coef or d_ret is NULL or the layout rule fails, the
 * call returns -1 before anything is launched and the outputs are untouched.  d_lag may be NULL.
 *   Outputs.  Entry j (0-based) of pair i is at index i*k + j of d_lag, d_coef and d_ret.
 *   The rule (float64 semantics, exact by construction like every entry point).  A_1 is the pair's window.  A_j is A_1 minus every
 * lag l with |l - lag_i| <= min_separation for an earlier entry i < j -- linear lag distance, so lags -N and N-1 are far apart.
 * Entry j is max_abs_index() (src/cross_correlation.c:52-67) over the elements of A_j in ascending index order (lag l >= 0 is
 * index l, lag l < 0 index 2N + l, as in the window rule): the smallest index of A_j is the seed and competes with its SIGNED
 * value, every other element with fabs and the strict '>'.  A window with no zone is exactly the window rule.  After the peak,
 * the lag wrap, the segments and the Pearson coefficient follow cross_correlation() (:256-272), as for entry 0.
 *   If A_j is empty, entry j and every later entry of the pair are (0, NaN, -3).  An invalid row gives (0, NaN, -2) for all k
 * entries of its pair.  The other pairs are untouched, bit for bit.
 *   Entry 0 of every pair that did not take the second look is bit for bit the (lag, coef, ret) of asx_xcorr_strided_f32_dev
 * (d_windows == NULL) or asx_xcorr_windowed_f32_dev (with d_windows) on the same plan; k = 1 launches exactly that call, so it is
 * bit for bit that call for every pair, the second look and the counters included.  Entries j >= 1 take either Pearson form
 * within the 1e-5 contract; with asx_plan_set_pearson(plan, 0) entry j's coefficient is bit for bit the direct reduction at its
 * lag (what the windowed call returns for the row [lag_j, lag_j]).
 *   Exact mode (the default).  A pair whose near-tie list overflows in any of its passes is listed once; the second look then
 * recomputes all k entries of that pair with lists that hold every lag and the direct Pearson form.  asx_plan_peak_overflows and
 * asx_plan_peak_repairs count such a pair once per call.  Under the spectral setting, asx_plan_pearson_modes counts every entry of
 * every pair once, in the mode its pass took (an entry with no lag left, and every entry of an invalid row, as a direct reduction;
 * the second look's recomputation is not counted again); under the direct setting it counts nothing, as for every entry point.
 *   Asynchronous mode (asx_plan_set_exact(plan, 0)): the overflowing entry and every later entry of that pair get ret = 1 (their
 * zones came from a float32 argmax), whatever they hold; earlier entries keep their values; nothing is left on the overflow list.
 * The call is then asynchronous and capturable.  Its per-group state lives in workspaces the plan allocates when it is created.
 *   Cost: the transforms run once per call; every further entry is one more inverse column pass over the resident product
 * spectrum plus the tail (finalize, exact re-evaluation, Pearson).  A runner-up at the noise floor has many near-ties in |r|,
 * and their exact re-evaluation makes its pass cost more. */
#define ASX_TOPK_MAX 8
int asx_xcorr_topk_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                           const float *d_sample, size_t sample_stride,
                           const int64_t *d_windows, size_t window_stride,
                           size_t batch, int k, int64_t min_separation,
                           int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream);

/* GCC-PHAT: the strided batch with the phase transform.  Every other entry point ranks lags by the raw correlation r, whose peak
 * belongs to whatever carries the most energy (a shared mains hum, a bass line, a room mode), not to the best alignment.  Here
 * every bin of the cross spectrum Q = X conj(Y), at F = 2N, is divided by its magnitude before the inverse transform, so each
 * frequency has one vote:  Q'[k] = Q[k] / |Q[k]| where |Q[k]| > 0, and Q'[k] = 0 where Q[k] is exactly zero.  Pure PHAT: no floor,
 * no exponent.  The division gives a unit-magnitude bin for every finite non-zero float32 Q[k] whatever its exponent (the exponent
 * is taken out before squaring: tracks scaled by 2^40 or 2^-40 weigh as the unscaled ones do); a NaN bin stays NaN.
 *   Inputs.  Strides, broadcast (a stride of 0), the 16-byte layout rule and the stream rule are those of
 * asx_xcorr_strided_f32_dev.  d_windows == NULL: the plan's lag window (asx_plan_set_lag_window) applies to every pair.  Otherwise
 * d_windows holds per-pair rows exactly as in asx_xcorr_windowed_f32_dev, and the plan's window is ignored and left as it is.
 * Real-column plans only (asx_plan_layout() == 1, where F = 2N): a packed plan returns -1, as the pool calls do.  A NULL d_source,
 * d_sample, d_coef or d_ret, a base pointer that is not 16-byte aligned and a non-zero stride that is not a multiple of 4 also
 * return -1 with nothing launched and the outputs untouched.  d_lag and d_peak may be NULL.  batch == 0 returns 0.
 *   The peak.  max_abs_index() (src/cross_correlation.c:52-67) over the window in ascending index order -- the seed with its
 * signed value, every other element with fabs and the strict '>' -- applied to the FLOAT32 values of r_phat that the device
 * computes; among equal float32 values the smallest index wins.  This is the float32 argmax, NOT the float64 argmax by
 * construction: the error bound, the near-tie lists, the exact re-evaluation and the second look of the other entry points rest
 * on r being the plain time-domain sum, and none of that holds for a whitened spectrum.  The resolution is the float32 error of
 * r_phat / F, measured against a float64 model over all 2N lags: at most 2.2e-8 of full scale at N = 144 000 and 3.2e-8 at N = 960 000
 * (tests/test_gpu_phat.py).  Two lags whose peak heights differ by less than that may come back in either order.
 *   Outputs per pair.  lag: the peak's lag after the reference's wrap (:256-263).  coef: the reference's Pearson coefficient of
 * the ORIGINAL samples at that lag, always in the direct form: under asx_plan_set_pearson(plan, 0) bit for bit what
 * asx_xcorr_windowed_f32_dev returns for the row [lag, lag] (the precedent of the top-k call's later entries), so
 * asx_results_to_ms_dev and the acceptance rule keep working.  peak: |r_phat[lag]| / F, between 0 and 1 -- 1 for a pure circular
 * delay, 0 for a silent pair.  ret: 0, -1 for a NaN coefficient, -2 for a row that is not a window (that pair gets lag 0 and NaN
 * for coef and peak; the other pairs are untouched, bit for bit).  ret is never 1.
 *   A pair with a digitally silent track returns the seed's lag (lag 0 without a window), as the plain rule does, with peak 0.
 *   What the call never does.  It never lists a pair, never takes a second look and never synchronises the host: it is
 * asynchronous whatever asx_plan_set_exact says.  It leaves asx_plan_peak_overflows, asx_plan_peak_repairs, asx_plan_pearson_modes
 * and asx_plan_prune_stats unchanged (the pruned inverse pass is never used: |Q'| = 1 makes its energy bound useless).  It
 * allocates nothing after plan creation, but for the broadcast slot's first allocation under asx_xcorr_strided_f32_dev's rule.
 *   Weakness.  Bins that hold only rounding noise vote too: on band-limited material the empty part of the spectrum adds noise
 * to r_phat and lowers the peak.  asx_xcorr_phat_band_f32_dev, below, lets only a chosen range of bins vote, and
 * asx_xcorr_pool_phat_f32_dev takes listed pairs of two track pools, and asx_xcorr_phat_topk_f32_dev returns the K strongest
 * separated lags of r_phat.  Not offered with PHAT: the double ABI, streams, packed plans, and the neighbourhood of each entry of the
 * top-k call. */
int asx_xcorr_phat_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                           const float *d_sample, size_t sample_stride,
                           const int64_t *d_windows, size_t window_stride, size_t batch,
                           int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Normalised cross-correlation: the strided batch with the lags ranked by the Pearson coefficient itself.  Every other search ranks
 * lags by the raw r or the whitened r_phat and reports the coefficient only at the one lag that won, so a louder, merely similar
 * stretch of the source, a level step or slow rumble can win r with a coefficient near 0.  This call searches the curve of
 * coefficients (what other toolkits call normxcorr or the `coeff` option of xcorr).
 *   The definition.  N = sample_len, x = the source (2N float32), y = the sample (N float32).  Only the lags 0 <= l <= N-1 exist for
 * this call: there the sample lies wholly inside the source, the reference's segment for l >= 0 being source[l, l+N) against the whole
 * sample (src/cross_correlation.c:264-271).  Negative lags are out of scope here: there the circular r[2N + l] also holds the |l|
 * products that wrapped around, and keeping them out for every lag is a second correlation, which prefix sums cannot supply.
 * asx_xcorr_ncc_full_f32_dev, below, runs that second correlation and ranks the lags -(N-1)..N-1.  In float64:
 *     mu     = mean of all 2N source frames
 *     Sx[l]  = sum_{n<N} x[l+n]             (accumulated as sums of x - mu, then N*mu added back: an offset costs no digits)
 *     Vx[l]  = sum_{n<N} (x[l+n] - mean_l)^2 = Sxx'[l] - Sx'[l]^2 / N    on the mu-shifted values
 *     Sy, Vy = the same over the sample, about its own mean
 *     c[l]   = (r32[l] / s  -  Sx[l] * Sy / N) / sqrt(Vx[l] * Vy)
 *     c32[l] = (float) c[l]
 * r32[l] is the float32 value the plan's transforms produce for index l (what asx_xcorr_debug_r_dev returns) and s the factor it
 * carries against the plain sum (asx_plan_fft_len()).  Everything behind r32 is float64: in exact arithmetic c[l] is
 * pearson_coefficient() of the reference's segments at lag l, and the only float32 error in it is that of r32.
 *   Which lags compete.  Vmax = max of Vx[l] over ALL lags 0..N-1, whatever the window.  Lag l competes iff Vy > 0,
 * Vx[l] >= min_energy * Vmax, and c[l] is not NaN (nor infinite: a window of exactly constant frames under an inexact r32).
 * ASX_NCC_MIN_ENERGY (1e-6) <= min_energy <= 1; anything else, a NaN included, is refused.  The floor keeps windows of digital silence
 * out (their coefficient is 0/0) and windows so quiet that the error of r32 divided by their energy is noise of order 1.  A lag whose
 * Vx lies within a relative 1e-6 of the threshold may fall on either side.
 *   The peak.  Among the competing lags of the pair's window the largest |c32[l]| wins, the smallest lag among equal float32 values.
 * There is no signed seed: the reference's arr[0] quirk belongs to max_abs_index() over r, and this curve is not r.  If no lag
 * competes the pair returns lag = the window's lag_min and peak = 0 (a constant or silent sample, a silent source, N = 1).  It is the
 * float32 argmax, NOT the float64 argmax by construction, as for PHAT and for the same reason: two lags closer than the curve's
 * resolution (measured: DESIGN.md, tests/test_gpu_ncc.py) may come back in either order.
 *   Outputs per pair.  lag: the winner.  coef: the reference's coefficient of the ORIGINAL samples at that lag, in the direct form:
 * under asx_plan_set_pearson(plan, 0) bit for bit what asx_xcorr_windowed_f32_dev returns for the row [lag, lag].  peak:
 * (double)|c32[lag]|.  ret: 0 for a computed pair; -1 for a NaN coefficient (lag, coef and peak are still written); -2 for a row that
 * does not satisfy 0 <= lag_min <= lag_max <= N-1 (lag 0, coef NaN, peak NaN, the other pairs untouched bit for bit).  ret is never 1.
 *   Inputs.  Strides, broadcast (a stride of 0), strides below the track length, the 16-byte layout rule on real-column plans and
 * the stream rule are those of asx_xcorr_strided_f32_dev.  The call runs on every plan, packed ones included.  d_windows == NULL
 * means every lag 0..N-1: the plan's own window is ignored and left as it is, because its default [-N, N-1] is not a window of this
 * call.  Otherwise d_windows holds per-pair rows, read on the device as in asx_xcorr_windowed_f32_dev, under the stricter rule above.
 *   Refusals: -1 with nothing launched and the outputs untouched for a NULL plan, track, d_coef, d_peak or d_ret, min_energy out of
 * range, the layout rule failing, and the first allocation (below) failing or falling inside a stream capture.  d_lag may be NULL.
 * batch == 0 returns 0.
 *   What the call never does.  It lists nothing and takes no second look.  It behaves the same whatever asx_plan_set_exact,
 * asx_plan_set_pearson, asx_plan_set_prune, asx_plan_set_qstore and the plan's window say.  It leaves asx_plan_peak_overflows,
 * asx_plan_peak_repairs, asx_plan_pearson_modes, asx_plan_prune_stats, asx_plan_qstore_stats and asx_plan_workspace_bytes unchanged.
 * After its first call on a plan it allocates nothing (but for the broadcast slot's first allocation under
 * asx_xcorr_strided_f32_dev's rule, which that call counts in asx_plan_workspace_bytes), and it never synchronises the host.  Every value of a pair is independent of the
 * batch size and of the pair's position in the batch: the reduction trees are fixed by N alone.  A broadcast track's moments are
 * computed once per call.
 *   Memory.  r of every lag (8N bytes per pair) and a per-lag table of the source's sliding sums (16N bytes per source track) for one
 * group of pairs form one set, allocated at the plan's first NCC call and kept with the plan; it is not counted in
 * asx_plan_workspace_bytes.  The call works in groups of min(asx_plan_group(), 2^30 / 24N) pairs, at least one, so the set holds at
 * most 1 GiB (or one pair's 24N bytes).
 *   Cost: the transforms of the strided call with every inverse tile in its general form (r is written out), three passes over the
 * tracks for the moments and one over r and the table (measured: DESIGN.md).
 *   Not offered: negative lags in this call (asx_xcorr_ncc_full_f32_dev has them), a neighbourhood or fractional lag
 * (asx_xcorr_curve_f32_dev serves the returned lag), the double ABI, streams, and a fused inverse pass.  Offered as calls of their
 * own, below: top-k (asx_xcorr_ncc_topk_f32_dev), pools (asx_xcorr_pool_ncc_f32_dev, asx_xcorr_pool_ncc_topk_f32_dev) and the full
 * range of lags (asx_xcorr_ncc_full_f32_dev, asx_xcorr_ncc_full_topk_f32_dev). */
#define ASX_NCC_MIN_ENERGY 1e-6
int asx_xcorr_ncc_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                          const float *d_sample, size_t sample_stride,
                          const int64_t *d_windows, size_t window_stride, size_t batch,
                          double min_energy,
                          int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);
/* ONE contiguous pair, every lag competing under min_energy: c32 of lags 0..N-1 to d_c (N floats, NaN where the lag does not
 * compete); the results are those of asx_xcorr_ncc_f32_dev for that pair without rows */
int asx_xcorr_ncc_debug_c_dev(asx_plan *plan, const float *d_source, const float *d_sample, double min_energy,
                              float *d_c, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* The K strongest separated lags of the coefficient curve per pair.  The true offset can be the third-best normalised peak (a
 * quiet copy of the sample next to louder ones, with a level step that the raw top-k call ranks first): this call returns it.
 *   c[l], c32[l], Vmax, min_energy, which lags compete and the row rule 0 <= lag_min <= lag_max <= N-1 are those of
 * asx_xcorr_ncc_f32_dev, word for word; Vmax is over all lags 0..N-1, whatever the window and the zones.  Inputs, strides,
 * broadcast, the layout rule, the stream rule and d_windows are that call's too; the call runs on every plan.
 *   Outputs.  Entry j (0-based) of pair i is at index i*k + j of d_lag, d_coef, d_peak and d_ret.  1 <= k <= ASX_TOPK_MAX (8) and
 * min_separation >= 0.
 *   The rule.  A_0 is the set of lags of the pair's row: 0..N-1 when there are no rows (the plan's window is ignored, as in the NCC
 * call).  A_j is A_0 minus every lag l with |l - lag_i| <= min_separation for an earlier entry i < j.
 *   Entry j, when A_j holds a competing lag: the largest |c32| among the competing lags of A_j wins, the smallest lag among equal
 * float32 values; there is no signed seed.  peak = (double)|c32[lag]|.  coef is the direct Pearson form at that lag: under
 * asx_plan_set_pearson(plan, 0) bit for bit what asx_xcorr_windowed_f32_dev returns for the row [lag, lag].  ret is 0, or -1 for a
 * NaN coefficient.
 *   Entry j, when A_j is not empty but no lag of it competes: lag = the smallest lag of A_j, peak = 0, coef and ret as above.  The
 * zone around that lag is taken like any other.  (What the NCC call does for entry 0, and the PHAT top-k call for a silent pair.)
 *   Entry j, when A_j is empty: entry j and every later entry are (0, NaN, peak NaN, -3).
 *   A row that is not a row of this call gives (0, NaN, NaN, -2) in all k entries.  The other pairs are untouched, bit for bit.
 * ret is never 1.
 *   k = 1 launches exactly asx_xcorr_ncc_f32_dev.  Entry 0 is always bit for bit the k = 1 result.  It is the float32 argmax of each
 * pass, NOT the float64 argmax by construction, as the NCC call states for its one pass.
 *   Refusals: those of asx_xcorr_ncc_f32_dev (a NULL plan, track, d_coef, d_peak or d_ret, min_energy out of range, the layout rule,
 * the first allocation inside a stream capture), and k or min_separation out of range: -1 with nothing launched and the outputs
 * untouched.  d_lag may be NULL.  batch == 0 returns 0.
 *   What the call never does is what the NCC call never does: no listing, no second look, no counters, no host synchronisation.  It
 * behaves the same whatever asx_plan_set_exact, asx_plan_set_pearson, asx_plan_set_prune and asx_plan_set_qstore say, and leaves
 * asx_plan_workspace_bytes unchanged.  Once the plan's NCC set exists the call is asynchronous and capturable.
 *   Memory and cost.  The first pass forms c32 of every lag anyway; it is kept in the upper half of the group's r (the negative lags,
 * which no NCC kernel reads), so the set's size rule is that of asx_xcorr_ncc_f32_dev, plus 80 bytes per pair.  Every further entry
 * rescans those 4N bytes per pair with the row and at most 7 zones masked, and runs one direct Pearson pass: no further inverse
 * transform, and no dependence on the height of the runner-up (measured: DESIGN.md). */
int asx_xcorr_ncc_topk_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                               const float *d_sample, size_t sample_stride,
                               const int64_t *d_windows, size_t window_stride, size_t batch,
                               double min_energy, int k, int64_t min_separation,
                               int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Normalised cross-correlation over listed pairs of two track pools.  All-pairs over C clips is C^2 pairs but only C sources and C
 * samples: here every track's transform (the bank) AND its moments -- the per-lag table {Sx, Vx} and Vmax of a source track, {mu, Sy,
 * Vy} of a sample track -- are formed once per call, not once per pair.
 *   Everything before `batch` means what it means in asx_xcorr_pool_f32_dev: aliasing pools, strides below the track length,
 * d_pairs == NULL = every combination, source-major; the layout and stream rules are the same, and the bank is filled once per call
 * with the same growth rule.  Real-column plans only.  d_windows == NULL means every lag 0..N-1; otherwise per-pair rows under the NCC
 * call's rule 0 <= lag_min <= lag_max <= N-1.  min_energy, the curve, which lags compete, the peak and the outputs per pair are those
 * of asx_xcorr_ncc_f32_dev.
 *   Per pair inside its pools, the results are bit for bit those of asx_xcorr_ncc_f32_dev for that pair alone on the same plan: the
 * bank gives the same float32 Q, so the same r32, and the moment trees are fixed by N.
 *   A pool index outside its pool gives (0, NaN, NaN, -4).  It takes precedence over -2, and nothing outside the pools is read.  The
 * other pairs are untouched, bit for bit.  ret is never 1.
 *   Refusals: every refusal of asx_xcorr_pool_f32_dev, plus the NCC call's (min_energy out of range, a NULL d_peak): -1, nothing
 * launched, outputs untouched.  batch == 0 returns 0.
 *   Memory.  Beside the bank and the NCC set, the plan keeps a track set sized by the pools: 16N bytes per source track, plus the
 * chunk sums (three doubles per 2048 frames of every track) and four doubles per track.  It is allocated at the first pool NCC call
 * and grows like the bank: everything is reallocated behind a device synchronisation when a call names more tracks, never inside a
 * stream capture (such a call returns -1; make one call with pools at least this large outside the capture first).  It is not
 * counted in asx_plan_workspace_bytes.  Once its sets exist the call is asynchronous and capturable.
 *   What the call never does is what the NCC call never does. */
int asx_xcorr_pool_ncc_f32_dev(asx_plan *plan, const float *d_sources, size_t source_stride, size_t nsources,
                               const float *d_samples, size_t sample_stride, size_t nsamples,
                               const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride, size_t batch,
                               double min_energy,
                               int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* ... with the K strongest separated lags per pair: the rule and the outputs of asx_xcorr_ncc_topk_f32_dev over the pairs of
 * asx_xcorr_pool_ncc_f32_dev.  k = 1 launches exactly asx_xcorr_pool_ncc_f32_dev, and entry 0 is always bit for bit the k = 1 result.
 * For a pair inside its pools, all k entries are bit for bit those of asx_xcorr_ncc_topk_f32_dev for that pair alone on the same plan.
 * A pool index outside its pool gives (0, NaN, NaN, -4) in all k entries; it takes precedence over -2 and -3.  Refusals: those of the
 * pool call above plus k and min_separation out of range.  The bank and the track set are filled once per call whatever k is.
 *   The [C][C][k] tables of an all-pairs call have the layout asx_pool_closure_dev takes, but feeding them to it is not offered: this
 * curve holds the lags 0..N-1 only, so a pair whose true lag is negative has no entry to offer.  The tables for closure come from
 * asx_xcorr_pool_ncc_full_topk_f32_dev, below, whose curve holds the lags -(N-1)..N-1. */
int asx_xcorr_pool_ncc_topk_f32_dev(asx_plan *plan, const float *d_sources, size_t source_stride, size_t nsources,
                                    const float *d_samples, size_t sample_stride, size_t nsamples,
                                    const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride, size_t batch,
                                    double min_energy, int k, int64_t min_separation,
                                    int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Full-range normalised cross-correlation: asx_xcorr_ncc_f32_dev over the lags -(N-1) <= l <= N-1, so that a pair whose sample starts
 * before the source has an entry too.  Lag -N has no overlap and does not exist for these calls.  N = sample_len, x = the source (2N
 * float32), y = the sample (N float32).
 *   Lags l >= 0.  Everything is that of asx_xcorr_ncc_f32_dev, word for word: mu, Sx[l], Vx[l], Sy, Vy, Vmax (the maximum of Vx[l] over
 * the lags 0..N-1), c[l], c32[l] and the competing rule Vx[l] >= min_energy * Vmax.  c32[l] is bit for bit what
 * asx_xcorr_ncc_debug_c_dev writes: the same transforms and the same moment kernels on the same chunks.
 *   Lags l < 0.  The overlap is m = N + l frames and the segments are the reference's own (src/cross_correlation.c:256-262): x[0, m)
 * against y[-l, N).  In float64, with a[n] = x[n] - mu (the same mu) and b[n] = y[n] - mean(y):
 *     P1[m] = sum_{n<m} a[n],      P2[m] = sum_{n<m} a[n]^2
 *     T1[m] = sum_{n>=N-m} b[n],   T2[m] = sum_{n>=N-m} b[n]^2
 *     Sx[l] = P1[m] + m*mu         Vx[l] = P2[m] - P1[m]^2 / m
 *     Sy[l] = T1[m] + m*mean(y)    Vy[l] = T2[m] - T1[m]^2 / m
 *     c[l]  = (rlo32[2N + l] / s  -  Sx[l] * Sy[l] / m) / sqrt(Vx[l] * Vy[l]),   c32[l] = (float) c[l]
 * rlo32 is the float32 r that the plan's transforms produce for the pair (x_lo, y), x_lo being x with the frames N..2N-1 set to zero,
 * and s = asx_plan_fft_len().  With the upper half zero nothing wraps around: index 2N + l holds exactly the m wanted products.  (The
 * difference r[2N + l] - corr(x_hi, y) is not formed: it would subtract two float32 numbers of the size of whatever fooled the raw
 * search.)
 *   Which negative lags compete.  Lag l < 0 competes iff m >= min_overlap, Vy > 0 (the whole sample's), Vx[l] * Vy[l] >= min_energy *
 * Vmax * Vy, and c[l] is finite.  For l >= 0 the product rule would reduce to the NCC call's, which stays as it is.  The floor means
 * the same on both sides: the error of r32 over the segment energies.  A lag within a relative 1e-6 of the threshold may fall on
 * either side.  1 <= min_overlap <= N, anything else is refused; min_energy as in the NCC call.
 *   Rows.  -(N-1) <= lag_min <= lag_max <= N-1; any other row gives (0, NaN, NaN, -2), the other pairs untouched bit for bit.
 * d_windows == NULL means every lag -(N-1)..N-1; the plan's own window is ignored and left as it is.
 *   The peak.  The largest |c32| among the competing lags of the row wins, the smallest (most negative) lag among equal float32
 * values.  There is no signed seed.  If no lag competes: lag = the row's lag_min (-(N-1) without rows) and peak = 0.  It is the float32
 * argmax, NOT the float64 argmax by construction, as in the NCC call.
 *   Outputs per pair.  lag; coef: the direct Pearson form at the returned lag, under asx_plan_set_pearson(plan, 0) bit for bit what
 * asx_xcorr_windowed_f32_dev returns for the row [lag, lag]; peak: (double)|c32[lag]|; ret: 0, -1 (a NaN coefficient) or -2.  Never 1.
 *   Consequences.  (a) A pair with a row inside [0, N-1] returns, bit for bit, asx_xcorr_ncc_f32_dev's result for that row.  (b) With
 * min_overlap == N no negative lag competes: the competing set and the peak value are the NCC call's, and a pair whose NCC result has
 * a competing lag returns that result bit for bit.
 *   Strides, broadcast (a stride of 0), strides below the track length, the layout rule, the stream rule, the refusals (plus
 * min_overlap out of range) and what the call never does are the NCC call's.  The calls run on every plan, packed ones included.
 * Every value of a pair is independent of the batch size and of the pair's position in the batch.  A broadcast track's moments, staged
 * copy and tables are formed once per call.
 *   Memory.  A set of its own, allocated at the plan's first full-range call and kept with the plan; not counted in
 * asx_plan_workspace_bytes; refused inside a stream capture until it exists.  Per pair of one group: two r buffers (16N bytes; the
 * top-k call keeps the curve in the halves of them that nothing reads), the staged x_lo (8N), the per-lag tables of the source for
 * the lags >= 0 and < 0 (16N each) and of the sample (16N): 72N bytes, plus three doubles per 2048 frames of every track.  The call
 * works in groups of min(asx_plan_group(), 2^30 / 72N) pairs, at least one, so the set holds at most 1 GiB (or one pair's 72N bytes).
 *   Cost: two transform passes per group instead of one, the NCC call's moment passes, one pass over the first halves of the tracks
 * for the tables of the negative lags and a peak pass over twice the lags: about twice the NCC call (measured: DESIGN.md).
 *   Not offered: pools in this call (asx_xcorr_pool_ncc_full_f32_dev, below, has them, and with them the tables
 * asx_pool_closure_dev takes); the double ABI, streams, and a fused inverse pass. */
int asx_xcorr_ncc_full_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                               const float *d_sample, size_t sample_stride,
                               const int64_t *d_windows, size_t window_stride, size_t batch,
                               double min_energy, int64_t min_overlap,
                               int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);
/* ... with the K strongest separated lags per pair, under asx_xcorr_ncc_topk_f32_dev's rule over the signed lags: A_0 is the row, or
 * [-(N-1), N-1]; the zones are |l - lag_i| <= min_separation in signed lags, with no wrap between N-1 and -(N-1); an entry whose A_j
 * holds no competing lag takes A_j's smallest lag with peak = 0; entries behind an empty A_j are (0, NaN, NaN, -3); a row that is not
 * a row of this call gives (0, NaN, NaN, -2) in all k entries.  k = 1 launches exactly asx_xcorr_ncc_full_f32_dev, and entry 0 is
 * always bit for bit the k = 1 result.  Refusals: those of that call, plus k and min_separation out of range. */
int asx_xcorr_ncc_full_topk_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                                    const float *d_sample, size_t sample_stride,
                                    const int64_t *d_windows, size_t window_stride, size_t batch,
                                    double min_energy, int64_t min_overlap, int k, int64_t min_separation,
                                    int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);
/* ONE contiguous pair, every lag competing under min_energy and min_overlap: c32 of the lags -(N-1)..N-1 to d_c (2N - 1 floats, lag l
 * at index l + N - 1, NaN where the lag does not compete); the results are those of asx_xcorr_ncc_full_f32_dev for that pair without
 * rows */
int asx_xcorr_ncc_full_debug_c_dev(asx_plan *plan, const float *d_source, const float *d_sample, double min_energy,
                                   int64_t min_overlap, float *d_c, int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret,
                                   void *stream);

/* Ragged normalised cross-correlation: the curve of asx_xcorr_ncc_full_f32_dev for pairs whose tracks are shorter than the plan's
 * shape.  Pair i's source holds Ls <= 2N frames and its sample Lm <= N, and every moment of a lag is taken over the frames that the
 * two really share there.  (Cutting every track to the shortest throws the overlap away; zero-padding them lets the padding into Sy,
 * Vy and the window sums, and a sample that rides on an offset becomes a rectangular pulse that is ranked against other pulses.)
 *   Lengths.  Pair i's row {Ls, Lm} is read on the device, at d_lengths + 2 * i * length_stride, the way the rows of d_windows are
 * read; a length_stride of 0 means one row for all pairs, and d_lengths == NULL means (2N, N) for every pair.  A row is valid iff
 * 1 <= Ls <= 2N and 1 <= Lm <= N; any other row gives (0, NaN, NaN, -5) in all entries, which takes precedence over -2 and -3, the
 * other pairs untouched bit for bit.  The tracks still occupy 2N and N floats at the caller's strides.  Frames at and beyond a track's
 * length are ignored whatever they hold, NaN included: the call stages, per pair, x' = x[0, Ls) then zeros up to 2N, x_lo' =
 * x[0, min(Ls, N)) then zeros, and y' = y[0, Lm) then zeros, and reads nothing else of them.  A broadcast track (a stride of 0) is
 * staged and summed per pair as well, since each pair may cut it differently.
 *   The curve.  Lags -(N-1) <= l <= N-1 at index l + N - 1, 2N - 1 values, as in the full-range call.  In float64, behind r32:
 *     mu = mean x[0, Ls),  my = mean y[0, Lm),  a = x - mu,  b = y - my
 *     PA1[j] = sum_{n<j} a[n],  PA2[j] = sum_{n<j} a[n]^2  (j = 0..Ls);   PB1, PB2 likewise over b (j = 0..Lm)
 *     n0 = max(0, -l),  n1 = min(Lm, Ls - l),  m = n1 - n0            (m <= 0: the lag does not exist)
 *     S1x = PA1[n1+l] - PA1[n0+l],  S2x likewise,  Vx[l] = S2x - S1x^2 / m,  Sx = S1x + m*mu   (y: over [n0, n1))
 *     c[l] = (r32 / s - Sx * Sy / m) / sqrt(Vx[l] * Vy[l]),   c32 = (float) c
 *     r32 = rA32[l] for l >= 0,  rlo32[2N + l] for l < 0;   s = asx_plan_fft_len()
 * rA32 is the float32 r of the plan's transforms for (x', y'), rlo32 for (x_lo', y').  With the zeros in place nothing wraps: for
 * l >= 0 the source index n + l is at most 2N - 2, and for l < 0 the wrapped indices fall in the zero half of x_lo'.
 *   Which lags compete.  Lag l competes iff m >= min(min_overlap, Ls, Lm), Vy > 0, Vx[l] * Vy[l] >= min_energy * Vmax * Vy, and c[l]
 * is finite.  Vy = PB2[Lm] - PB1[Lm]^2 / Lm is the sample's energy about my over [0, Lm); Vmax is the largest window energy
 * (PA2[j+w] - PA2[j]) - (PA1[j+w] - PA1[j])^2 / w of the source over the windows x[j, j+w), w = min(Ls, Lm), 0 <= j <= min(Ls - w,
 * N - 1).  1 <= min_overlap <= N, min_energy as in the NCC call.  With (2N, N) this is the full-range call's rule on both sides of
 * zero (the sums are formed in another order, so a lag at the threshold may fall on the other side and the last bits of c32 may
 * differ).  A short sample under the default min_overlap competes only at the lags of full overlap: template matching.  A lag within
 * a relative 1e-6 of the threshold may fall on either side.
 *   Rows, the peak, the outputs: the full-range call's, word for word -- rows -(N-1) <= lag_min <= lag_max <= N-1 or (0, NaN, NaN,
 * -2); the largest |c32| wins, the smallest lag among equals; no lag competes: lag = the row's lag_min and peak = 0.  coef is the
 * direct Pearson form over source[n0+l, n1+l) against sample[n0, n1), from the caller's tracks; a returned lag with m <= 0 has an
 * empty segment: coef = NaN and ret = -1, the reference's empty-segment case.  ret is never 1.
 *   Strides, the layout rule, the stream rule and the refusals are the full-range call's, plus d_lengths == NULL together with a
 * length_stride other than 0.  Every value of a pair is independent of the batch size and of the pair's position in the batch: the
 * sums are fixed trees that N and the pair's lengths decide, Vmax an order-free maximum.  The call takes no listing and no second
 * look, touches no counters, never synchronises the host, behaves the same whatever the plan's setters say and runs on every plan,
 * packed ones included.
 *   Memory.  A set of its own, allocated at the plan's first ragged call and kept with the plan; not counted in
 * asx_plan_workspace_bytes; refused inside a stream capture until it exists.  Per pair of one group: the staged x' and x_lo' (8N
 * bytes each) and y' (4N), two r buffers (16N; the top-k call keeps the curve in the halves that nothing reads), the prefix tables
 * of 2N + 1 and N + 1 double2 (32N + 16N): 84N bytes, plus three doubles per 2048 frames of every track.  The call works in groups
 * of min(asx_plan_group(), 2^30 / 84N) pairs, at least one, so the set holds at most 1 GiB (or one pair's 84N bytes).
 *   Cost: the full-range call's two transform passes, and in place of its moment passes one pass that stages the tracks and three
 * over the staged copies and tables (measured: DESIGN.md).
 *   Not offered: pools (the next step, as the full-range call went); lags >= N, which a short sample would leave unwrapped in pass
 * A; the double ABI; streams. */
int asx_xcorr_ncc_ragged_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                                 const float *d_sample, size_t sample_stride,
                                 const int64_t *d_lengths, size_t length_stride,
                                 const int64_t *d_windows, size_t window_stride, size_t batch,
                                 double min_energy, int64_t min_overlap,
                                 int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);
/* ... with the K strongest separated lags per pair: the rule and the outputs of asx_xcorr_ncc_full_topk_f32_dev (signed lags, no wrap
 * between N-1 and -(N-1), -3 behind an empty A_j, -2 and -5 in all k entries) over the ragged curve.  k = 1 launches exactly
 * asx_xcorr_ncc_ragged_f32_dev, and entry 0 is always bit for bit the k = 1 result.  Refusals: those of that call, plus k and
 * min_separation out of range. */
int asx_xcorr_ncc_ragged_topk_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                                      const float *d_sample, size_t sample_stride,
                                      const int64_t *d_lengths, size_t length_stride,
                                      const int64_t *d_windows, size_t window_stride, size_t batch,
                                      double min_energy, int64_t min_overlap, int k, int64_t min_separation,
                                      int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);
/* ONE contiguous pair of the lengths (source_len, sample_len), host values under the rule of a row of d_lengths: c32 of the lags
 * -(N-1)..N-1 to d_c (2N - 1 floats, lag l at index l + N - 1, NaN where the lag does not exist or does not compete); the results
 * are those of asx_xcorr_ncc_ragged_f32_dev for that pair without rows */
int asx_xcorr_ncc_ragged_debug_c_dev(asx_plan *plan, const float *d_source, const float *d_sample, int64_t source_len,
                                     int64_t sample_len, double min_energy, int64_t min_overlap, float *d_c, int64_t *d_lag,
                                     double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Full-range normalised cross-correlation over listed pairs of two track pools: the pairs of asx_xcorr_pool_ncc_f32_dev under the
 * curve of asx_xcorr_ncc_full_f32_dev.  An all-pairs table over the clips of one event needs both: every track transformed once, and
 * the negative lags, since lag_ba = -lag_ab puts a negative true lag in half the table.
 *   From asx_xcorr_pool_ncc_f32_dev: everything before `batch` (aliasing pools, strides below the track length, d_pairs == NULL =
 * every combination, source-major), the 16-byte alignment rule, the stride rule and the stream rule, real-column plans only, and its
 * refusals.  A pool index outside its pool gives (0, NaN, NaN, -4); it takes precedence over -2, nothing outside the pools is read,
 * and the other pairs are untouched bit for bit.  batch == 0 returns 0.
 *   From asx_xcorr_ncc_full_f32_dev: the curve over -(N-1) <= l <= N-1, min_energy, min_overlap and the two competing rules, the row
 * rule -(N-1) <= lag_min <= lag_max <= N-1 (d_windows == NULL: every lag), the peak rule, the outputs per pair, and the additional
 * refusal for min_overlap outside [1, N].
 *   Per pair inside its pools, the results are bit for bit those of asx_xcorr_ncc_full_f32_dev for that pair alone on the same plan.
 * Every value of a pair is independent of the batch, of the pair's position in it and of the group boundaries.  ret is never 1; no
 * listing, no second look, no counters, no host synchronisation.
 *   Once per call, before the groups, for every TRACK (the strided call does this once per pair): the forward column pass (the bank),
 * the moments and the per-lag table, x_lo of every source track and its forward column pass into a second bank of source spectra
 * (the sample side of pass B is the first bank's: the samples are the same in both passes), the prefix table of every source and the
 * suffix table of every sample track.  Each group then runs only the row and inverse passes of pass A and pass B, the peak pass and
 * the tails.
 *   Memory.  Beside the bank and the pool NCC call's track set (16N bytes per source track), the plan keeps a full-range track set
 * sized by the pools: per source track x_lo (8N bytes), its column spectrum (one bank row: about 8N bytes) and the prefix table
 * (16N), per sample track the suffix table (16N), plus the norm partials and band sums of a bank.  It is allocated at the first such
 * call and grows like the bank: everything is reallocated behind a device synchronisation when a call names more tracks, never
 * inside a stream capture (such a call returns -1; make one call with pools at least this large outside the capture first).  It is
 * not counted in asx_plan_workspace_bytes.  The per-group buffers -- two r buffers per pair (16N bytes), the packed maxima and the
 * top-k records -- are those of the strided full-range set, which this call allocates whole if the plan has none (72N bytes per pair
 * of a group; its per-pair track buffers lie idle in this call) and whose bound of 1 GiB stays: the call works in groups of
 * min(asx_plan_group(), 2^30 / 72N) pairs, at least one, which is smaller than the plan's group wherever 72N * asx_plan_group()
 * exceeds 1 GiB.
 *   Cost (measured: DESIGN.md): per pair the two row and inverse passes, the peak pass and the tails; per track everything else. */
int asx_xcorr_pool_ncc_full_f32_dev(asx_plan *plan, const float *d_sources, size_t source_stride, size_t nsources,
                                    const float *d_samples, size_t sample_stride, size_t nsamples,
                                    const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride, size_t batch,
                                    double min_energy, int64_t min_overlap,
                                    int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* ... with the K strongest separated lags per pair: the rule and the outputs of asx_xcorr_ncc_full_topk_f32_dev (signed lags, no wrap
 * between N-1 and -(N-1)) over the pairs of asx_xcorr_pool_ncc_full_f32_dev.  k = 1 launches exactly that call, and entry 0 is always
 * bit for bit the k = 1 result.  For a pair inside its pools, all k entries are bit for bit those of asx_xcorr_ncc_full_topk_f32_dev
 * for that pair alone on the same plan.  A pool index outside its pool gives (0, NaN, NaN, -4) in all k entries; it takes precedence
 * over -2 and -3.  Refusals: those of the call above plus k and min_separation out of range.  The banks and the track sets are filled
 * once per call whatever k is.
 *   With ONE pool as both sides, d_pairs == NULL and nsources = nsamples = C, the [C][C][k] tables are the input of
 * asx_pool_closure_dev: every pair has an entry for its true lag, whatever its sign. */
int asx_xcorr_pool_ncc_full_topk_f32_dev(asx_plan *plan, const float *d_sources, size_t source_stride, size_t nsources,
                                         const float *d_samples, size_t sample_stride, size_t nsamples,
                                         const int32_t *d_pairs, const int64_t *d_windows, size_t window_stride, size_t batch,
                                         double min_energy, int64_t min_overlap, int k, int64_t min_separation,
                                         int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Band-limited GCC-PHAT: asx_xcorr_phat_f32_dev in which only the bins of a frequency band vote.  Most material is band-limited
 * (speech, codecs that low-pass, hum and rumble at the bottom): outside its band the cross spectrum is rounding noise, and with
 * every bin at unit weight that noise lowers the peak and can move it.  Everything asx_xcorr_phat_f32_dev says holds, but for this:
 *   The band.  Bins are those of the length-F = 2N real transform: bin m, 0 <= m <= N, is the frequency m * rate / (2N)
 * (asx_band_bins converts).  Q'[k] = Q[k] / |Q[k]| when bin_lo <= min(k, F - k) <= bin_hi and Q[k] != 0, and Q'[k] = 0 otherwise: a
 * bin and its mirror are one frequency, so r_phat stays real.  The band must satisfy 0 <= bin_lo <= bin_hi <= N; any other returns
 * -1 with nothing launched and the outputs untouched, as every refusal of asx_xcorr_phat_f32_dev does here too.  One band per
 * call, for every pair.
 *   The peak.  peak = |r_phat[lag]| / V with V = 2 (bin_hi - bin_lo + 1) - [bin_lo == 0] - [bin_hi == N], the number of k in
 * [0, F) that vote: between 0 and 1, and 1 for a pure circular delay whatever the band.  A narrow band makes a wide peak: what
 * the float32 argmax resolves is still the float32 error of r_phat / V over the lags (tests/test_gpu_phat_band.py).
 *   The full band [0, N] IS asx_xcorr_phat_f32_dev: the same kernels, the same bits.
 *   Measured on float64 models of three pairs low-passed at N/6 with noise of 1e-4 under them (N = 144 000, tests/test_phat_band.py):
 * peak 0.041 / 0.027 / 0.096 with every bin voting, one lag wrong; 0.248 / 0.148 / 0.570 with bins [1, N/6], every lag right.
 *   The call costs what asx_xcorr_phat_f32_dev costs, within two percent either way by the band (measured: DESIGN.md); rows
 * that hold no bin of the band are not skipped.  Not offered: a band per pair, a magnitude floor, an exponent. */
int asx_xcorr_phat_band_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                                const float *d_sample, size_t sample_stride,
                                const int64_t *d_windows, size_t window_stride, size_t batch,
                                int64_t bin_lo, int64_t bin_hi,
                                int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* Sub-sample GCC-PHAT: asx_xcorr_phat_band_f32_dev, plus the curve around each pair's peak and a fractional lag.  A delay is
 * rarely a whole number of frames, and the shape of the peak -- its width, its side lobes -- says how far to trust it.
 *   Everything asx_xcorr_phat_band_f32_dev says holds: inputs, strides, broadcast, the layout rule, windows (rows or the plan's), the
 * band and its vote count V (the full band [0, N] runs the plain PHAT kernels, V = F), every refusal, asynchronous whatever
 * asx_plan_set_exact says, no counter touched, nothing allocated.  (lag, coef, peak, ret) are bit for bit that call's results for
 * every pair: what is added runs behind it and only reads.
 *   New arguments.  1 <= half_width <= ASX_NEAR_MAX; d_frac must not be NULL; d_near may be.  Anything else returns -1 with nothing
 * launched and the outputs untouched.
 *   d_near.  With h = half_width and p_i the index of pair i's peak in r_phat (lag l >= 0 is index l, lag l < 0 index 2N + l),
 * d_near[i * (2h + 1) + (d + h)] = r_phat[(p_i + d) mod 2N] / V for d = -h .. h: signed, 2h + 1 doubles per pair.  Neighbours are
 * taken in index space, circularly: index 2N - 1 (lag -1) sits beside index 0, and index N (lag -N) beside index N - 1.  The
 * neighbourhood does not depend on the window: lags outside the pair's window are reported like any other, and one of them may
 * exceed the peak.  Each value is a float64 sum over one column of the group's float32 whitened spectrum Q' (DESIGN.md), so the
 * centre entry is the float64 sum over the same float32 Q' from which peak's float32 inverse transform came: |centre| may differ
 * from peak by the float32 rounding of that transform (at most 2e-7 of full scale, tests/test_gpu_phat_sub.py).
 *   d_frac.  d_frac[i] is the vertex of the parabola through the three centre values y-, y0, y+ (d = -1, 0, 1), all in float64 and
 * in this order: s = -1 when y0 < 0, else +1; a = s y-, b = s y0, c = s y+; den = (a - 2 b) + c.  frac = NaN when any of the three
 * is NaN; frac = 0 when den >= 0 (a flat top, a silent pair); otherwise frac = 0.5 (a - c) / den, clamped to [-0.5, 0.5].  The
 * delay estimate is lag + frac frames.
 *   The parabola is biased on a sinc-shaped peak: a full-band pure delay of a quarter frame past a whole lag gives frac of about
 * 0.14, and 0.4 gives about 0.29 (the table: DESIGN.md).  That is why d_near is offered: a caller fits the interpolator of their
 * choice over 2h + 1 points.
 *   Special pairs.  A silent pair: peak 0, every near entry 0, frac 0.  A pair with ret -2 gets NaN in frac and in all of its near
 * entries; the other pairs are untouched.
 *   Cost: one small kernel per launch group, (M1 + 1)(2h + 1) reads of 8 bytes per pair.  Measured on full groups: 1 % (h = 1) to
 * 4 % (h = 8) of the banded call at N = 144 000, 0.5 % to 1.3 % at N = 1 440 000. */
#define ASX_NEAR_MAX 8
int asx_xcorr_phat_sub_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                               const float *d_sample, size_t sample_stride,
                               const int64_t *d_windows, size_t window_stride, size_t batch,
                               int64_t bin_lo, int64_t bin_hi, int half_width,
                               int64_t *d_lag, double *d_coef, double *d_peak,
                               double *d_frac, double *d_near, int32_t *d_ret, void *stream);

/* Top-k GCC-PHAT: the K strongest separated lags per pair by the whitened curve, each with its coefficient and its peak height.  An
 * echo, a chorus and a second loudspeaker are separate peaks of r_phat; on material whose raw correlation follows a shared hum, these
 * runner-ups by phase alignment are the candidates a closure over several clips (asx_pool_closure_dev) needs.
 *   Inputs.  Strides, broadcast (a stride of 0), the 16-byte layout rule, real-column plans only, per-pair window rows or the plan's
 * window (d_windows == NULL), the band and its vote count V and the stream rule are those of asx_xcorr_phat_band_f32_dev.  The band
 * is always given; the full band [0, N] is plain PHAT and runs the plain PHAT row kernels.  k and min_separation are those of
 * asx_xcorr_topk_f32_dev.  Entry j (0-based) of pair i is at index i*k + j of d_lag, d_coef, d_peak and d_ret.  d_lag and d_peak
 * may be NULL.
 *   The rule.  A_1 is the pair's window.  A_j is A_1 minus every lag l with |l - lag_i| <= min_separation for an earlier entry
 * i < j -- linear lag distance, so lags -N and N-1 are far apart.  Entry j is asx_xcorr_phat_f32_dev's peak rule over A_j in
 * ascending index order, applied to the float32 values of r_phat that the device computes: the smallest index of A_j is the seed and
 * competes with its SIGNED value, every other element with fabs and the strict '>'; among equal float32 values the smallest index
 * wins.  This is the float32 argmax of each pass, exactly as that call states for its one pass: two candidates whose heights differ
 * by less than its resolution may come back in either order.
 *   Outputs per entry.  lag: the peak's lag after the reference's wrap.  coef: the reference's Pearson coefficient of the ORIGINAL
 * samples at that lag, always in the direct form: under asx_plan_set_pearson(plan, 0) bit for bit what asx_xcorr_windowed_f32_dev
 * returns for the row [lag, lag].  peak: |r_phat[lag]| / V.  ret: 0, or -1 for a NaN coefficient.  ret is never 1.
 *   Special entries.  If A_j is empty, entry j and every later entry of the pair are (0, NaN, peak NaN, -3).  A row that is not a
 * window gives (0, NaN, NaN, -2) in all k entries of its pair.  Every other pair is untouched, bit for bit.  A pair with a digitally
 * silent track follows the rule as it stands: every pass finds an empty maximum and returns the seed of A_j with peak 0.
 *   Relation to the other calls.  Entry 0 of every pair is bit for bit the (lag, coef, peak, ret) of asx_xcorr_phat_band_f32_dev on
 * the same plan with the same band and window; k = 1 launches exactly that call.
 *   What the call never does.  It lists nothing, takes no second look and never synchronises the host.  It runs the same whatever
 * asx_plan_set_exact, _pearson, _prune and _qstore say, and leaves asx_plan_peak_overflows, asx_plan_peak_repairs,
 * asx_plan_pearson_modes, asx_plan_prune_stats and asx_plan_qstore_stats unchanged.  It allocates nothing after plan creation (but
 * for the broadcast slot's first allocation under asx_xcorr_strided_f32_dev's rule), asx_plan_workspace_bytes does not change, and
 * it is asynchronous and capturable, as the PHAT call is.
 *   Returns -1 with nothing launched and the outputs untouched on every refusal of asx_xcorr_phat_band_f32_dev, for k outside
 * 1..ASX_TOPK_MAX and for min_separation < 0.  batch == 0 returns 0.
 *   Cost.  The transforms and the row pass run once per call.  Every further entry is one inverse column pass over the resident Q',
 * plus the PHAT tail, the direct Pearson launch and the step; no pass does any exact re-evaluation, so unlike the raw top-k call a
 * runner-up at the noise floor costs what any other pass costs (measured: DESIGN.md).
 *   Not offered: the neighbourhood and fractional lag per entry (asx_xcorr_curve_f32_dev serves raw entries; a PHAT caller re-runs
 * asx_xcorr_phat_sub_f32_dev with a row [lag, lag]), a band per pair, packed plans, the double ABI, streams. */
int asx_xcorr_phat_topk_f32_dev(asx_plan *plan, const float *d_source, size_t source_stride,
                                const float *d_sample, size_t sample_stride,
                                const int64_t *d_windows, size_t window_stride, size_t batch,
                                int64_t bin_lo, int64_t bin_hi, int k, int64_t min_separation,
                                int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* The bins of the band [f_lo_hz, f_hi_hz] for a plan of sample_len = N at sample_rate: bin_lo = ceil(f_lo 2N / rate), bin_hi =
 * min(N, floor(f_hi 2N / rate)) (a band that reaches past the Nyquist frequency ends there).  Host arithmetic, no device.  Returns
 * 0, or -1 with the outputs untouched for a rate that is not positive, f_lo < 0, f_lo > f_hi, a NaN, or a band that holds no bin. */
int asx_band_bins(size_t sample_len, double sample_rate, double f_lo_hz, double f_hi_hz,
                  int64_t *bin_lo, int64_t *bin_hi);

/* Many tracks against many: listed pairs of two track pools, every track transformed once per call.
 * Source track a is d_sources + a*source_stride (2N floats), sample track b is d_samples + b*sample_stride
 * (N floats); strides in floats.  The pools may overlap or alias (one pool of clips as both, for all-pairs),
 * and a stride may be below the track length (windows of one recording).  Row i of d_pairs (int32, device
 * memory, read when the kernels run) is pair i = {a_i, b_i}.  d_pairs == NULL: every combination,
 * source-major -- pair i = (i / nsamples, i % nsamples) -- and batch must be nsources * nsamples.
 * d_windows / window_stride: NULL (the plan's window), or per-pair rows exactly as asx_xcorr_windowed_f32_dev.
 * Pair i's (lag, coef, ret) are bit for bit what asx_xcorr_strided_f32_dev returns for that pair alone on the
 * same plan (with a row: asx_xcorr_windowed_f32_dev with that row), in both Pearson forms, exact and
 * asynchronous (ret = 1) mode alike; the overflow and repair counters count each valid pair as that call
 * would.  A row with an index outside its pool gives that pair (0, NaN, -4) and reads nothing outside the
 * pools; the other pairs are untouched.
 * Returns -1 with the outputs untouched when a pointer is NULL (the pools, d_coef, d_ret), a pool is empty
 * while batch > 0, the plan is not a real-column plan (asx_plan_layout() != 1), the pools are not 16-byte
 * aligned or a stride is not a multiple of 4 floats, or the bank cannot be allocated.  batch == 0 returns 0.
 * One stream at a time per plan, as for the strided call.
 * The bank: the plan keeps the forward column pass of every track of a call, (M1+1)*M2 complex floats per
 * track plus its norm partials and band sums -- about 11.5 MB per track at N = 1 440 000, 1.15 MB at 144 000
 * (8 bytes per frame of 2N, roughly).  It is allocated at the first pool call, grown (behind a device
 * synchronisation) when a call names more tracks, and freed with the plan; it is not counted in
 * asx_plan_workspace_bytes.  Growing it during a stream capture fails (-1): make a call with pools at least
 * as large outside the capture first.  asx_xcorr_pool_topk_f32_dev returns the K strongest lags of every pair. */
int asx_xcorr_pool_f32_dev(asx_plan *plan,
                           const float *d_sources, size_t source_stride, size_t nsources,
                           const float *d_samples, size_t sample_stride, size_t nsamples,
                           const int32_t *d_pairs,
                           const int64_t *d_windows, size_t window_stride,
                           size_t batch, int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream);

/* The K strongest separated lags per pair of two track pools: asx_xcorr_pool_f32_dev's pairs with asx_xcorr_topk_f32_dev's entries.
 * All-pairs over a pool of clips of one event is where runner-ups matter: choruses and bars repeat in every clip, and the candidates
 * of each pair let a caller test triangle closure (lag_ab + lag_bc = lag_ac) over more than two clips.
 *   Everything before `batch` means what it means in asx_xcorr_pool_f32_dev: the pools, strides and aliasing, d_pairs == NULL =
 * every combination source-major (batch = nsources * nsamples), per-pair window rows or the plan's window (d_windows == NULL), the
 * layout rule, the stream rule and the bank -- which is filled ONCE per call, whatever k is.  k and min_separation mean what they
 * mean in asx_xcorr_topk_f32_dev.  Entry j of pair i is at index i*k + j of d_lag, d_coef and d_ret; d_lag may be NULL.
 *   Per pair it is the top-k call: for a pair whose indices are inside their pools, all k entries (lag, coef, ret) are bit for bit
 * what asx_xcorr_topk_f32_dev returns for that pair alone on the same plan with the same k, min_separation and window (the pair's
 * row, or the plan's window) -- in both Pearson settings, in exact and in asynchronous mode (ret = 1 from the overflowing entry on),
 * -3 once no lag is left and -2 in all k entries for a row that is not a window.  k = 1 launches exactly asx_xcorr_pool_f32_dev:
 * the same kernels and the same results, counters and second look included.
 *   A row of d_pairs with an index outside its pool gives (0, NaN, -4) in all k entries of that pair (over -2 and -3), reads nothing
 * outside the pools and leaves the other pairs untouched; such a pair never overflows and is never listed, counted or repaired.
 *   Counters: asx_plan_peak_overflows / asx_plan_peak_repairs count a valid pair once per call if any of its passes overflows.
 * Under the spectral setting asx_plan_pearson_modes grows by batch * k per call (every entry once, in the mode its pass took; the
 * second look's recomputation is not counted again); under the direct setting it counts nothing.
 *   Exact mode: a listed pair's row {a, b} is copied back and the pair is redone alone on explicit pointers -- all k entries, lists
 * that hold every lag, the direct Pearson form -- as the top-k call's second look does.  Asynchronous mode
 * (asx_plan_set_exact(plan, 0)): with a bank already large enough the call makes no host synchronisation and allocates nothing;
 * its per-group state lives in workspaces the plan allocated when it was created.
 *   Returns -1 with the outputs untouched and nothing launched on every refusal of asx_xcorr_pool_f32_dev (a NULL pool, d_coef or
 * d_ret; an empty pool while batch > 0; not a real-column plan; alignment; strides that are not multiples of 4 floats; d_pairs ==
 * NULL with batch != nsources * nsamples; a bank that cannot be allocated, or would have to grow during a stream capture) and of
 * asx_xcorr_topk_f32_dev (k outside 1..ASX_TOPK_MAX, min_separation < 0).  batch == 0 returns 0.
 *   Cost: the bank fill and each group's row pass once per call; every further entry is one more inverse column pass over the
 * resident product spectrum plus the tail, as in asx_xcorr_topk_f32_dev. */
int asx_xcorr_pool_topk_f32_dev(asx_plan *plan,
                                const float *d_sources, size_t source_stride, size_t nsources,
                                const float *d_samples, size_t sample_stride, size_t nsamples,
                                const int32_t *d_pairs,
                                const int64_t *d_windows, size_t window_stride,
                                size_t batch, int k, int64_t min_separation,
                                int64_t *d_lag, double *d_coef, int32_t *d_ret, void *stream);

/* GCC-PHAT over two track pools: asx_xcorr_pool_f32_dev's pairs ranked as asx_xcorr_phat_band_f32_dev ranks them.  All pairs over the
 * clips of one event share a hum, a bass line or a room mode, which is where the raw correlation picks the loudest common component
 * and where the bank pays most: c clips are c * c pairs and 2c forward column passes.
 *   Everything before `batch` means what it means in asx_xcorr_pool_f32_dev: the pools, which may alias or overlap, strides that may
 * be below the track length, d_pairs == NULL = every combination source-major (batch = nsources * nsamples), per-pair window rows or
 * the plan's window (d_windows == NULL), the 16-byte layout rule, the stream rule and the bank with its growth rule -- filled once
 * per call, never grown inside a stream capture.
 *   bin_lo, bin_hi, d_peak, the vote count V and the peak rule mean what they mean in asx_xcorr_phat_band_f32_dev.  The band is always
 * given: the full band [0, N] is plain PHAT, the kernels and the bits of a banded strided call over the full band.
 *   Per pair it is the banded PHAT call: for a pair whose indices are inside their pools, (lag, coef, peak, ret) are bit for bit what
 * asx_xcorr_phat_band_f32_dev returns for that pair alone on the same plan with the same band and window (the pair's row, or the
 * plan's window): the bank holds the same column spectra and the row pass forms the same float32 Q'.  A row that is not a window
 * gives that pair (0, NaN, NaN, -2).  A pair with a digitally silent track returns the seed's lag with peak 0, ret following its NaN
 * coefficient.  ret is never 1.
 *   A row of d_pairs with an index outside its pool gives that pair lag 0, coef NaN, peak NaN and ret -4 (over -2), reads nothing
 * outside the pools and leaves the other pairs untouched, bit for bit.
 *   What the call never does, as the PHAT call: it lists nothing, takes no second look and does not synchronise the host beyond what
 * a bank that must grow costs; it leaves asx_plan_peak_overflows, asx_plan_peak_repairs, asx_plan_pearson_modes, asx_plan_prune_stats
 * and asx_plan_qstore_stats unchanged and runs the same whatever asx_plan_set_exact says.  With a bank already large enough it
 * allocates nothing.
 *   Returns -1 with the outputs untouched and nothing launched on every refusal of asx_xcorr_pool_f32_dev (a NULL pool, d_coef or
 * d_ret; an empty pool while batch > 0; not a real-column plan; alignment; strides that are not multiples of 4 floats; d_pairs ==
 * NULL with batch != nsources * nsamples; a bank that cannot be allocated, or would have to grow during a stream capture) and for a
 * band outside 0 <= bin_lo <= bin_hi <= N.  d_lag and d_peak may be NULL.  batch == 0 returns 0.
 *   Cost: the bank fill once per call, then per group the row pass of the strided PHAT call on the bank's rows and its tail
 * (measured: DESIGN.md).  asx_xcorr_pool_phat_topk_f32_dev returns the K strongest lags of every pair.  Not offered: a band per
 * pair. */
int asx_xcorr_pool_phat_f32_dev(asx_plan *plan,
                                const float *d_sources, size_t source_stride, size_t nsources,
                                const float *d_samples, size_t sample_stride, size_t nsamples,
                                const int32_t *d_pairs,
                                const int64_t *d_windows, size_t window_stride,
                                size_t batch, int64_t bin_lo, int64_t bin_hi,
                                int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* ... with the curve around each pair's peak and a fractional lag: asx_xcorr_pool_phat_f32_dev's arguments up to bin_hi and
 * everything that call says (the pools, d_pairs, windows, the band, the bank, every refusal; (lag, coef, peak, ret) bit for bit its
 * results), then half_width, d_frac and d_near as asx_xcorr_phat_sub_f32_dev defines them, with the same two refusals.  A pair
 * with ret -2 or -4 gets NaN in frac and in all of its near entries; the other pairs are untouched. */
int asx_xcorr_pool_phat_sub_f32_dev(asx_plan *plan,
                                    const float *d_sources, size_t source_stride, size_t nsources,
                                    const float *d_samples, size_t sample_stride, size_t nsamples,
                                    const int32_t *d_pairs,
                                    const int64_t *d_windows, size_t window_stride,
                                    size_t batch, int64_t bin_lo, int64_t bin_hi, int half_width,
                                    int64_t *d_lag, double *d_coef, double *d_peak,
                                    double *d_frac, double *d_near, int32_t *d_ret, void *stream);

/* Top-k GCC-PHAT over two track pools: asx_xcorr_pool_phat_f32_dev's pairs with asx_xcorr_phat_topk_f32_dev's entries.  An all-pairs
 * call over the clips of one event gives the [C, C, k] tables that asx_pool_closure_dev places the clips from, ranked by phase
 * alignment where a shared hum makes the raw ranking least trustworthy.
 *   Everything before `batch` means what it means in asx_xcorr_pool_phat_f32_dev (the pools, d_pairs, windows, the layout and stream
 * rules, the bank, filled ONCE per call whatever k is); the band, k, min_separation, the entry layout (index i*k + j of d_lag,
 * d_coef, d_peak and d_ret; d_lag and d_peak may be NULL), the rule and the outputs are those of asx_xcorr_phat_topk_f32_dev.
 *   Per pair it is that call: for a pair whose indices are inside their pools, all k entries are bit for bit what
 * asx_xcorr_phat_topk_f32_dev returns for that pair alone on the same plan with the same band, k, min_separation and window; entry 0
 * is bit for bit asx_xcorr_pool_phat_f32_dev's result, and k = 1 launches exactly that call.
 *   A row of d_pairs with an index outside its pool gives (0, NaN, NaN, -4) in all k entries of that pair (over -2 and -3), reads
 * nothing outside the pools and leaves the other pairs untouched, bit for bit.
 *   What the call never does is what asx_xcorr_phat_topk_f32_dev never does; the one host synchronisation it can make is a bank that
 * must grow, under asx_xcorr_pool_f32_dev's rule.
 *   Returns -1 with the outputs untouched and nothing launched on every refusal of asx_xcorr_pool_phat_f32_dev, for k outside
 * 1..ASX_TOPK_MAX and for min_separation < 0.  batch == 0 returns 0.
 *   Cost: the bank fill and each group's row pass once per call; every further entry is one inverse column pass over the resident
 * Q' plus the tail, as in asx_xcorr_phat_topk_f32_dev.  Not offered: what that call does not offer. */
int asx_xcorr_pool_phat_topk_f32_dev(asx_plan *plan,
                                     const float *d_sources, size_t source_stride, size_t nsources,
                                     const float *d_samples, size_t sample_stride, size_t nsamples,
                                     const int32_t *d_pairs,
                                     const int64_t *d_windows, size_t window_stride, size_t batch,
                                     int64_t bin_lo, int64_t bin_hi, int k, int64_t min_separation,
                                     int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* The batched variant over several GPUs of one node from ONE process (BASELINE.json north_star; no
 * reference equivalent): plans[i] was created on device i (any devices; all the same sample_len); the
 * batch is block-partitioned over the plans, each block runs concurrently on its device, results come
 * back in pair order.  Pairs are independent: nothing is exchanged between devices.  (bench.py uses
 * one process per GPU and RCCL for the result gather instead; this is the entry point for C hosts.) */
int asx_xcorr_batch_multi(asx_plan *const *plans, int nplans, const float *source, const float *sample,
                          size_t batch, int64_t *lag, double *coef, int32_t *ret);

/* The same with DEVICE-RESIDENT shards and the result gather done by RCCL inside the library (one
 * host thread and one stream per device in a single process, ncclCommInitAll, one ncclAllGather per batch):
 *
 *   asx_shard_range(total, nshards, i, &start, &count)   block partition of a batch: the first total % nshards
 *                       shards hold one pair more (the rule bench.py's sharding.py uses between processes)
 *   asx_comm_create(plans, nplans)   one RCCL communicator over the plans' devices (all different, one plan each,
 *                       all the same sample_len); librccl.so.1 is dlopen()ed here, not linked: hosts that never
 *                       shard do not load it.  NULL on failure (asx_last_error()).
 *   asx_xcorr_batch_multi_dev(comm, d_source, d_sample, counts, width, d_gathered)
 *                       shard i = counts[i] <= width pairs resident on plans[i]'s device (d_source[i]: counts[i] * 2N
 *                       floats, d_sample[i]: counts[i] * N).  Every device runs its shard on its plan's stream from
 *                       its own host thread, then the shards' result records -- asx_result_bytes(width) bytes each
 *                       (20 * width rounded up to a multiple of 8, so that every record starts 8-byte aligned):
 *                       int64 lag[width] | double coef[width] | int32 ret[width], entries past counts[i] zero --
 *                       are all-gathered over xGMI: d_gathered[i] (device i, nplans * asx_result_bytes(width)
 *                       bytes) receives the record of every shard, in shard order.  Returns after all streams
 *                       have been synchronised.  The data path itself exchanges nothing: pairs are independent.
 *   asx_comm_destroy(comm) */
typedef struct asx_comm asx_comm;
int asx_shard_range(size_t total, int nshards, int shard, size_t *start, size_t *count);
size_t asx_result_bytes(size_t width);
asx_comm *asx_comm_create(asx_plan *const *plans, int nplans);
void asx_comm_destroy(asx_comm *comm);
int asx_xcorr_batch_multi_dev(asx_comm *comm, const float *const *d_source, const float *const *d_sample,
                              const size_t *counts, size_t width, void *const *d_gathered);

/* Debug/parity aid: run ONE device-resident pair and also return the raw
 * correlation r[0..2N) (device pointer, 2N floats; scaled by F/(2N) relative
 * to the reference when the length had to be embedded).  Like every entry point it
 * takes the second look at a pair whose near-tie list overflowed (exact mode, the
 * default) or marks it with ret = 1 (asx_plan_set_exact(plan, 0)), and leaves nothing
 * on the plan's overflow list either way; the coefficient is the direct form's. */
int asx_xcorr_debug_r_dev(asx_plan *plan, const float *d_source, const float *d_sample,
                          float *d_r, int64_t *d_lag, double *d_coef, int32_t *d_ret,
                          void *stream);

/* The same aid for asx_xcorr_phat_f32_dev: ONE contiguous pair under the plan's window, and the whole of r_phat to d_r: 2N floats,
 * unnormalised (F times the value that peak reports).  d_r, d_coef and d_ret must not be NULL; real-column plans only. */
int asx_xcorr_phat_debug_r_dev(asx_plan *plan, const float *d_source, const float *d_sample, float *d_r,
                               int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* ... and for asx_xcorr_phat_band_f32_dev: d_r is V times the value that peak reports (V: the number of bins that vote). */
int asx_xcorr_phat_band_debug_r_dev(asx_plan *plan, const float *d_source, const float *d_sample,
                                    int64_t bin_lo, int64_t bin_hi, float *d_r,
                                    int64_t *d_lag, double *d_coef, double *d_peak, int32_t *d_ret, void *stream);

/* pearson_coefficient() on two equal-length host double ranges. Writes the
 * coefficient (NaN for a constant range, like the reference). */
int asx_pearson_f64(const double *source_seg, const double *sample_seg, size_t n, int device,
                    double *coefficient);

/* ---- result consumers ---------------------------------------------------- */

/* What audiosync_run does with a result (src/audiosync.c:254-256,
 * include/audiosync/audiosync.h:21,24), for a whole batch on the device:
 *   accept[i]  = ret[i] == 0 && coef[i] >= min_confidence      (1 / 0)
 *   lag_ms[i]  = round(lag[i] * 1000 / sample_rate)            (C round(): halves away from zero)
 * All pointers are device pointers; d_accept may be NULL. Asynchronous on `stream`. */
int asx_results_to_ms_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret,
                          size_t batch, double min_confidence, double sample_rate,
                          int64_t *d_lag_ms, int32_t *d_accept, void *stream);

/* The entry to keep of each pair of a top-k call (asx_xcorr_topk_f32_dev, asx_xcorr_pool_topk_f32_dev), on the device: runner-ups are
 * asked for to pick by coefficient.  Per pair i over its entries j = 0..k-1 at index i*k + j: among the entries with ret == 0 the one
 * with the largest SIGNED coefficient wins (the acceptance above is signed: coef >= min_confidence), the smallest j among equal
 * coefficients; its (lag, coef, 0) go to index i of d_best_lag / d_best_coef / d_best_ret and j to d_best_entry[i].  When no entry of
 * the pair has ret == 0 (NaN coefficients, inexact, no lag left, an invalid row or pair), entry 0 is copied as it is and
 * d_best_entry[i] = 0.  The outputs have the layout asx_results_to_ms_dev takes.
 * All pointers are device pointers; d_best_lag and d_best_entry may be NULL, the others may not; k outside 1..ASX_TOPK_MAX or a NULL
 * pointer returns -1 before anything is launched.  Asynchronous on `stream`; allocates nothing. */
int asx_topk_best_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret,
                      size_t batch, int k,
                      int64_t *d_best_lag, double *d_best_coef, int32_t *d_best_ret, int32_t *d_best_entry,
                      void *stream);

/* Each pair's lag by triangle closure over a clip pool, and the clips placed: the consumer of an all-pairs top-k call that uses
 * more than one pair at a time.  asx_topk_best_dev picks by coefficient alone, which takes the wrong entry exactly where runner-ups
 * were asked for (a chorus, an echo, a loud private event); this call picks the entry that the other clips agree with.
 *   Input.  The outputs of asx_xcorr_pool_topk_f32_dev (or of asx_xcorr_pool_f32_dev, with k = 1) over ONE pool used as both sides
 * -- or those of asx_xcorr_pool_ncc_full_topk_f32_dev, the coefficient curve over signed lags, which a loud private event does not fool --,
 * with d_pairs == NULL and nsources = nsamples = C = nclips: pair (a, b) is index a * C + b, entry j of that pair is at
 * (a * C + b) * k + j.  With clip start times T (in frames of the common event), frame i of clip b is frame
 * i + T_b - T_a of clip a, and a lag l says sample[i] = source[i + l]: with clip a as the source and clip b as the sample, the lag
 * of pair (a, b) estimates T_b - T_a.  Hence lag_ac + lag_cb = (T_c - T_a) + (T_b - T_c) = lag_ab, and lag_ab = -lag_ba.  A caller
 * who computed only some pairs fills the others with ret != 0.
 *   The rule.  Everything is integer arithmetic, apart from coefficient comparisons; no result depends on the launch geometry.
 *   Valid entries.  An entry is valid when ret == 0 and |lag| <= ASX_CLOSURE_LAG_MAX; every sum below then fits an int64.
 *   Votes, of a valid entry (a, b, j) with a != b: one vote if some valid (b, a, q) has |lag_abj + lag_baq| <= tolerance; one vote
 * for each third clip c outside {a, b} for which valid (a, c, p) and (c, b, q) exist with |lag_acp + lag_cbq - lag_abj| <= tolerance.
 * Votes count clips, not combinations: the range is 0 .. C - 1.  Invalid entries and the diagonal get 0.  d_votes, if given,
 * receives all C * C * k values.
 *   Pick.  For each pair (a, b), scan j upwards over the valid entries: entry j replaces the current best when its votes are larger,
 * or when its votes are equal and coef[j] > coef[best] -- strictly, so a NaN never wins and the smallest j wins ties.  If the pair
 * has no valid entry, entry 0 is copied as it is and best_entry = 0.  (lag, coef, ret) of the pick go to index a * C + b of
 * d_best_lag / d_best_coef / d_best_ret and j to d_best_entry: the layout asx_results_to_ms_dev takes; the coefficient is copied
 * bit for bit.  On the diagonal this is asx_topk_best_dev's rule (votes are all 0); with k = 1 the pick is the identity.
 *   Confirm.  Let L be the picked lags.  Pair (a, b) is good when a != b and it has a valid entry.  d_confirm[a * C + b] is 0 for a
 * pair that is not good; for a good pair it is [(b, a) good and |L_ab + L_ba| <= tolerance] plus the number of c outside {a, b} with
 * (a, c) and (c, b) good and |L_ac + L_cb - L_ab| <= tolerance.  Here only the PICKED entries vote, so a pool in which every pair
 * picked the same periodic decoy confirms nothing.  A pair is usable when it is good and confirm >= min_confirm.
 *   Root.  If root is in [0, C), that clip is the root.  If root == -1, score[a] = #usable (a, .) + #usable (., a); the largest
 * score wins, and the smallest index wins among equals.  d_root[0] receives the root.
 *   Offsets.  The root r gets offset 0, support 0, placed 1.  Every other clip b has a multiset E_b of estimates of T_b - T_r:
 * L_rb if (r, b) is usable; -L_br if (b, r) is usable; and for every c outside {r, b}: L_rc + L_cb if both are usable, and
 * -(L_bc + L_cr) if both are usable.  d_offset[b] is the lower median of E_b, the element at index (|E_b| - 1) / 2 of E_b sorted
 * ascending; d_support[b] is the number of elements of E_b within tolerance of the median; d_placed[b] = 1 when E_b is not empty.
 * An empty E_b gives offset 0, support 0, placed 0.
 *   Ambiguity.  If every pair carries decoys at +-P, shifting one clip by P closes every triangle as well as the truth does, so lags
 * alone cannot decide: the votes of the true entries and of the decoys tie, and the pick falls back to the coefficient, which is
 * what asx_topk_best_dev does.  A wrong pick that no other pick agrees with has confirm 0: test d_confirm before trusting a pair.  The
 * converse does not hold: with periodic decoys in many pairs, two wrong picks one period off can confirm one another, so
 * confirm >= 1 is not proof that a pick is right; a larger min_confirm, and d_support against the number of clips, say more.
 *   Refusals: -1 with nothing launched and the outputs untouched for a NULL pointer other than d_votes; nclips == 0;
 * nclips * nclips * k > INT32_MAX; k outside 1..ASX_TOPK_MAX; tolerance < 0 or > ASX_CLOSURE_LAG_MAX; min_confirm < 0; root outside
 * [-1, nclips).  nclips == 1 is legal: it has the diagonal only and root 0.
 *   All pointers are device pointers: d_votes [C * C * k]; d_best_lag, d_best_coef, d_best_ret, d_best_entry, d_confirm [C * C] each;
 * d_root [1]; d_offset, d_support, d_placed [C] each.  The call takes no plan, allocates nothing, never synchronises the host, and is
 * asynchronous and capturable on `stream`: four kernel launches in order, each reading required outputs of those before it (there
 * is no workspace), so the outputs must not alias the inputs or one another.
 *   Not offered: clips reachable only over three or more hops are not placed (E_b holds one- and two-hop estimates; asx_pool_place_dev, below, walks longer chains from this call's outputs); a least-squares
 * solve over all pairs; an explicit pair list (unlisted pairs are stated by ret != 0); weighting by coefficient. */
#define ASX_CLOSURE_LAG_MAX ((int64_t)1 << 40)
int asx_pool_closure_dev(const int64_t *d_lag, const double *d_coef, const int32_t *d_ret,
                         size_t nclips, int k, int64_t tolerance, int min_confirm, int root,
                         int32_t *d_votes,
                         int64_t *d_best_lag, double *d_best_coef, int32_t *d_best_ret,
                         int32_t *d_best_entry, int32_t *d_confirm,
                         int32_t *d_root,
                         int64_t *d_offset, int32_t *d_support, int32_t *d_placed,
                         void *stream);

/* Every clip that a chain of usable pairs reaches, placed, and a verdict per pair: the consumer behind asx_pool_closure_dev for events
 * longer than a clip.  A pool pair is clip a's 2N frames against clip b's first N, so a true lag exists only for |T_b - T_a| < N: in
 * an event of more than about three clip lengths most pairs hold garbage, the truth lives in a band around the diagonal, and most
 * clips are three or more hops from any root, where closure's one- and two-hop estimates end.  This call walks the chains.
 *   Input.  d_lag, d_ret, d_confirm are closure's d_best_lag, d_best_ret, d_confirm ([C * C], pair (a, b) at index a * C + b, L_ab its
 * lag, an estimate of T_b - T_a) with the tolerance and min_confirm that call was given, or any tables of that layout.  d_root [1] is
 * closure's d_root or the caller's, in DEVICE memory: it is read when the kernels run, so closure followed by this call needs no
 * host step in between, and a replayed graph follows a root that changed.
 *   The rule.  Everything is int64 sums and integer counts; no output depends on the launch geometry.
 *   Usable, exactly as in asx_pool_closure_dev: usable(x, y) holds when x != y, ret == 0, |lag| <= ASX_CLOSURE_LAG_MAX and
 * confirm[x * C + y] >= min_confirm.
 *   Root.  r = d_root[0].  If r is outside [0, C), no clip is reached: every hops is -1, every state is 0 and everything else is 0.
 * Otherwise hops[r] = 0 and offset[r] = 0.
 *   Layers.  For h = 1 .. max_hops and every clip b not yet reached, E_b is the multiset of o[c] + L_cb over the clips c with
 * 0 <= hops[c] < h and usable(c, b), and of o[c] - L_bc over the clips c with 0 <= hops[c] < h and usable(b, c).  If E_b is not
 * empty, hops[b] = h and offset[b] is the lower median of E_b, the element at index (|E_b| - 1) / 2 of E_b sorted ascending
 * (closure's definition).  By the breadth-first property the neighbours that count at layer h all lie in layer h - 1.  A median over
 * them, not a spanning tree: one wrong pick cannot carry a clip away while it is outvoted.  A clip never reached has hops -1,
 * offset 0, support 0, degree 0 and step 0.
 *   Sweeps, a Jacobi median relaxation over all usable pairs.  For s = 1 .. sweeps, every clip b with hops > 0 takes the lower
 * median of o_{s-1}[c] + L_cb and o_{s-1}[c] - L_bc over ALL reached c with the pair usable; all clips read the offsets of the sweep
 * before; the root stays 0.  d_step[b] = o_s[b] - o_{s-1}[b] of the last sweep, and 0 for the root, for a clip that was not reached
 * and when sweeps == 0: all of d_step zero says the offsets are a fixed point.  |offset| <= (max_hops + sweeps) * 2^40 < 2^52.
 *   What sweeps do not do.  Along a chain without redundancy, +-1 frame of jitter per pair adds up to about one frame per hop, and
 * no sweep shrinks that: sweeps only bring in the pairs to clips of the same and of later layers.  Without sweeps a clip's error is
 * bounded by its own hops times the jitter, with sweeps by the largest hops of the pool.
 *   Per clip, with the final offsets o, for every reached clip, the root included: d_degree[b] = |E_b| over ALL reached neighbours,
 * d_support[b] = the number of those elements within tolerance of o[b].
 *   Per pair (a, b): when usable(a, b) and both ends are reached, d_resid = L_ab - (o[b] - o[a]) and d_state = 1 if |resid| <=
 * tolerance, 2 if not; anything else, the diagonal included: state 0, resid 0.  The pairs of state 2 are the ones to run again under a
 * lag window around o[b] - o[a].
 *   The input decides.  In a large pool random garbage lags close triangles by accident and come out usable (hundreds of pairs at
 * C = 300, k = 2, min_confirm = 1), and a clip reached over such a pair alone lands anywhere.  Mask the pairs you do not believe --
 * ret != 0, a coefficient or peak threshold, a larger min_confirm -- and read d_state and d_support against d_degree.
 *   Refusals: -1 with nothing launched and the outputs untouched for a NULL pointer other than d_scratch when sweeps == 0;
 * nclips == 0; nclips * nclips > INT32_MAX; tolerance < 0 or > ASX_CLOSURE_LAG_MAX; min_confirm < 0; max_hops outside
 * [1, ASX_PLACE_HOPS_MAX]; sweeps outside [0, ASX_PLACE_SWEEPS_MAX].  nclips == 1 is legal.
 *   All pointers are device pointers: d_scratch, d_offset, d_hops, d_support, d_degree, d_step [C] each; d_resid, d_state [C * C] each.
 * The call takes no plan, allocates nothing, needs no workspace beyond d_scratch (which may be NULL iff sweeps == 0), never
 * synchronises the host, and is asynchronous and capturable on `stream`: 2 + max_hops + sweeps kernel launches whatever the tables
 * hold, none of which waits for another block; a layer behind the last one that placed a clip costs a launch whose blocks leave at
 * once.  It keeps its state between launches in the outputs and resets it: they may be dirty, and a second call or a replay gives the
 * same bytes.  The outputs must not alias the inputs or one another.
 *   Not offered: components other than the root's (call again with a clip of hops -1 as the root); weighting by coefficient; a
 * floating-point least-squares solve. */
#define ASX_PLACE_HOPS_MAX   1024
#define ASX_PLACE_SWEEPS_MAX 64
int asx_pool_place_dev(const int64_t *d_lag, const int32_t *d_ret, const int32_t *d_confirm,
                       size_t nclips, int64_t tolerance, int min_confirm,
                       const int32_t *d_root,
                       int max_hops, int sweeps,
                       int64_t *d_scratch,
                       int64_t *d_offset, int32_t *d_hops, int32_t *d_support, int32_t *d_degree, int64_t *d_step,
                       int64_t *d_resid, int32_t *d_state,
                       void *stream);

/* The exact correlation curve and a fractional lag around given lags: a consumer that runs behind the batch, strided, windowed, top-k
 * and pool calls on the lags they returned.  Those calls rank lags by the raw correlation r and hand back one coefficient per lag;
 * this one says how sharp a candidate is: r and the Pearson coefficient at the 2h + 1 indices around it, and the parabola's vertex.
 * It needs no transform -- r at an index is the time-domain sum r[idx] = sum_{n<N} source[(n + idx) mod 2N] * sample[n], the quantity
 * the exact re-evaluation computes -- so it runs on every plan, packed ones included.
 *   Inputs.  Pair i's inputs are exactly those of asx_xcorr_strided_f32_dev: strides in floats, a stride of 0 broadcasts, strides
 * below the track length are allowed.  Real-column plans keep the 16-byte layout rule (16-byte aligned base pointers, every stride a
 * multiple of 4 floats); packed plans take any float-aligned pointer and any stride.  1 <= entries <= ASX_TOPK_MAX.  Entry
 * e = i * entries + j belongs to pair i = e / entries; its centre is the lag d_center[e] (int64, device memory, read when the kernels
 * run), in the convention of every d_lag output: the d_lag of a top-k call with k = entries can be passed straight in, and
 * entries = 1 serves the other calls.  1 <= half_width <= ASX_NEAR_MAX.
 *   Outputs, with h = half_width, n = 2h + 1 and p the centre's index (lag l >= 0 is index l, lag l < 0 index 2N + l):
 *   d_r[e * n + (d + h)] = r[(p + d) mod 2N] for d = -h .. h: the plain sum above in float64 (products of two float32 values are exact
 * in float64), unnormalised and signed.  Neighbours are taken in index space, circularly: index 2N - 1 (lag -1) sits beside index 0,
 * and index N (lag -N) beside index N - 1.  Every value is within N * 2^-53 * sum_n |source * sample| (over the terms of its index)
 * of the exact sum.
 *   d_coef[e * n + (d + h)] = the reference's Pearson coefficient at that index's lag, after the wrap and with the segments of
 * src/cross_correlation.c:256-272, always in the direct form: bit for bit what asx_xcorr_windowed_f32_dev returns on the same plan for
 * that pair with the row [l, l] under asx_plan_set_pearson(plan, 0) (the precedent of the top-k call's later entries), and NaN where
 * that call's coefficient is NaN (the empty segment at lag -N, a constant segment).  d_coef may be NULL: no Pearson pass runs then.
 *   d_frac[e] = the vertex of the parabola through the three centre values of d_r, by the rule and in the operation order stated for
 * asx_xcorr_phat_sub_f32_dev: s by the sign of y0, den = (a - 2 b) + c, 0 when den >= 0, clamped to [-0.5, 0.5], NaN when any of the
 * three is NaN.
 *   d_ret[e] = 0 for a computed entry, -2 for a centre outside [-N, N-1].  A -2 entry gets NaN in frac and in all n values of r and
 * coef, and reads nothing; the other entries are untouched, bit for bit.
 *   Every value of an entry is independent of the batch size and of the entry's position in the batch (a fixed reduction tree).
 *   Refusals: a NULL plan, track, d_center, d_r, d_frac or d_ret, entries or half_width out of range, and the layout rule on a
 * real-column plan return -1 with nothing launched and the outputs untouched.  batch == 0 returns 0.
 *   What the call never does.  It allocates nothing after plan creation (asx_plan_workspace_bytes stays the same), never
 * synchronises the host and touches no counter: overflows, repairs, Pearson modes, prune and qstore stats stay unchanged.  It behaves
 * the same whatever asx_plan_set_exact, asx_plan_set_pearson, asx_plan_set_prune or the plan's lag window say.  It uses the plan's
 * lane workspaces, so the one-stream-at-a-time rule of asx_xcorr_batch_f32_dev applies.
 *   Cost.  r and frac: one pass over each entry's tracks, 8N bytes, for all n sums (a block's stretch of the source goes through LDS
 * once, with a halo of 2h).  The coefficient curve: one direct Pearson pass per neighbour, n passes per entry; d_coef == NULL skips
 * them.  Measured: DESIGN.md. */
int asx_xcorr_curve_f32_dev(asx_plan *plan,
                            const float *d_source, size_t source_stride,
                            const float *d_sample, size_t sample_stride,
                            size_t batch, int entries, const int64_t *d_center, int half_width,
                            double *d_r, double *d_coef, double *d_frac, int32_t *d_ret, void *stream);

/* ... for pairs of two track pools: the inputs of asx_xcorr_pool_f32_dev -- the pools, which may alias or overlap, strides that may be
 * below the track length, d_pairs == NULL = every combination source-major, batch then nsources * nsamples -- with entries,
 * d_center, half_width and the outputs of asx_xcorr_curve_f32_dev: each entry is what that call returns for the pair's two tracks.
 * Real-column plans only, as every pool call.  It never touches, fills or grows the bank: it reads the tracks themselves.
 *   d_ret[e] = -4 for an entry whose pair's row names a track outside its pool (over -2): NaN in frac and in all its values of r and
 * coef, nothing read outside the pools, the other entries untouched, bit for bit.
 *   Returns -1 with the outputs untouched and nothing launched on the refusals of asx_xcorr_curve_f32_dev and on every refusal of
 * asx_xcorr_pool_f32_dev that does not concern the bank (a NULL pool; an empty pool while batch > 0; not a real-column plan;
 * alignment; strides that are not multiples of 4 floats; d_pairs == NULL with batch != nsources * nsamples).  batch == 0 returns 0. */
int asx_xcorr_pool_curve_f32_dev(asx_plan *plan,
                                 const float *d_sources, size_t source_stride, size_t nsources,
                                 const float *d_samples, size_t sample_stride, size_t nsamples,
                                 const int32_t *d_pairs,
                                 size_t batch, int entries, const int64_t *d_center, int half_width,
                                 double *d_r, double *d_coef, double *d_frac, int32_t *d_ret, void *stream);

/* A lag track: the exact r per time segment around given lags, and a drift fit.  Every other call returns one lag for a whole window
 * of N frames, which assumes that the lag is constant over the window.  Two recorders never share a clock: at 20 - 100 ppm of
 * relative drift the lag moves by dozens of frames across a 30 s window and a whitened peak smears away.  This call is the curve
 * call's sibling, a consumer behind any call on the lags it returned: it keeps the curve's sum apart per stretch of time, over a lag
 * range wide enough to hold a drifting peak -- r as a function of (time segment, lag) -- and fits a line through its ridge.  It runs
 * no transform and no launch group, so it works on every plan, packed ones included.
 *   Inputs: exactly those of asx_xcorr_curve_f32_dev -- strides in floats, a stride of 0 broadcasts, strides below the track length
 * are allowed; the 16-byte layout rule on real-column plans only; 1 <= entries <= ASX_TOPK_MAX; entry e = i * entries + j belongs
 * to pair i; d_center[e] is a lag in the d_lag convention, read when the kernels run.  1 <= half_width <= ASX_TRACK_HALF_MAX.
 * 1 <= segments <= min(ASX_TRACK_SEG_MAX, N).
 *   Definitions, with h = half_width, n = 2h + 1, S = segments and p the centre's index (lag l >= 0 is index l, lag l < 0 index
 * 2N + l): segment s covers the sample's frames [b_s, b_{s+1}) with b_s = floor(s * N / S) in 64-bit integers; its time is
 * t_s = (b_s + b_{s+1} - 1) / 2, the mean frame index, exact in float64.
 *   d_r[(e * S + s) * n + (d + h)] = r_s[d] = sum_{n in segment s} source[(n + p + d) mod 2N] * sample[n] for d = -h .. h: in float64
 * (products of two float32 values are exact), signed and unnormalised; neighbours are circular in index space, as in the curve
 * call.  Each value is within len_s * 2^-53 * sum |products of its terms| of the exact sum, and over s the sums add up to the curve
 * call's r[(p + d) mod 2N].
 *   d_seg[(e * S + s) * 2 + {0, 1}] = {off_s, w_s}.  m_s is the d with the largest |r_s[d]|, scanned from d = -h upwards with fabs
 * and a strict >: the smallest d wins ties and an all-zero segment gives -h.  w_s = |r_s[m_s]|.  An interior peak, -h < m_s < h:
 * off_s = (double)m_s + frac, one add, with frac the parabola rule of asx_xcorr_phat_sub_f32_dev on r_s[m_s - 1], r_s[m_s],
 * r_s[m_s + 1].  At an edge off_s = -h or +h exactly.  A segment is used when its peak is interior and all of its n values are
 * finite.  d_seg may be NULL.  It is offered so that a caller can fit robustly themselves (a median slope, an outlier cut) where
 * the weighted line below is not what they want.
 *   d_used[e] = the number of used segments.
 *   d_fit[e * 3 + {0, 1, 2}] = {drift, lag0, rms}: the weighted least-squares line through (t_s, off_s) over the used segments with
 * weights w_s, in float64, the used segments taken in ascending s: W = sum w, tbar = sum w t / W, ybar = sum w off / W,
 * Stt = sum w (t - tbar)^2, Sty = sum w (t - tbar)(off - ybar), drift = Sty / Stt, lag0 = ybar - drift * tbar,
 * rms = sqrt(sum w (off - (lag0 + drift * t))^2 / W).  With fewer than two used segments all three are NaN: segments = 1 is a wide
 * curve with no fit.  Meaning: sample frame n lines up with source frame n + center + lag0 + drift * n, so 1e6 * drift is the clock
 * offset in ppm.  Within a segment the lag still moves: a segment smears by drift * N / S frames, so pick S large enough that this
 * stays near or below one frame for the drift you expect, and half_width large enough to hold drift * N / 2 on either side.
 *   d_ret[e] = 0, or -2 for a centre outside [-N, N-1]: such an entry gets NaN in all of its r, seg and fit values and used = 0, and
 * reads nothing; the other entries are untouched, bit for bit.
 *   Refusals: a NULL plan, track, d_center, d_r, d_fit, d_used or d_ret, entries, half_width or segments out of range, and the curve
 * call's layout refusals return -1 with nothing launched and the outputs untouched.  batch == 0 returns 0.
 *   What the call never does.  It allocates nothing after plan creation (asx_plan_workspace_bytes stays the same), never
 * synchronises the host, and touches no counter and no bank.  It behaves the same whatever asx_plan_set_exact,
 * asx_plan_set_pearson, asx_plan_set_prune, asx_plan_set_qstore or the plan's lag window say.  It uses the plan's lane workspaces,
 * so the one-stream-at-a-time rule of asx_xcorr_batch_f32_dev applies.  Every value of an entry is independent of the batch size,
 * of the entry's position in the batch and of the plan's max_batch: the reduction tree is fixed by N, S and h alone.
 *   Cost: one pass over the entry's tracks, 8N bytes, per tile of 17 lags (h = 8: one pass, h = 64: eight).  Measured: DESIGN.md. */
#define ASX_TRACK_HALF_MAX 64
#define ASX_TRACK_SEG_MAX  64
int asx_xcorr_track_f32_dev(asx_plan *plan,
                            const float *d_source, size_t source_stride,
                            const float *d_sample, size_t sample_stride,
                            size_t batch, int entries, const int64_t *d_center, int half_width, int segments,
                            double *d_r, double *d_seg, double *d_fit, int32_t *d_used, int32_t *d_ret, void *stream);

/* ... for pairs of two track pools: the pools, d_pairs and batch of asx_xcorr_pool_curve_f32_dev with the remaining arguments and
 * the outputs of asx_xcorr_track_f32_dev.  Real-column plans only, as every pool call.  It never touches, fills or grows the bank.
 *   d_ret[e] = -4 for an entry whose pair's row names a track outside its pool (over -2): NaN in all of its r, seg and fit values,
 * used = 0, nothing read outside the pools, the other entries untouched, bit for bit.
 *   Returns -1 with the outputs untouched and nothing launched on the refusals of asx_xcorr_track_f32_dev and on the pool refusals of
 * asx_xcorr_pool_curve_f32_dev.  batch == 0 returns 0. */
int asx_xcorr_pool_track_f32_dev(asx_plan *plan,
                                 const float *d_sources, size_t source_stride, size_t nsources,
                                 const float *d_samples, size_t sample_stride, size_t nsamples,
                                 const int32_t *d_pairs,
                                 size_t batch, int entries, const int64_t *d_center, int half_width, int segments,
                                 double *d_r, double *d_seg, double *d_fit, int32_t *d_used, int32_t *d_ret, void *stream);

/* A warped correlation: the exact r and the Pearson coefficient along a drift line.  The track call reports how fast the lag moves;
 * every coefficient of the other calls is the reference's Pearson coefficient at one constant lag, and on a drifting pair it
 * collapses although the tracks match (white noise, 12 frames of drift over the window: 0.11 - 0.16 at the best constant lag, 1.0
 * along the line).  This call takes the line and computes along it: the exact correlation around the line, the parabola vertex
 * across it, and the reference's Pearson coefficient of the frames that line up -- a confidence that asx_results_to_ms_dev can
 * test.  It is a consumer behind the track call, in one pass over the two tracks; it runs no transform and no launch group, so it
 * works on every plan, packed ones included.
 *   Inputs: exactly those of asx_xcorr_curve_f32_dev -- strides in floats, a stride of 0 broadcasts, strides below the track length
 * are allowed; the 16-byte layout rule on real-column plans only; 1 <= entries <= ASX_TOPK_MAX; entry e = i * entries + j belongs
 * to pair i; d_center[e] is a lag in the d_lag convention; 1 <= half_width <= ASX_NEAR_MAX.  Entry e's line is
 * a = d_line[e * line_stride] (the drift, in frames per frame) and b = d_line[e * line_stride + 1] (lag0, in frames): sample frame
 * n meets source frame n + center + lag0 + drift * n, rounded to the nearest frame.  line_stride counts doubles: 3 passes the track
 * call's d_fit straight in, 2 is a packed array of lines, 0 is one line for every entry, 1 is refused.  Centres and lines are read
 * when the kernels run.
 *   Definitions, with N the plan's sample_len, h = half_width, c = d_center[e] and p the centre's index (lag l >= 0 is index l, lag
 * l < 0 index 2N + l).
 *   The shift: k_n = floor((b + a * (double)n) + 0.5) as an int64, all in float64, the multiply, the two adds and the floor each
 * rounded on their own, no fused multiply-add: numpy's np.floor((b + a * n) + 0.5) is the same integer for every n.
 *   A valid line: a and b finite, |a| <= ASX_WARP_DRIFT_MAX and |b| <= N.  Then n + k_n is non-decreasing, four consecutive frames
 * hold at most one step and a sweep of 1024 frames spans at most 17 steps.
 *   d_r[e * (2h + 1) + (d + h)] = sum_{n<N} source[(n + p + d + k_n) mod 2N] * sample[n] for d = -h .. h, the mod mathematical
 * (never negative): in float64 (products of two float32 values are exact), signed and unnormalised; circular in index space, as
 * in the curve call.  Each value is within N * 2^-53 * sum |products of its terms| of the exact sum.  The line (0, 0) gives the
 * curve call's r.
 *   d_frac[e] = the parabola rule of asx_xcorr_phat_sub_f32_dev on the three centre values of d_r: the vertex across the line.
 *   The lined-up frames: u_n = n + c + k_n, linear with no wrap, for d = 0; V = {n in [0, N) : 0 <= u_n < 2N}, one contiguous
 * range; d_len[e] = |V|.  d_len may be NULL.  For the line (0, 0) V is the reference's segment for the lag c
 * (src/cross_correlation.c:256-271).
 *   d_coef[e] = pearson_coefficient() (src/cross_correlation.c:74-116) over the pairs (source[u_n], sample[n]), n in V: in float64
 * from the float32 samples in the direct form, partial statistics with the exact pairwise merge of the direct Pearson kernels.  NaN
 * when V is empty or a side is constant.
 *   d_ret[e] = 0 for a computed entry; -1 when the coefficient is NaN (r, frac and len are still written), so that (d_center,
 * d_coef, d_ret) feed asx_results_to_ms_dev as they stand; -2 for a centre outside [-N, N-1]; -5 for a line that is not valid,
 * the NaN line that the track call returns with fewer than two used segments included.  -2 takes precedence over -5.  Such an
 * entry gets NaN in r, frac and coef and len = 0, and reads nothing; the other entries are untouched, bit for bit.
 *   Refusals: a NULL plan, track, d_center, d_line, d_r, d_frac, d_coef or d_ret, entries or half_width out of range,
 * line_stride == 1, and the curve call's layout refusals return -1 with nothing launched and the outputs untouched.  batch == 0
 * returns 0.
 *   What the call never does.  It allocates nothing after plan creation (asx_plan_workspace_bytes stays the same), never
 * synchronises the host, and touches no counter and no bank.  It behaves the same whatever asx_plan_set_exact,
 * asx_plan_set_pearson, asx_plan_set_prune, asx_plan_set_qstore or the plan's lag window say.  It uses lane 0's records and psums,
 * so the one-stream-at-a-time rule of asx_xcorr_batch_f32_dev applies.  Every value of an entry is independent of the batch size,
 * of the entry's position in the batch and of the plan's max_batch: the reduction tree is fixed by N alone.
 *   What is not offered: interpolation between frames (nearest frame only: the sums stay exact products of stored samples, and at
 * the drifts of real clocks a frame is repeated or dropped once in 10^4 or more), a coefficient for d != 0, a piecewise path
 * through the track call's d_seg.
 *   Cost: one pass over the entry's tracks, 8N bytes.  Measured: DESIGN.md. */
#define ASX_WARP_DRIFT_MAX 0.015625   /* 2^-6 */
int asx_xcorr_warp_f32_dev(asx_plan *plan,
                           const float *d_source, size_t source_stride,
                           const float *d_sample, size_t sample_stride,
                           size_t batch, int entries, const int64_t *d_center,
                           const double *d_line, size_t line_stride, int half_width,
                           double *d_r, double *d_frac, double *d_coef, int64_t *d_len, int32_t *d_ret, void *stream);

/* ... for pairs of two track pools: the pools, d_pairs and batch of asx_xcorr_pool_curve_f32_dev with the remaining arguments and
 * the outputs of asx_xcorr_warp_f32_dev.  Real-column plans only, as every pool call.  It never touches, fills or grows the bank.
 *   d_ret[e] = -4 for an entry whose pair's row names a track outside its pool (over -2, which is over -5): NaN in r, frac and
 * coef, len = 0, nothing read outside the pools, the other entries untouched, bit for bit.
 *   Returns -1 with the outputs untouched and nothing launched on the refusals of asx_xcorr_warp_f32_dev and on the pool refusals of
 * asx_xcorr_pool_curve_f32_dev.  batch == 0 returns 0. */
int asx_xcorr_pool_warp_f32_dev(asx_plan *plan,
                                const float *d_sources, size_t source_stride, size_t nsources,
                                const float *d_samples, size_t sample_stride, size_t nsamples,
                                const int32_t *d_pairs,
                                size_t batch, int entries, const int64_t *d_center,
                                const double *d_line, size_t line_stride, int half_width,
                                double *d_r, double *d_frac, double *d_coef, int64_t *d_len, int32_t *d_ret, void *stream);

/* ---- growing-window (streaming) mode ------------------------------------ */

/* The reference re-runs the whole correlation on growing prefixes of the two
 * tracks (3, 6, 10, 15, 20, 30 s; src/audiosync.c:50-57,226-259) and rebuilds
 * plans and buffers every time.  A stream keeps both tracks resident in HBM:
 * only NEW frames are uploaded (as the producers' f64le doubles,
 * src/capture/linux_capture.c:370, and converted to float32 on the device),
 * and one plan per prefix length is built once and reused. */
typedef struct asx_stream asx_stream;

/* Capacity: sample track max_sample_len frames, source track 2*max_sample_len. */
asx_stream *asx_stream_create(size_t max_sample_len, int device);
void asx_stream_destroy(asx_stream *stream);
/* Append frames to the tracks (either count may be 0). -1 if capacity would be exceeded. */
int asx_stream_append_f64(asx_stream *stream, const double *source_frames, size_t n_source,
                          const double *sample_frames, size_t n_sample);
/* Frames appended so far. */
int asx_stream_lengths(const asx_stream *stream, size_t *n_source, size_t *n_sample);
/* Forget all frames (plans stay). */
int asx_stream_reset(asx_stream *stream);
/* cross_correlation() on the prefixes source[0,2*sample_len), sample[0,sample_len) that are
 * already resident.  Same return convention as asx_xcorr_f64.  -1 (outputs untouched) if
 * fewer frames than that have been appended. */
int asx_stream_xcorr(asx_stream *stream, size_t sample_len, long *lag, double *coefficient);
/* The lag window (asx_plan_set_lag_window) of every later asx_stream_xcorr, in frames: clamped to [-n, n-1] for each
 * prefix length n it correlates.  Default: unbounded.  -1 when lag_min > lag_max. */
int asx_stream_set_lag_window(asx_stream *stream, int64_t lag_min, int64_t lag_max);

/* ---- synthetic inputs and timing -------------------------------------- */

/* Fill device buffers with pairs [first_pair, first_pair+count) of the
 * deterministic generator specified in oracle/xcorr_oracle.h (bit-identical
 * to oracle_synth_pair).  d_true_lag may be NULL. */
int asx_synth_pairs_dev(uint64_t seed, uint64_t first_pair, size_t count, size_t sample_len,
                        int noise_shift, float *d_source, float *d_sample, int64_t *d_true_lag,
                        void *stream);

/* Milliseconds spent by recent asx_xcorr_batch_f32_dev calls on `plan`, per kernel family, measured
 * with HIP events on the stream the kernels ran on.  asx_plan_set_profiling(plan, depth): depth > 0
 * keeps the events of the last `depth` calls (so that consecutive steps can be timed with no host
 * synchronisation between them), 0 switches profiling off.  asx_plan_timings_ms(plan, calls_back, out):
 * the call `calls_back` calls ago (0 = the latest); asx_plan_last_timings_ms = calls_back 0.
 * out[0..5] = fwd_cols, rows, inv_cols, finalize (+ exact re-evaluation), pearson, total. */
int asx_plan_set_profiling(asx_plan *plan, int depth);
int asx_plan_timings_ms(asx_plan *plan, int calls_back, float out[6]);
int asx_plan_last_timings_ms(asx_plan *plan, float out[6]);

/* Raw device memory helpers so a C host (no torch) can stage buffers. */
void *asx_device_malloc(size_t bytes, int device);
int asx_device_free(void *ptr);
/* Page-locked host memory: frames appended from it (asx_stream_append_f64) or passed to the host-array entry points travel
 * by DMA without the runtime's bounce buffer.  The track buffers of audiosync_run() are allocated with it -- what
 * fftw_alloc_real was to the reference's source buffer (src/audiosync.c:189): the allocation its backend wants. */
void *asx_host_malloc(size_t bytes);
int asx_host_free(void *ptr);
int asx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int asx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int asx_stream_sync(asx_plan *plan, void *stream);

#ifdef __cplusplus
}
#endif
#endif
