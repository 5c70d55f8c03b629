"""old-audiosync_amd — MI355X (gfx950) implementation of ONE path of
vidify/old-audiosync: the FFT cross-correlation of src/cross_correlation.c.

The product is native: csrc/ (hand-written HIP kernels behind the C-ABI of
include/audiosync/xcorr_hip.h -> libaudiosync_hip.so) and host/ (plain C, the
reference's own API -> libaudiosync.so, and the CPython module `audiosync`).
This Python package is only a thin ctypes view of that C-ABI for tests, the
benchmark and notebooks.  There is no CPU fallback: loading fails loudly when
the library has not been built, and every call fails when no GPU works.

The directory name contains a hyphen, so import it with `load()` from
__graft_entry__.py (importlib), e.g.  `asx = __graft_entry__.load()`.
"""
from .hipxcorr import (  # noqa: F401
    LIB_PATH, AsxError, Plan, Stream, abi_version, device_count, lib, pearson_f64, planmath_candidates, planmath_describe, planmath_group_form, planmath_kernel_table, planmath_kernels,
    planmath_table, planmath_twiddles, band_bins, results_to_ms_dev, synth_pairs_dev, topk_best_dev, xcorr_batch_multi,
    Comm, PinnedArray, result_bytes, shard_range, closure_args, pool_closure, pool_closure_dev, phat_topk_args, pool_phat_topk_args,
    NCC_MIN_ENERGY, ncc_args, ncc_topk_args, pool_ncc_args, pool_ncc_topk_args,
    ncc_full_args, ncc_full_topk_args, pool_ncc_full_args, pool_ncc_full_topk_args,
    ncc_ragged_args, ncc_ragged_topk_args, ragged_pack,
    PLACE_HOPS_MAX, PLACE_SWEEPS_MAX, place_args, pool_place, pool_place_dev,
)
