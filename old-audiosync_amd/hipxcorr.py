"""ctypes view of libaudiosync_hip.so (the C-ABI in include/audiosync/xcorr_hip.h)."""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaudiosync_hip.so")
_lib = None

c_f32p = ctypes.POINTER(ctypes.c_float)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_intp = ctypes.POINTER(ctypes.c_int)

_vp, _sz, _int, _i64, _u64, _dbl, _str = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64,
                                          ctypes.c_double, ctypes.c_char_p)
_vpp, _szp, _longp = ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_long)
_u32p, _u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

# name -> (restype, argtypes) of every function include/audiosync/xcorr_hip.h declares; lib() applies it, ABI_SYMBOLS lists it, and
# tests/test_binding_signatures.py holds it against the header's prototypes
_HEADER_SIGNATURES = {
    "asx_device_count": (_int, []),
    "asx_current_device": (_int, []),
    "asx_last_error": (_str, []),
    "asx_abi_version": (_int, []),
    "asx_plan_create": (_vp, [_sz, _sz, _int]),
    "asx_plan_create_ex": (_vp, [_sz, _sz, _int, _str]),
    "asx_plan_destroy": (None, [_vp]),
    "asx_plan_sample_len": (_sz, [_vp]),
    "asx_plan_fft_len": (_sz, [_vp]),
    "asx_plan_group": (_sz, [_vp]),
    "asx_plan_workspace_bytes": (_sz, [_vp]),
    "asx_plan_peak_capacity": (_sz, [_vp]),
    "asx_plan_threads": (_int, [_vp, c_intp, c_intp]),
    "asx_plan_split": (_int, [_vp, c_intp, c_intp, c_intp]),
    "asx_plan_layout": (_int, [_vp]),
    "asx_plan_peak_overflows": (_int, [_vp, _u64p]),
    "asx_plan_peak_repairs": (_int, [_vp, _u64p]),
    "asx_plan_narrowed_calls": (_int, [_vp, _u64p]),
    "asx_plan_set_exact": (_int, [_vp, _int]),
    "asx_plan_set_lag_window": (_int, [_vp, _i64, _i64]),
    "asx_plan_lag_window": (_int, [_vp, c_i64p, c_i64p]),
    "asx_stream_set_lag_window": (_int, [_vp, _i64, _i64]),
    "asx_plan_placement": (_int, [_vp, c_f64p, c_intp]),
    "asx_plan_set_pearson": (_int, [_vp, _int]),
    "asx_plan_pearson_modes": (_int, [_vp, _u64p]),
    "asx_plan_set_prune": (_int, [_vp, _int]),
    "asx_plan_prune_stats": (_int, [_vp, _u64p, _u64p]),
    "asx_plan_set_qstore": (_int, [_vp, _int]),
    "asx_plan_qstore_stats": (_int, [_vp, _u64p]),
    "asx_plan_set_profiling": (_int, [_vp, _int]),
    "asx_plan_last_timings_ms": (_int, [_vp, c_f32p]),
    "asx_plan_timings_ms": (_int, [_vp, _int, c_f32p]),
    "asx_xcorr_f64": (_int, [_vp, c_f64p, c_f64p, _longp, c_f64p]),
    "asx_xcorr_batch_f32": (_int, [_vp, c_f32p, c_f32p, _sz, c_i64p, c_f64p, c_i32p]),
    "asx_xcorr_batch_multi": (_int, [_vpp, _int, c_f32p, c_f32p, _sz, c_i64p, c_f64p, c_i32p]),
    "asx_xcorr_batch_f32_dev": (_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "asx_xcorr_strided_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "asx_xcorr_windowed_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "asx_xcorr_topk_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _int, _i64, _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_debug_c_dev": (_int, [_vp, _vp, _vp, _dbl, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_topk_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _int, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_ncc_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_ncc_topk_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _dbl, _int, _i64, _vp, _vp, _vp, _vp,
                                               _vp]),
    "asx_xcorr_ncc_full_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_full_topk_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _i64, _int, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_full_debug_c_dev": (_int, [_vp, _vp, _vp, _dbl, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_ragged_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_ncc_ragged_topk_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _dbl, _i64, _int, _i64, _vp, _vp, _vp,
                                                 _vp, _vp]),
    "asx_xcorr_ncc_ragged_debug_c_dev": (_int, [_vp, _vp, _vp, _i64, _i64, _dbl, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_ncc_full_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _dbl, _i64, _vp, _vp, _vp, _vp,
                                               _vp]),
    "asx_xcorr_pool_ncc_full_topk_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _dbl, _i64, _int, _i64, _vp,
                                                    _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_band_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_sub_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_topk_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _i64, _i64, _int, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_topk_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _int, _i64, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_phat_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_phat_sub_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _i64, _i64, _int, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp]),
    "asx_xcorr_pool_phat_topk_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _sz, _i64, _i64, _int, _i64, _vp, _vp,
                                                _vp, _vp, _vp]),
    "asx_xcorr_curve_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _sz, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_curve_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_track_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _sz, _int, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_track_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _int, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp,
                                            _vp]),
    "asx_xcorr_warp_f32_dev": (_int, [_vp, _vp, _sz, _vp, _sz, _sz, _int, _vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_pool_warp_f32_dev": (_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp, _sz, _int, _vp, _vp, _sz, _int, _vp, _vp, _vp, _vp,
                                           _vp, _vp]),
    "asx_xcorr_debug_r_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_debug_r_dev": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_xcorr_phat_band_debug_r_dev": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_band_bins": (_int, [_sz, _dbl, _dbl, _dbl, c_i64p, c_i64p]),
    "asx_pearson_f64": (_int, [c_f64p, c_f64p, _sz, _int, c_f64p]),
    "asx_results_to_ms_dev": (_int, [_vp, _vp, _vp, _sz, _dbl, _dbl, _vp, _vp, _vp]),
    "asx_topk_best_dev": (_int, [_vp, _vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _vp]),
    "asx_pool_closure_dev": (_int, [_vp, _vp, _vp, _sz, _int, _i64, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_pool_place_dev": (_int, [_vp, _vp, _vp, _sz, _i64, _int, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "asx_synth_pairs_dev": (_int, [_u64, _u64, _sz, _sz, _int, _vp, _vp, _vp, _vp]),
    "asx_shard_range": (_int, [_sz, _int, _int, _szp, _szp]),
    "asx_result_bytes": (_sz, [_sz]),
    "asx_comm_create": (_vp, [_vpp, _int]),
    "asx_comm_destroy": (None, [_vp]),
    "asx_xcorr_batch_multi_dev": (_int, [_vp, _vpp, _vpp, _szp, _sz, _vpp]),
    "asx_stream_create": (_vp, [_sz, _int]),
    "asx_stream_destroy": (None, [_vp]),
    "asx_stream_append_f64": (_int, [_vp, c_f64p, _sz, c_f64p, _sz]),
    "asx_stream_lengths": (_int, [_vp, _szp, _szp]),
    "asx_stream_reset": (_int, [_vp]),
    "asx_stream_xcorr": (_int, [_vp, _sz, _longp, c_f64p]),
    "asx_device_malloc": (_vp, [_sz, _int]),
    "asx_device_free": (_int, [_vp]),
    "asx_host_malloc": (_vp, [_sz]),
    "asx_host_free": (_int, [_vp]),
    "asx_memcpy_h2d": (_int, [_vp, _vp, _sz]),
    "asx_memcpy_d2h": (_int, [_vp, _vp, _sz]),
    "asx_stream_sync": (_int, [_vp, _vp]),
}

# exported by csrc/asx_api.hip for the tests and tools, NOT part of the public header: planning arithmetic (host only) and
# read-outs of a plan's state
_DIAGNOSTIC_SIGNATURES = {
    "asx_planmath_describe": (_int, [_sz, _str, _u32p, _u32p, c_intp, c_intp, c_intp, c_intp, c_intp, c_intp, c_intp]),
    "asx_planmath_table": (_int, [_sz, _str, _int, c_intp, _sz]),
    "asx_planmath_twiddles": (_int, [_sz, _str, _int, c_f32p, _sz]),
    "asx_planmath_candidates": (_int, [_sz, _sz, _str, _sz]),
    "asx_planmath_kernels": (_int, [_sz, _str, c_intp, c_intp, c_intp]),
    "asx_planmath_kernel_table": (_int, [_int, _int, c_intp]),
    "asx_planmath_group_form": (_int, [c_intp, _int, c_intp, _int]),
    "asx_plan_debug_kernels": (_int, [_vp, c_intp, c_intp, c_intp]),
    "asx_plan_debug_bank": (_int, [_vp, _u64p, _u64p, _u64p]),
    "asx_plan_debug_ncc": (_int, [_vp, _u64p]),
    "asx_plan_debug_ncc_full": (_int, [_vp, _u64p]),
    "asx_plan_debug_ncc_ragged": (_int, [_vp, _u64p]),
    "asx_plan_debug_ncc_tables": (_int, [_vp, _int, _sz, _sz, _vp, _vp, _vp, _vp, _vp]),
    "asx_plan_debug_prune": (_int, [_vp, _sz, c_f32p, c_intp, _sz]),
    "asx_plan_debug_peak": (_int, [_vp, _sz, c_f32p, _u32p, _u32p, _u64p, _vp, _vp, _sz]),
    "asx_plan_debug_spectral": (_int, [_vp, _sz, c_intp, _vp, _sz, c_f64p, ctypes.POINTER(ctypes.c_longlong), c_f64p]),
    "asx_plan_debug_over_list": (_int, [_vp, _u32p, _u32p]),
    "asx_plan_debug_stamps": (ctypes.c_long, [_vp, _vp, _sz]),
}

SIGNATURES = {**_HEADER_SIGNATURES, **_DIAGNOSTIC_SIGNATURES}

# every symbol include/audiosync/xcorr_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = list(_HEADER_SIGNATURES)

TOPK_MAX = 8  # ASX_TOPK_MAX, include/audiosync/xcorr_hip.h
NEAR_MAX = 8  # ASX_NEAR_MAX, include/audiosync/xcorr_hip.h
TRACK_HALF_MAX = 64  # ASX_TRACK_HALF_MAX, include/audiosync/xcorr_hip.h
TRACK_SEG_MAX = 64   # ASX_TRACK_SEG_MAX, include/audiosync/xcorr_hip.h
WARP_DRIFT_MAX = 2.0 ** -6  # ASX_WARP_DRIFT_MAX, include/audiosync/xcorr_hip.h
CLOSURE_LAG_MAX = 1 << 40   # ASX_CLOSURE_LAG_MAX, include/audiosync/xcorr_hip.h
PLACE_HOPS_MAX = 1024       # ASX_PLACE_HOPS_MAX, include/audiosync/xcorr_hip.h
PLACE_SWEEPS_MAX = 64       # ASX_PLACE_SWEEPS_MAX, include/audiosync/xcorr_hip.h
NCC_MIN_ENERGY = 1e-6       # ASX_NCC_MIN_ENERGY, include/audiosync/xcorr_hip.h


class AsxError(RuntimeError):
    pass


def _one_hip_runtime():
    """PyTorch's ROCm wheel ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process do not work, so when torch is installed it is imported FIRST: the
    loader then binds this library's libamdhip64.so.7 dependency to the copy torch already
    loaded, and torch tensors / streams can be handed to the C-ABI as raw pointers.
    ASX_NO_TORCH=1 skips this (pure C / ctypes users of the system runtime)."""
    if os.environ.get("ASX_NO_TORCH") == "1" or "torch" in sys.modules:
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib():
    """dlopen the HIP layer; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AsxError(LIB_PATH + " is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _one_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def _err():
    return lib().asx_last_error().decode("utf-8", "replace")


def _check(rc, message=None):
    """a C-ABI status: non-zero raises AsxError with asx_last_error(), or with `message` for the calls that set none"""
    if rc != 0:
        raise AsxError(message or _err())


def _handle(ptr):
    """a handle or allocation the C-ABI returned: null raises AsxError with asx_last_error()"""
    if not ptr:
        raise AsxError(_err())
    return ptr


def _counters(fn, handle, count, message=None):
    """the `count` uint64 out-parameters of fn(handle, ...) as a tuple of ints"""
    c = [ctypes.c_uint64(0) for _ in range(count)]
    _check(fn(handle, *c), message)
    return tuple(v.value for v in c)


def abi_version():
    return lib().asx_abi_version()


def device_count():
    return lib().asx_device_count()


def _split_arg(split):
    return split.encode() if split else None


def planmath_describe(sample_len, split=None):
    """host-only: what plan would be built for sample_len (no GPU needed)."""
    F, valid = ctypes.c_uint32(), ctypes.c_uint32()
    m1, m2, t, n1, n2 = (ctypes.c_int() for _ in range(5))
    r1 = (ctypes.c_int * 16)()
    r2 = (ctypes.c_int * 16)()
    _check(lib().asx_planmath_describe(sample_len, _split_arg(split), F, valid, m1, m2, t, n1, r1, n2, r2))
    return {"F": F.value, "src_valid": valid.value, "M1": m1.value, "M2": m2.value, "T": t.value,
            "radix1": list(r1[: n1.value]), "radix2": list(r2[: n2.value])}


KERNEL_ENTRY_CAP = 32   # ints per spelled entry the asx_*_kernels exports may write (asx_api.hip: ASX_KERNEL_ENTRY_CAP)


def _kernel_entry(v, nhead, flag=None):
    """(constants..., (radices...)) of a spelled entry, None for none; flag: the constant that is a bool"""
    if v[0] < 0:
        return None
    v = list(v)
    head = [bool(x) if i == flag else x for i, x in enumerate(v[:nhead])]
    return (*head, tuple(v[nhead:v.index(0, nhead)]))


def planmath_kernel_table():
    """host-only: the four lists of csrc/kernel_table.h, each entry as planmath_kernels spells it"""
    f = lib().asx_planmath_kernel_table
    table = {}
    for which, (name, nhead, flag) in enumerate((("real-column cols", 3, None), ("real-column rows", 3, 1),
                                                 ("packed cols", 4, None), ("packed rows", 3, None))):
        table[name], buf = [], (ctypes.c_int * KERNEL_ENTRY_CAP)()
        while f(which, len(table[name]), buf) == 0:
            table[name].append(_kernel_entry(buf, nhead, flag))
    return table


def _kernel_choice(call):
    """the dict of an AsxKernelChoice (asx_planmath_kernels / asx_plan_debug_kernels): an entry of csrc/kernel_table.h as the
    constants its list states and the tuple of its radices, None for a run-time schedule"""
    out, cols, rows = (ctypes.c_int * 7)(), (ctypes.c_int * KERNEL_ENTRY_CAP)(), (ctypes.c_int * KERNEL_ENTRY_CAP)()
    _check(call(out, cols, rows))
    real, entry = bool(out[0]), _kernel_entry
    # real-column: (M1, T, NT, radices) and (NT, two-half, n, radices); packed: (M1, T, NT, MAXR, radices) and (NT, MAXR, n, radices)
    return {"layout": "real-column" if real else "packed", "cols": entry(cols, 3 if real else 4),
            "rows": entry(rows, 3, 1 if real else None), "threads": (out[3], out[4]), "band_rows": out[5],
            "prunable": bool(out[6])}


def planmath_kernels(sample_len, split=None):
    """host-only: the kernels the plan of sample_len would run under the current environment (no GPU needed)."""
    f = lib().asx_planmath_kernels
    return _kernel_choice(lambda *a: f(sample_len, _split_arg(split), *a))


# a launch group's ask and form as csrc/plan_math.h orders them (AsxGroupAsk, AsxGroupForm)
GROUP_ASK = ("rlayout", "plan_prune", "plan_spectral", "band_sums", "over_list", "f32_inputs", "f32_abi", "listed", "r_out",
             "own_lists", "k", "search", "weight", "pool", "bc", "qstore")
GROUP_FORM = ("fwd", "rows", "weight", "bc", "pruned", "tail", "appends", "qstore", "takeback")
GROUP_ENUMS = {"search": ("all", "window", "rows", "topk"), "weight": ("none", "phat", "phat-band"),
               "fwd": ("pool", "real-column", "packed"), "rows": ("packed", "plain", "energy", "listed"),
               "tail": ("phat", "direct", "spectral")}


def planmath_group_form(**ask):
    """host-only: what run_group launches for a group (csrc/plan_math.cpp: asx_group_form).  ask: every name of GROUP_ASK -- bools,
    k and bc ints, search and weight by the names of GROUP_ENUMS; returns the dict of GROUP_FORM, its enums by name too."""
    if set(ask) != set(GROUP_ASK):
        raise ValueError("planmath_group_form: the ask is %s" % (GROUP_ASK,))
    a = (ctypes.c_int * len(GROUP_ASK))(*(GROUP_ENUMS[n].index(ask[n]) if n in GROUP_ENUMS else int(ask[n]) for n in GROUP_ASK))
    out = (ctypes.c_int * len(GROUP_FORM))()
    _check(lib().asx_planmath_group_form(a, len(a), out, len(out)))
    return {n: GROUP_ENUMS[n][v] if n in GROUP_ENUMS else v if n == "bc" else bool(v) for n, v in zip(GROUP_FORM, out)}


def planmath_candidates(sample_len, max_count=16):
    """host-only: the splits the measured mode (split="measure") would time, cheapest first."""
    buf = ctypes.create_string_buffer(64 * max_count + 1)
    n = lib().asx_planmath_candidates(sample_len, max_count, buf, len(buf))
    if n < 0:
        raise AsxError(_err())
    return [x for x in buf.value.decode().split("\n") if x]


def planmath_table(sample_len, which, split=None):
    d = planmath_describe(sample_len, split)
    cap = max(d["M1"], d["M2"])
    buf = (ctypes.c_int * cap)()
    n = lib().asx_planmath_table(sample_len, _split_arg(split), which, buf, cap)
    if n < 0:
        raise AsxError(_err())
    return np.array(buf[:n], dtype=np.int64)


def planmath_twiddles(sample_len, which, split=None):
    d = planmath_describe(sample_len, split)
    cap = max(d["M1"], d["M2"], 2048, (d["F"] >> 11) + 2)
    buf = np.zeros(2 * cap, dtype=np.float32)
    n = lib().asx_planmath_twiddles(sample_len, _split_arg(split), which,
                                    buf.ctypes.data_as(c_f32p), cap)
    if n < 0:
        raise AsxError(_err())
    return buf[: 2 * n].view(np.complex64).copy()


def pearson_f64(source_seg, sample_seg, device=-1):
    a = np.ascontiguousarray(source_seg, dtype=np.float64)
    b = np.ascontiguousarray(sample_seg, dtype=np.float64)
    assert a.size == b.size
    out = ctypes.c_double(0.0)
    _check(lib().asx_pearson_f64(a.ctypes.data_as(c_f64p), b.ctypes.data_as(c_f64p), a.size, device, ctypes.byref(out)))
    return out.value


def results_to_ms_dev(d_lag, d_coef, d_ret, batch, d_lag_ms, d_accept=0, min_confidence=0.95, sample_rate=48000.0, stream=0):
    _check(lib().asx_results_to_ms_dev(d_lag, d_coef, d_ret, batch, min_confidence, sample_rate, d_lag_ms,
                                       d_accept or None, stream or None))


def topk_best_dev(d_lag, d_coef, d_ret, batch, k, d_best_coef, d_best_ret, d_best_lag=0, d_best_entry=0, stream=0):
    """raw device pointers (ints): asx_topk_best_dev -- per pair, of its k entries at i*k + j, the one with ret == 0 and the largest
    signed coefficient (none: entry 0) to index i of the best arrays, which results_to_ms_dev takes; asynchronous on `stream`"""
    _check(lib().asx_topk_best_dev(d_lag, d_coef, d_ret, int(batch), int(k), d_best_lag or None, d_best_coef, d_best_ret,
                                   d_best_entry or None, stream or None))


def pool_closure_dev(d_lag, d_coef, d_ret, nclips, k, tolerance, min_confirm, root, d_best_lag, d_best_coef, d_best_ret, d_best_entry,
                     d_confirm, d_root, d_offset, d_support, d_placed, d_votes=0, stream=0):
    """raw device pointers (ints): asx_pool_closure_dev -- over the [C, C, k] tables of an all-pairs top-k call on one pool, per pair
    the entry the other clips agree with (triangle closure) to index a * C + b of the best arrays, which results_to_ms_dev takes,
    the clips that confirm each pick, the root and every clip's offset from it; d_votes [C * C * k] is optional; asynchronous on
    `stream`, on the current device"""
    _check(lib().asx_pool_closure_dev(d_lag, d_coef, d_ret, int(nclips), int(k), int(tolerance), int(min_confirm), int(root),
                                      d_votes or None, d_best_lag, d_best_coef, d_best_ret, d_best_entry, d_confirm, d_root, d_offset,
                                      d_support, d_placed, stream or None))


def closure_args(lag, coef, ret, tolerance, min_confirm=1, root=-1):
    """Host checks of pool_closure: lag and ret integer arrays and coef a real one, all of one shape [C, C, k] with C >= 1 and
    1 <= k <= TOPK_MAX (C * C * k <= 2^31 - 1, lags within int64, rets within int32); tolerance an integer in [0, CLOSURE_LAG_MAX],
    min_confirm an integer >= 0, root an integer in [-1, C) -- no bools, no floats.  -> (lag int64, coef float64, ret int32, C, k,
    tolerance, min_confirm, root) as contiguous arrays and ints.  ValueError on anything else.  The values of the tables are not
    checked: an entry with ret != 0 or |lag| > CLOSURE_LAG_MAX is not valid, which is part of the rule."""
    lg, cf, rt = np.asarray(lag), np.asarray(coef), np.asarray(ret)
    if lg.dtype.kind not in "iu" or rt.dtype.kind not in "iu":
        raise ValueError("lag and ret must hold integers, not %s and %s" % (lg.dtype, rt.dtype))
    if cf.dtype.kind not in "fiu":
        raise ValueError("coef must hold real numbers, not %s" % cf.dtype)
    if lg.ndim != 3 or lg.shape[0] != lg.shape[1] or cf.shape != lg.shape or rt.shape != lg.shape:
        raise ValueError("lag, coef and ret must share one shape [C, C, k], not %s, %s and %s"
                         % (list(lg.shape), list(cf.shape), list(rt.shape)))
    c, k = lg.shape[0], lg.shape[2]
    if c < 1 or not 1 <= k <= TOPK_MAX or c * c * k > 2 ** 31 - 1:
        raise ValueError("[C, C, k] needs C >= 1, 1 <= k <= %d and C * C * k <= 2^31 - 1, not C = %d, k = %d" % (TOPK_MAX, c, k))
    if lg.dtype == np.uint64 and lg.max() > 2 ** 63 - 1:
        raise ValueError("lags must fit int64")
    if rt.min() < -2 ** 31 or rt.max() > 2 ** 31 - 1:
        raise ValueError("rets must fit int32")
    for name, v, lo, hi in (("tolerance", tolerance, 0, CLOSURE_LAG_MAX), ("min_confirm", min_confirm, 0, 2 ** 31 - 1),
                            ("root", root, -1, c - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s must be an integer in [%d, %d], not %r" % (name, lo, hi, v))
    return (np.ascontiguousarray(lg, dtype=np.int64), np.ascontiguousarray(cf, dtype=np.float64),
            np.ascontiguousarray(rt, dtype=np.int32), c, k, int(tolerance), int(min_confirm), int(root))


class _CurrentDevice:
    """what _Staging needs of a plan, for the calls that take none: they run on the current device, on the null stream"""

    def __init__(self, device):
        current = lib().asx_current_device()
        if device not in (-1, current):
            raise AsxError("this call takes no plan and runs on the current device (%d), not on device %d" % (current, device))
        self.device = -1

    def sync(self):
        _check(lib().asx_stream_sync(None, None))


def pool_closure(lag, coef, ret, tolerance, min_confirm=1, root=-1, device=-1, votes=False):
    """Triangle closure over one clip pool (asx_pool_closure_dev) on host arrays: lag, coef, ret of shape [C, C, k] as
    Plan.xcorr_pool_topk_f32 returns them for one array as both pools (pairs=None).  Arguments are checked on the host (closure_args,
    ValueError) before anything is uploaded.  Returns a dict of numpy arrays: best_lag int64, best_coef float64, best_ret, best_entry
    and confirm int32 of shape [C, C]; root, an int; offset int64, support and placed int32 of shape [C]; votes int32 [C, C, k] when
    votes=True.  device: -1 or the current device (the call takes no plan)."""
    lg, cf, rt, c, k, tolerance, min_confirm, root = closure_args(lag, coef, ret, tolerance, min_confirm, root)
    with _Staging(_CurrentDevice(int(device))) as st:
        d_in = [st.upload(a) for a in (lg, cf, rt)]
        d_votes = st.output((c, c, k), np.int32) if votes else 0
        names = (("best_lag", (c, c), np.int64), ("best_coef", (c, c), np.float64), ("best_ret", (c, c), np.int32),
                 ("best_entry", (c, c), np.int32), ("confirm", (c, c), np.int32), ("root", (1,), np.int32), ("offset", (c,), np.int64),
                 ("support", (c,), np.int32), ("placed", (c,), np.int32))
        d_out = [st.output(shape, dt) for _, shape, dt in names]
        pool_closure_dev(*d_in, c, k, tolerance, min_confirm, root, *d_out, d_votes=d_votes)
        got = st.fetch()
    out = dict(zip([n for n, _, _ in names], got[1:] if votes else got))
    out["root"] = int(out["root"][0])
    if votes:
        out["votes"] = got[0]
    return out


def pool_place_dev(d_lag, d_ret, d_confirm, nclips, tolerance, min_confirm, d_root, max_hops, sweeps, d_offset, d_hops, d_support,
                   d_degree, d_step, d_resid, d_state, d_scratch=0, stream=0):
    """raw device pointers (ints): asx_pool_place_dev -- from closure's picked tables (d_best_lag, d_best_ret, d_confirm, [C * C]) and
    the root in device memory (d_root [1]), every clip that a chain of usable pairs reaches: hops from the root and offset per clip,
    support, degree and the last sweep's step [C each], and per pair the residual against the offsets and a state (1 agrees, 2
    disagrees, 0 not usable or an end not reached) [C * C each]; d_scratch [C] is needed when sweeps > 0; asynchronous on `stream`, on
    the current device"""
    _check(lib().asx_pool_place_dev(d_lag, d_ret, d_confirm, int(nclips), int(tolerance), int(min_confirm), d_root, int(max_hops),
                                    int(sweeps), d_scratch or None, d_offset, d_hops, d_support, d_degree, d_step, d_resid, d_state,
                                    stream or None))


def place_args(best_lag, best_ret, confirm, root, tolerance, min_confirm=1, max_hops=64, sweeps=0):
    """Host checks of pool_place: best_lag, best_ret and confirm integer arrays of one shape [C, C] with C >= 1 and C * C <= 2^31 - 1
    (lags within int64, rets and confirms within int32); root an integer within int32 (outside [0, C) is legal: no clip is reached);
    tolerance an integer in [0, CLOSURE_LAG_MAX], min_confirm an integer >= 0, max_hops one in [1, PLACE_HOPS_MAX], sweeps one in
    [0, PLACE_SWEEPS_MAX] -- no bools, no floats.  -> (lag int64, ret int32, confirm int32, C, root, tolerance, min_confirm, max_hops,
    sweeps) as contiguous arrays and ints.  ValueError on anything else."""
    lg, rt, cf = np.asarray(best_lag), np.asarray(best_ret), np.asarray(confirm)
    for name, a in (("best_lag", lg), ("best_ret", rt), ("confirm", cf)):
        if a.dtype.kind not in "iu":
            raise ValueError("%s must hold integers, not %s" % (name, a.dtype))
    if lg.ndim != 2 or lg.shape[0] != lg.shape[1] or rt.shape != lg.shape or cf.shape != lg.shape:
        raise ValueError("best_lag, best_ret and confirm must share one shape [C, C], not %s, %s and %s"
                         % (list(lg.shape), list(rt.shape), list(cf.shape)))
    c = lg.shape[0]
    if c < 1 or c * c > 2 ** 31 - 1:
        raise ValueError("[C, C] needs C >= 1 and C * C <= 2^31 - 1, not C = %d" % c)
    if lg.dtype == np.uint64 and lg.max() > 2 ** 63 - 1:
        raise ValueError("lags must fit int64")
    for name, a in (("rets", rt), ("confirms", cf)):
        if a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1:
            raise ValueError("%s must fit int32" % name)
    for name, v, lo, hi in (("root", root, -2 ** 31, 2 ** 31 - 1), ("tolerance", tolerance, 0, CLOSURE_LAG_MAX),
                            ("min_confirm", min_confirm, 0, 2 ** 31 - 1), ("max_hops", max_hops, 1, PLACE_HOPS_MAX),
                            ("sweeps", sweeps, 0, PLACE_SWEEPS_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s must be an integer in [%d, %d], not %r" % (name, lo, hi, v))
    return (np.ascontiguousarray(lg, dtype=np.int64), np.ascontiguousarray(rt, dtype=np.int32), np.ascontiguousarray(cf, dtype=np.int32),
            c, int(root), int(tolerance), int(min_confirm), int(max_hops), int(sweeps))


def pool_place(best_lag, best_ret, confirm, root, tolerance, min_confirm=1, max_hops=64, sweeps=0, device=-1):
    """Placement over chains of usable pairs (asx_pool_place_dev) on host arrays: best_lag, best_ret, confirm of shape [C, C] and root
    as pool_closure returns them, with the tolerance and min_confirm it was given.  Arguments are checked on the host (place_args,
    ValueError) before anything is uploaded.  Returns a dict of numpy arrays: offset and step int64, hops, support and degree int32 of
    shape [C]; resid int64 and state int32 of shape [C, C].  device: -1 or the current device (the call takes no plan)."""
    lg, rt, cf, c, root, tolerance, min_confirm, max_hops, sweeps = place_args(best_lag, best_ret, confirm, root, tolerance, min_confirm,
                                                                               max_hops, sweeps)
    with _Staging(_CurrentDevice(int(device))) as st:
        d_in = [st.upload(a) for a in (lg, rt, cf)]
        d_root = st.upload(np.array([root], dtype=np.int32))
        d_scratch = st.alloc(8 * c) if sweeps else 0
        names = (("offset", (c,), np.int64), ("hops", (c,), np.int32), ("support", (c,), np.int32), ("degree", (c,), np.int32),
                 ("step", (c,), np.int64), ("resid", (c, c), np.int64), ("state", (c, c), np.int32))
        d_out = [st.output(shape, dt) for _, shape, dt in names]
        pool_place_dev(*d_in, c, tolerance, min_confirm, d_root, max_hops, sweeps, *d_out, d_scratch=d_scratch)
        got = st.fetch()
    return dict(zip([n for n, _, _ in names], got))


def synth_pairs_dev(seed, first_pair, count, sample_len, noise_shift, d_src, d_smp, d_lag=0, stream=0):
    _check(lib().asx_synth_pairs_dev(seed, first_pair, count, sample_len, noise_shift, d_src, d_smp,
                                     d_lag or None, stream or None))


def xcorr_batch_multi(plans, source, sample):
    """host float32 arrays [B,2N], [B,N] block-partitioned over `plans` (one per device) -> (lag, coef, ret)"""
    s = np.ascontiguousarray(source, dtype=np.float32)
    t = np.ascontiguousarray(sample, dtype=np.float32)
    n = plans[0].sample_len
    batch = t.size // n
    assert t.size == batch * n and s.size == 2 * n * batch
    lag = np.zeros(batch, dtype=np.int64)
    coef = np.zeros(batch, dtype=np.float64)
    ret = np.zeros(batch, dtype=np.int32)
    handles = (ctypes.c_void_p * len(plans))(*[p._h for p in plans])
    _check(lib().asx_xcorr_batch_multi(handles, len(plans), s.ctypes.data_as(c_f32p), t.ctypes.data_as(c_f32p), batch,
                                       lag.ctypes.data_as(c_i64p), coef.ctypes.data_as(c_f64p), ret.ctypes.data_as(c_i32p)))
    return lag, coef, ret


def band_bins(sample_len, sample_rate, f_lo_hz, f_hi_hz):
    """asx_band_bins: (bin_lo, bin_hi) of the band [f_lo_hz, f_hi_hz] for the banded PHAT calls -- bins of the 2N-point transform, bin m at
    m * sample_rate / (2N) Hz, a band past the Nyquist frequency ending at bin N.  No device.  ValueError: no such band."""
    lo, hi = ctypes.c_int64(-1), ctypes.c_int64(-1)
    if lib().asx_band_bins(int(sample_len), float(sample_rate), float(f_lo_hz), float(f_hi_hz), ctypes.byref(lo), ctypes.byref(hi)) != 0:
        raise ValueError("no bins for the band [%r, %r] Hz at %r Hz and %r samples" % (f_lo_hz, f_hi_hz, sample_rate, sample_len))
    return int(lo.value), int(hi.value)


def _operands(n, source, sample):
    """the two operands of a strided call for sample length n -> (source [2N] or [B, 2N], sample [N] or [B, N]) as contiguous
    float32 arrays, (source_stride, sample_stride) in floats: 0 for a 1-D operand, which serves every pair"""
    s = np.ascontiguousarray(source, dtype=np.float32)
    t = np.ascontiguousarray(sample, dtype=np.float32)
    if s.ndim not in (1, 2) or t.ndim not in (1, 2) or s.shape[-1] != 2 * n or t.shape[-1] != n:
        raise ValueError("source must be [2N] or [B, 2N] and sample [N] or [B, N] with N = %d" % n)
    return s, t, 2 * n if s.ndim == 2 else 0, n if t.ndim == 2 else 0


def _window_rows(windows, batch=None):
    """lag windows -> contiguous int64 [2] or [B, 2] rows (lag_min, lag_max); batch: the B that a 2-D array must have"""
    w = np.asarray(windows)
    if w.dtype.kind not in "iu":
        raise ValueError("windows must hold integers (lag_min, lag_max), not %s" % w.dtype)
    w = np.ascontiguousarray(w, dtype=np.int64)
    if w.ndim not in (1, 2) or w.shape[-1] != 2 or (batch is not None and w.ndim == 2 and w.shape[0] != batch):
        raise ValueError("windows must be [2] or [B, 2]" + ("" if batch is None else " with B = %d pairs" % batch))
    return w


def _shared_batch(*arrays):
    """the batch size the 2-D arrays among `arrays` (None: absent) agree on; 1 when all are 1-D"""
    sizes = {a.shape[0] for a in arrays if a is not None and a.ndim == 2}
    if len(sizes) > 1:
        raise ValueError("source, sample and windows have different batch sizes %s" % sorted(sizes))
    return sizes.pop() if sizes else 1


def _strided_args(n, source, sample, w):
    """windowed_args' tuple for checked window rows w; w None (no rows): None and a window stride of 0 in their places"""
    s, t, ss, ts = _operands(n, source, sample)
    batch = _shared_batch(s, t, w)
    if batch < 1:
        raise ValueError("empty batch")
    return s, t, w, batch, ss, ts, 1 if w is not None and w.ndim == 2 else 0


def _topk_option(k, min_separation):
    """-> (k, min_separation) as ints; ValueError unless they are integers (no bools), 1 <= k <= TOPK_MAX, min_separation >= 0"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError("k must be an integer in [1, %d], not %r" % (TOPK_MAX, k))
    if isinstance(min_separation, bool) or not isinstance(min_separation, (int, np.integer)) or int(min_separation) < 0:
        raise ValueError("min_separation must be an integer >= 0, not %r" % (min_separation,))
    return int(k), int(min_separation)


def windowed_args(n, source, sample, windows):
    """Host checks of Plan.xcorr_windowed_f32 for a plan of sample length n: source [2N] or [B, 2N], sample [N] or [B, N], windows
    [2] or [B, 2] integers (a 1-D operand serves every pair).  -> (source, sample, windows, batch, source_stride, sample_stride,
    window_stride) as contiguous float32 / int64 arrays and strides in elements / rows.  ValueError on anything else.  The rows'
    values are not checked: a row that is not a window comes back as (0, NaN, -2)."""
    return _strided_args(n, source, sample, _window_rows(windows))


def _energy_option(min_energy):
    """-> min_energy as a float; ValueError unless it is a real number (no bool) with NCC_MIN_ENERGY <= min_energy <= 1"""
    if isinstance(min_energy, bool) or not isinstance(min_energy, (int, float, np.integer, np.floating)) or \
            not NCC_MIN_ENERGY <= float(min_energy) <= 1.0:
        raise ValueError("min_energy must be a number in [%g, 1], not %r" % (NCC_MIN_ENERGY, min_energy))
    return float(min_energy)


def ncc_args(n, source, sample, windows=None, min_energy=1e-3):
    """Host checks of Plan.xcorr_ncc_f32: the shapes of windowed_args (windows=None: every lag 0..N-1, no rows) and
    NCC_MIN_ENERGY <= min_energy <= 1.  -> (source, sample, windows or None, batch, source_stride, sample_stride, window_stride,
    min_energy).  ValueError on anything else.  The rows' values are not checked: a row outside [0, N-1] comes back as ret = -2."""
    option = _energy_option(min_energy)
    return _strided_args(n, source, sample, None if windows is None else _window_rows(windows)) + (option,)


def ncc_topk_args(n, source, sample, k, min_separation, windows=None, min_energy=1e-3):
    """Host checks of Plan.xcorr_ncc_topk_f32: ncc_args' checks, and k and min_separation as topk_args checks them.  -> ncc_args' tuple
    + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return ncc_args(n, source, sample, windows, min_energy) + option


def _overlap_option(n, min_overlap):
    """-> min_overlap as an int; None: (N + 1) // 2.  ValueError unless it is an integer (no bool) with 1 <= min_overlap <= N"""
    if min_overlap is None:
        return (n + 1) // 2
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer)) or not 1 <= int(min_overlap) <= n:
        raise ValueError("min_overlap must be an integer in [1, %d], not %r" % (n, min_overlap))
    return int(min_overlap)


def ncc_full_args(n, source, sample, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_ncc_full_f32: ncc_args' checks (windows=None: every lag -(N-1)..N-1, no rows), and min_overlap as an
    integer in [1, N] (None: (N + 1) // 2).  -> ncc_args' tuple + (min_overlap,).  ValueError on anything else.  The rows' values are
    not checked: a row outside [-(N-1), N-1] comes back as ret = -2."""
    option = _overlap_option(n, min_overlap)
    return ncc_args(n, source, sample, windows, min_energy) + (option,)


def ncc_full_topk_args(n, source, sample, k, min_separation, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_ncc_full_topk_f32: ncc_full_args' checks, and k and min_separation as topk_args checks them.  ->
    ncc_full_args' tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return ncc_full_args(n, source, sample, windows, min_energy, min_overlap) + option


def ragged_pack(tracks, width):
    """1-D arrays of differing sizes -> (float32 [n, width], zero-padded behind each track, and their sizes as int64 [n]): an
    operand of Plan.xcorr_ncc_ragged_f32 and its column of lengths.  ValueError for a track that is not 1-D, is empty or is longer
    than width."""
    rows = [np.asarray(t, dtype=np.float32) for t in tracks]
    if not rows or any(r.ndim != 1 or not 1 <= r.size <= width for r in rows):
        raise ValueError("tracks must be 1-D arrays of 1..%d frames each, at least one of them" % width)
    out = np.zeros((len(rows), int(width)), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :r.size] = r
    return out, np.array([r.size for r in rows], dtype=np.int64)


def _length_rows(lengths, batch=None):
    """track lengths -> contiguous int64 [2] or [B, 2] rows (Ls, Lm); batch: the B that a 2-D array must have"""
    v = np.asarray(lengths)
    if v.dtype.kind not in "iu":
        raise ValueError("lengths must hold integers (source frames, sample frames), not %s" % v.dtype)
    v = np.ascontiguousarray(v, dtype=np.int64)
    if v.ndim not in (1, 2) or v.shape[-1] != 2 or (batch is not None and v.ndim == 2 and v.shape[0] != batch):
        raise ValueError("lengths must be [2] or [B, 2]" + ("" if batch is None else " with B = %d pairs" % batch))
    return v


def ncc_ragged_args(n, source, sample, lengths=None, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_ncc_ragged_f32: ncc_full_args' checks, and lengths as None (every pair (2N, N)) or integers [2] /
    [B, 2] rows (Ls, Lm); a 2-D lengths array counts towards the batch size like the other operands.  -> (source, sample, lengths or
    None, windows or None, batch, source_stride, sample_stride, length_stride, window_stride, min_energy, min_overlap).  ValueError on
    anything else.  The rows' values are not checked: a row outside 1 <= Ls <= 2N, 1 <= Lm <= N comes back as ret = -5."""
    me, mo = _energy_option(min_energy), _overlap_option(n, min_overlap)
    s, t, ss, ts = _operands(n, source, sample)
    v = None if lengths is None else _length_rows(lengths)
    w = None if windows is None else _window_rows(windows)
    batch = _shared_batch(s, t, v, w)
    if batch < 1:
        raise ValueError("empty batch")
    return (s, t, v, w, batch, ss, ts, 1 if v is not None and v.ndim == 2 else 0, 1 if w is not None and w.ndim == 2 else 0, me, mo)


def ncc_ragged_topk_args(n, source, sample, k, min_separation, lengths=None, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_ncc_ragged_topk_f32: ncc_ragged_args' checks, and k and min_separation as topk_args checks them.  ->
    ncc_ragged_args' tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return ncc_ragged_args(n, source, sample, lengths, windows, min_energy, min_overlap) + option


def topk_args(n, source, sample, k, min_separation, windows=None):
    """Host checks of Plan.xcorr_topk_f32: the shapes of windowed_args (windows=None: the plan's window, no rows), 1 <= k <= TOPK_MAX
    and min_separation >= 0, integers.  -> (source, sample, windows or None, batch, source_stride, sample_stride, window_stride, k,
    min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return _strided_args(n, source, sample, None if windows is None else _window_rows(windows)) + option


def pool_args(n, sources, samples, pairs=None, windows=None):
    """Host checks of Plan.xcorr_pool_f32 for a plan of sample length n: sources [S, 2N] and samples [R, N] float arrays (S, R >= 1),
    pairs None (every combination, source-major) or integers [B, 2] rows (source index, sample index), windows None or integers [2] /
    [B, 2] rows (lag_min, lag_max) as in xcorr_windowed_f32.  -> (sources, samples, pairs or None, windows or None, batch,
    window_stride) as contiguous float32 / int32 / int64 arrays.  ValueError on anything else.  The indices and the rows' values are
    not checked: an index outside its pool comes back as (0, NaN, -4), a row that is not a window as (0, NaN, -2)."""
    s = np.ascontiguousarray(sources, dtype=np.float32)
    t = np.ascontiguousarray(samples, dtype=np.float32)
    if s.ndim != 2 or t.ndim != 2 or s.shape[1] != 2 * n or t.shape[1] != n:
        raise ValueError("sources must be [S, 2N] and samples [R, N] with N = %d" % n)
    if s.shape[0] < 1 or t.shape[0] < 1:
        raise ValueError("empty pool (%d sources, %d samples)" % (s.shape[0], t.shape[0]))
    if s.shape[0] > 2 ** 31 - 1 or t.shape[0] > 2 ** 31 - 1:
        raise ValueError("a pool of more than 2^31 - 1 tracks")
    if pairs is None:
        pr = None
        batch = s.shape[0] * t.shape[0]
    else:
        pr = np.asarray(pairs)
        if pr.dtype.kind not in "iu":
            raise ValueError("pairs must hold integers (source index, sample index), not %s" % pr.dtype)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] < 1:
            raise ValueError("pairs must be [B, 2] with B >= 1")
        if pr.size and (pr.min() < -2 ** 31 or pr.max() > 2 ** 31 - 1):
            raise ValueError("pair indices must fit int32")
        pr = np.ascontiguousarray(pr, dtype=np.int32)
        batch = pr.shape[0]
    w = None if windows is None else _window_rows(windows, batch)
    return s, t, pr, w, batch, 1 if w is not None and w.ndim == 2 else 0


def pool_topk_args(n, sources, samples, k, min_separation, pairs=None, windows=None):
    """Host checks of Plan.xcorr_pool_topk_f32: k and min_separation as topk_args checks them, the rest as pool_args.  -> pool_args'
    tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return pool_args(n, sources, samples, pairs, windows) + option


def pool_ncc_args(n, sources, samples, pairs=None, windows=None, min_energy=1e-3):
    """Host checks of Plan.xcorr_pool_ncc_f32: min_energy as ncc_args checks it, the rest as pool_args (windows None: every lag
    0..N-1).  -> pool_args' tuple + (min_energy,).  ValueError on anything else."""
    option = _energy_option(min_energy)
    return pool_args(n, sources, samples, pairs, windows) + (option,)


def pool_ncc_topk_args(n, sources, samples, k, min_separation, pairs=None, windows=None, min_energy=1e-3):
    """Host checks of Plan.xcorr_pool_ncc_topk_f32: k and min_separation as topk_args checks them, the rest as pool_ncc_args.  ->
    pool_ncc_args' tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return pool_ncc_args(n, sources, samples, pairs, windows, min_energy) + option


def pool_ncc_full_args(n, sources, samples, pairs=None, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_pool_ncc_full_f32: min_overlap as ncc_full_args checks it (None: (N + 1) // 2), the rest as
    pool_ncc_args (windows None: every lag -(N-1)..N-1).  -> pool_ncc_args' tuple + (min_overlap,).  ValueError on anything else.  The
    rows' values are not checked: a row outside [-(N-1), N-1] comes back as ret = -2."""
    option = _overlap_option(n, min_overlap)
    return pool_ncc_args(n, sources, samples, pairs, windows, min_energy) + (option,)


def pool_ncc_full_topk_args(n, sources, samples, k, min_separation, pairs=None, windows=None, min_energy=1e-3, min_overlap=None):
    """Host checks of Plan.xcorr_pool_ncc_full_topk_f32: k and min_separation as topk_args checks them, the rest as
    pool_ncc_full_args.  -> pool_ncc_full_args' tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return pool_ncc_full_args(n, sources, samples, pairs, windows, min_energy, min_overlap) + option


def pool_phat_args(n, sources, samples, pairs=None, windows=None, band=None):
    """Host checks of Plan.xcorr_pool_phat_f32: band None (every bin, (0, N)) or integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi
    <= N, the rest as pool_args.  -> pool_args' tuple + (bin_lo, bin_hi).  ValueError on anything else."""
    lo, hi = (0, n) if band is None else band
    if any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) for b in (lo, hi)) or not 0 <= int(lo) <= int(hi) <= n:
        raise ValueError("band must be integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi <= %d, not %r" % (n, band))
    return pool_args(n, sources, samples, pairs, windows) + (int(lo), int(hi))


def _band_option(n, band):
    """band None (every bin, (0, N)) or integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi <= N -> (bin_lo, bin_hi) as ints"""
    lo, hi = (0, n) if band is None else band
    if any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) for b in (lo, hi)) or not 0 <= int(lo) <= int(hi) <= n:
        raise ValueError("band must be integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi <= %d, not %r" % (n, band))
    return int(lo), int(hi)


def _near_option(half_width):
    """-> half_width as an int; ValueError unless it is an integer (no bool) in [1, NEAR_MAX]"""
    if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or not 1 <= int(half_width) <= NEAR_MAX:
        raise ValueError("half_width must be an integer in [1, %d], not %r" % (NEAR_MAX, half_width))
    return int(half_width)


def phat_sub_args(n, source, sample, windows=None, band=None, half_width=1):
    """Host checks of Plan.xcorr_phat_sub_f32: the shapes of windowed_args (windows=None: the plan's window, no rows), band None
    (every bin) or integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi <= N, half_width an integer in [1, NEAR_MAX].  ->
    (source, sample, windows or None, batch, source_stride, sample_stride, window_stride, bin_lo, bin_hi, half_width).  ValueError on
    anything else."""
    option = _band_option(n, band) + (_near_option(half_width),)
    return _strided_args(n, source, sample, None if windows is None else _window_rows(windows)) + option


def pool_phat_sub_args(n, sources, samples, pairs=None, windows=None, band=None, half_width=1):
    """Host checks of Plan.xcorr_pool_phat_sub_f32: half_width an integer in [1, NEAR_MAX], the rest as pool_phat_args.  ->
    pool_phat_args' tuple + (half_width,).  ValueError on anything else."""
    h = _near_option(half_width)
    return pool_phat_args(n, sources, samples, pairs, windows, band) + (h,)


def phat_topk_args(n, source, sample, k, min_separation, windows=None, band=None):
    """Host checks of Plan.xcorr_phat_topk_f32: the shapes of windowed_args (windows=None: the plan's window, no rows), band None
    (every bin) or integers (bin_lo, bin_hi) with 0 <= bin_lo <= bin_hi <= N, k and min_separation as topk_args checks them.  ->
    (source, sample, windows or None, batch, source_stride, sample_stride, window_stride, bin_lo, bin_hi, k, min_separation).
    ValueError on anything else."""
    option = _band_option(n, band) + _topk_option(k, min_separation)
    return _strided_args(n, source, sample, None if windows is None else _window_rows(windows)) + option


def pool_phat_topk_args(n, sources, samples, k, min_separation, pairs=None, windows=None, band=None):
    """Host checks of Plan.xcorr_pool_phat_topk_f32: k and min_separation as topk_args checks them, the rest as pool_phat_args.  ->
    pool_phat_args' tuple + (k, min_separation).  ValueError on anything else."""
    option = _topk_option(k, min_separation)
    return pool_phat_args(n, sources, samples, pairs, windows, band) + option


def _curve_option(half_width, entries):
    """-> (half_width, entries) as ints; ValueError unless they are integers (no bools), half_width in [1, NEAR_MAX] and entries in
    [1, TOPK_MAX]"""
    if isinstance(entries, bool) or not isinstance(entries, (int, np.integer)) or not 1 <= int(entries) <= TOPK_MAX:
        raise ValueError("entries must be an integer in [1, %d], not %r" % (TOPK_MAX, entries))
    return _near_option(half_width), int(entries)


def _centers(centers, lead, entries):
    """the centre lags of a curve call -> a contiguous int64 array of shape lead + (entries,), or lead alone when entries == 1
    (lead: the shape of the pairs; a None in it: any size).  -> (centers, their leading shape)"""
    c = np.asarray(centers)
    if c.dtype.kind not in "iu":
        raise ValueError("centers must hold integers (lags), not %s" % c.dtype)
    c = np.ascontiguousarray(c, dtype=np.int64)
    shapes = [tuple(lead) + (entries,)] + ([tuple(lead)] if entries == 1 else [])
    for want in shapes:
        if c.ndim == len(want) and all(w is None or w == g for w, g in zip(want, c.shape)):
            return c, c.shape[:len(lead)]
    raise ValueError("centers must be of shape %s, not %s" % (" or ".join(str(list(w)).replace("None", "B") for w in shapes), list(c.shape)))


def curve_args(n, source, sample, centers, half_width=1, entries=1):
    """Host checks of Plan.xcorr_curve_f32 for a plan of sample length n: source [2N] or [B, 2N], sample [N] or [B, N] (a 1-D operand
    serves every pair), centers integers [B, entries] (or [B] when entries == 1) -- B the batch of the 2-D operands, any B >= 1 when
    both are 1-D -- half_width an integer in [1, NEAR_MAX], entries in [1, TOPK_MAX].  -> (source, sample, centers, batch,
    source_stride, sample_stride, half_width, entries) as contiguous float32 / int64 arrays and strides in floats.  ValueError on
    anything else.  The centres' values are not checked: one outside [-N, N-1] comes back with ret -2."""
    h, entries = _curve_option(half_width, entries)
    s, t, ss, ts = _operands(n, source, sample)
    sizes = {a.shape[0] for a in (s, t) if a.ndim == 2}
    if len(sizes) > 1:
        raise ValueError("source and sample have different batch sizes %s" % sorted(sizes))
    c, lead = _centers(centers, (sizes.pop() if sizes else None,), entries)
    if lead[0] < 1:
        raise ValueError("empty batch")
    return s, t, c, lead[0], ss, ts, h, entries


def pool_curve_args(n, sources, samples, centers, pairs=None, half_width=1, entries=1):
    """Host checks of Plan.xcorr_pool_curve_f32: the pools and pairs of pool_args, centers integers [B, entries] (or [B] when entries
    == 1) with pairs, [S, R, entries] (or [S, R]) without, half_width and entries as curve_args checks them.  -> (sources, samples,
    pairs or None, centers, batch, half_width, entries).  ValueError on anything else."""
    h, entries = _curve_option(half_width, entries)
    s, t, pr, _, batch, _ = pool_args(n, sources, samples, pairs)
    c, _ = _centers(centers, (batch,) if pr is not None else (s.shape[0], t.shape[0]), entries)
    return s, t, pr, c, batch, h, entries


def _track_option(n, half_width, segments, entries):
    """-> (half_width, segments, entries) as ints; ValueError unless they are integers (no bools), half_width in [1, TRACK_HALF_MAX],
    segments in [1, min(TRACK_SEG_MAX, n)] and entries in [1, TOPK_MAX]"""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not integer(entries) or not 1 <= int(entries) <= TOPK_MAX:
        raise ValueError("entries must be an integer in [1, %d], not %r" % (TOPK_MAX, entries))
    if not integer(half_width) or not 1 <= int(half_width) <= TRACK_HALF_MAX:
        raise ValueError("half_width must be an integer in [1, %d], not %r" % (TRACK_HALF_MAX, half_width))
    if not integer(segments) or not 1 <= int(segments) <= min(TRACK_SEG_MAX, int(n)):
        raise ValueError("segments must be an integer in [1, %d], not %r" % (min(TRACK_SEG_MAX, int(n)), segments))
    return int(half_width), int(segments), int(entries)


def track_args(n, source, sample, centers, half_width, segments, entries=1):
    """Host checks of Plan.xcorr_track_f32 for a plan of sample length n: source, sample and centers as curve_args checks them,
    half_width an integer in [1, TRACK_HALF_MAX], segments in [1, min(TRACK_SEG_MAX, n)], entries in [1, TOPK_MAX].  -> (source,
    sample, centers, batch, source_stride, sample_stride, half_width, segments, entries).  ValueError on anything else."""
    h, segs, entries = _track_option(n, half_width, segments, entries)
    s, t, c, batch, ss, ts, _, _ = curve_args(n, source, sample, centers, 1, entries)
    return s, t, c, batch, ss, ts, h, segs, entries


def pool_track_args(n, sources, samples, centers, half_width, segments, pairs=None, entries=1):
    """Host checks of Plan.xcorr_pool_track_f32: the pools, pairs and centers of pool_curve_args, the options of track_args.  ->
    (sources, samples, pairs or None, centers, batch, half_width, segments, entries).  ValueError on anything else."""
    h, segs, entries = _track_option(n, half_width, segments, entries)
    s, t, pr, c, batch, _, _ = pool_curve_args(n, sources, samples, centers, pairs, 1, entries)
    return s, t, pr, c, batch, h, segs, entries


def _lines(lines, shape):
    """the drift lines of a warp call for centres of `shape` -> (a contiguous float64 array, line_stride in doubles): [2] or [3], one
    line {drift, lag0} for every entry (stride 0), or shape + [2] (packed lines) or shape + [3] (the track call's fit, whose rms is
    not read).  The values are not checked: a line that is not valid comes back with ret -5."""
    ln = np.asarray(lines)
    if ln.dtype.kind not in "fiu":
        raise ValueError("lines must hold numbers {drift, lag0}, not %s" % ln.dtype)
    ln = np.ascontiguousarray(ln, dtype=np.float64)
    if ln.ndim == 1 and ln.shape[0] in (2, 3):
        return ln, 0
    if ln.ndim == len(shape) + 1 and ln.shape[:-1] == tuple(shape) and ln.shape[-1] in (2, 3):
        return ln, ln.shape[-1]
    raise ValueError("lines must be of shape [2], [3] or %s + [2] or [3], not %s" % (list(shape), list(ln.shape)))


def warp_args(n, source, sample, centers, lines, half_width=1, entries=1):
    """Host checks of Plan.xcorr_warp_f32 for a plan of sample length n: source, sample, centers, half_width and entries as curve_args
    checks them, lines as _lines does.  -> (source, sample, centers, lines, batch, source_stride, sample_stride, line_stride,
    half_width, entries).  ValueError on anything else."""
    s, t, c, batch, ss, ts, h, entries = curve_args(n, source, sample, centers, half_width, entries)
    ln, ls = _lines(lines, c.shape)
    return s, t, c, ln, batch, ss, ts, ls, h, entries


def pool_warp_args(n, sources, samples, centers, lines, pairs=None, half_width=1, entries=1):
    """Host checks of Plan.xcorr_pool_warp_f32: the pools, pairs and centers of pool_curve_args, lines as warp_args.  -> (sources,
    samples, pairs or None, centers, lines, batch, line_stride, half_width, entries).  ValueError on anything else."""
    s, t, pr, c, batch, h, entries = pool_curve_args(n, sources, samples, centers, pairs, half_width, entries)
    ln, ls = _lines(lines, c.shape)
    return s, t, pr, c, ln, batch, ls, h, entries


def position_rows(n, hop, batch, p_lo, p_hi):
    """Lag windows of Plan.xcorr_windows_f32(..., positions=(p_lo, p_hi)): window k (source frames k*hop .. k*hop + 2N - 1 of the
    recording, 0 <= k < batch) holds a sample that starts at recording frame k*hop + lag, so its rows are
    [p_lo - k*hop, p_hi - k*hop] clipped to [-N, N-1].  The windows whose clipped row is not empty are k0 <= k < k1, a contiguous
    range.  -> (k0, k1, rows int64 [k1 - k0, 2]); k0 == k1 when no window can hold such a start."""
    n, hop, batch, p_lo, p_hi = int(n), int(hop), int(batch), int(p_lo), int(p_hi)
    if hop < 1 or p_lo > p_hi:
        raise ValueError("need hop >= 1 and p_lo <= p_hi")
    # non-empty: p_lo - k hop <= N - 1 and p_hi - k hop >= -N
    k0 = max(0, -((n - 1 - p_lo) // hop))       # ceil((p_lo - N + 1) / hop)
    k1 = min(batch, (p_hi + n) // hop + 1)      # floor((p_hi + N) / hop) + 1
    if k1 <= k0:
        return 0, 0, np.zeros((0, 2), dtype=np.int64)
    k = np.arange(k0, k1, dtype=np.int64) * hop
    rows = np.stack([np.maximum(p_lo - k, -n), np.minimum(p_hi - k, n - 1)], axis=1)
    return k0, k1, np.ascontiguousarray(rows, dtype=np.int64)


class PinnedArray:
    """a numpy float64 array in page-locked host memory (asx_host_malloc): what audiosync_run() keeps its tracks in"""

    def __init__(self, count, dtype=np.float64):
        self.nbytes = int(count) * np.dtype(dtype).itemsize
        self._p = _handle(lib().asx_host_malloc(self.nbytes))
        buf = (ctypes.c_char * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(count))

    def close(self):
        if self._p:
            self.array = None
            lib().asx_host_free(self._p)
            self._p = None


def shard_range(total, nshards, shard):
    """block partition of a batch over shards (asx_shard_range): -> (start, count)"""
    start, count = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().asx_shard_range(total, nshards, shard, ctypes.byref(start), ctypes.byref(count)))
    return start.value, count.value


def result_bytes(width):
    return int(lib().asx_result_bytes(width))


class Comm:
    """One RCCL communicator over the devices of `plans` (one plan per device), created inside the library
    (ncclCommInitAll); `run` = asx_xcorr_batch_multi_dev: device-resident shards, one all-gather of the result records."""

    def __init__(self, plans):
        self.plans = list(plans)
        handles = (ctypes.c_void_p * len(self.plans))(*[p._h for p in self.plans])
        self._h = _handle(lib().asx_comm_create(handles, len(self.plans)))

    def run(self, d_sources, d_samples, counts, width, d_gathered):
        n = len(self.plans)
        assert len(d_sources) == len(d_samples) == len(counts) == len(d_gathered) == n
        src = (ctypes.c_void_p * n)(*d_sources)
        smp = (ctypes.c_void_p * n)(*d_samples)
        out = (ctypes.c_void_p * n)(*d_gathered)
        cnt = (ctypes.c_size_t * n)(*counts)
        _check(lib().asx_xcorr_batch_multi_dev(self._h, src, smp, cnt, width, out))

    def close(self):
        if self._h:
            lib().asx_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Stream:
    """asx_stream: both tracks resident in HBM, new frames appended, one plan per prefix length."""

    def __init__(self, max_sample_len, device=-1):
        self._h = _handle(lib().asx_stream_create(int(max_sample_len), int(device)))
        self._destroy = lib().asx_stream_destroy  # bound now: module globals may be gone at interpreter exit

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def append(self, source_frames, sample_frames):
        s = np.ascontiguousarray(source_frames, dtype=np.float64)
        t = np.ascontiguousarray(sample_frames, dtype=np.float64)
        _check(lib().asx_stream_append_f64(self._h, s.ctypes.data_as(c_f64p), s.size, t.ctypes.data_as(c_f64p), t.size))

    def lengths(self):
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        lib().asx_stream_lengths(self._h, a, b)
        return a.value, b.value

    def reset(self):
        lib().asx_stream_reset(self._h)

    def set_lag_window(self, lo, hi):
        """search the peak only at lags lo..hi (frames), clamped to [-n, n-1] for each prefix length n that xcorr correlates"""
        _check(lib().asx_stream_set_lag_window(self._h, int(lo), int(hi)))

    def xcorr(self, sample_len):
        lag = ctypes.c_long(0)
        coef = ctypes.c_double(0.0)
        ret = lib().asx_stream_xcorr(self._h, int(sample_len), ctypes.byref(lag), ctypes.byref(coef))
        return ret, lag.value, coef.value


class _Staging:
    """Device copies of one call's host arrays on a plan's device.  Inside the `with` block: upload() the inputs, output() the
    results' buffers, make the asynchronous _dev call with the pointers those returned, fetch() the results.  Every pointer handed
    out is freed once when the block ends, also when something raised in between."""

    def __init__(self, plan):
        self._plan, self._lib, self._ptrs, self._outs = plan, lib(), [], []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        while self._ptrs:
            self._lib.asx_device_free(self._ptrs.pop())

    def alloc(self, nbytes):
        """a device pointer to nbytes (at least 16) of the plan's device"""
        self._ptrs.append(_handle(self._lib.asx_device_malloc(max(int(nbytes), 16), self._plan.device)))
        return self._ptrs[-1]

    def upload(self, host):
        """a device pointer to a copy of the host array; None (an optional argument left out): 0"""
        if host is None:
            return 0
        ptr = self.alloc(host.nbytes)
        _check(self._lib.asx_memcpy_h2d(ptr, host.ctypes.data, host.nbytes))
        return ptr

    def output(self, shape, dtype):
        """a device pointer to room for an array that fetch() will return"""
        host = np.zeros(shape, dtype=dtype)
        self._outs.append((host, self.alloc(host.nbytes)))
        return self._outs[-1][1]

    def fetch(self):
        """wait for the plan's stream, then the outputs as host arrays, in the order they were reserved"""
        self._plan.sync()
        for host, ptr in self._outs:
            _check(self._lib.asx_memcpy_d2h(host.ctypes.data, ptr, host.nbytes))
        return tuple(host for host, _ in self._outs)


_RESULTS = (np.int64, np.float64, np.int32)                    # lag, coef, ret
_PHAT_RESULTS = (np.int64, np.float64, np.float64, np.int32)   # lag, coef, peak, ret


class Plan:
    """asx_plan: fixed sample_len, owns tables + HBM workspaces on one device."""

    def __init__(self, sample_len, max_batch=1, device=-1, split=None):
        self._h = _handle(lib().asx_plan_create_ex(int(sample_len), int(max_batch), int(device), _split_arg(split)))
        self._destroy = lib().asx_plan_destroy  # bound now: module globals may be gone at interpreter exit
        self.sample_len = int(sample_len)
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def fft_len(self):
        return lib().asx_plan_fft_len(self._h)

    @property
    def group(self):
        return lib().asx_plan_group(self._h)

    @property
    def peak_capacity(self):
        return lib().asx_plan_peak_capacity(self._h)

    def peak_overflows(self):
        """pairs (since plan creation) with more near-tied lags than the plan re-evaluates exactly"""
        return _counters(lib().asx_plan_peak_overflows, self._h, 1)[0]

    def set_lag_window(self, lo, hi):
        """search the peak only at lags lo..hi, -N <= lo <= hi <= N-1 (asx_plan_set_lag_window); (-N, N-1) = every lag, the default"""
        _check(lib().asx_plan_set_lag_window(self._h, int(lo), int(hi)))

    @property
    def lag_window(self):
        lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().asx_plan_lag_window(self._h, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def set_exact(self, on=True):
        """on (the default): every entry point takes the second look at overflowing pairs (the device-resident batch waits
        once per call for its kernels); off: that entry point stays asynchronous and marks such pairs with ret = 1"""
        _check(lib().asx_plan_set_exact(self._h, 1 if on else 0))

    def placement(self):
        """("measure" plans) -> ((ms of the forward column kernel on the first / second allocation of its workspaces), kept)"""
        ms = (ctypes.c_double * 2)()
        kept = ctypes.c_int(-1)
        _check(lib().asx_plan_placement(self._h, ms, ctypes.byref(kept)))
        return (float(ms[0]), float(ms[1])), int(kept.value)

    def set_pearson(self, spectral=True):
        """spectral (the default on real-column plans): the coefficient from r[peak] and the forward pass's band sums, no second
        pass over the inputs; False: the reference's reduction over both segments (include/audiosync/xcorr_hip.h)"""
        _check(lib().asx_plan_set_pearson(self._h, 1 if spectral else 0))

    def pearson_modes(self):
        """pairs so far that took (spectral, spectral + wrap-around correction, direct) under the spectral setting"""
        c = (ctypes.c_uint64 * 3)()
        _check(lib().asx_plan_pearson_modes(self._h, c))
        return tuple(int(v) for v in c)

    def set_prune(self, on=True):
        """on (the default on real-column plans): in-scope groups skip the inverse column tiles whose energy bound rules out the
        peak and its near-ties; same lag, ret and coefficient bits either way (include/audiosync/xcorr_hip.h)"""
        _check(lib().asx_plan_set_prune(self._h, 1 if on else 0))

    def prune_stats(self):
        """(column tiles the pruned groups transformed, tiles those groups had in all) over the plan's life"""
        return _counters(lib().asx_plan_prune_stats, self._h, 2)

    def set_qstore(self, mode=1):
        """partial storing of Q in the pruned pass: 0 off, 1 auto (large groups of the two longest lengths), 2 always; same lag, ret and
        coefficient bits in every mode (include/audiosync/xcorr_hip.h)"""
        _check(lib().asx_plan_set_qstore(self._h, int(mode)))

    def qstore_stats(self):
        """(pairs given a list, pairs that stored everything, pairs run again, tiles stored) over the plan's life"""
        c = (ctypes.c_uint64 * 4)()
        _check(lib().asx_plan_qstore_stats(self._h, c))
        return tuple(int(v) for v in c)

    def narrowed_calls(self):
        """xcorr_f64 calls whose frames were all exactly float32 and crossed PCIe as 4 bytes each"""
        return _counters(lib().asx_plan_narrowed_calls, self._h, 1)[0]

    def peak_repairs(self):
        """overflowing pairs that were looked at again with lists for all 2N lags"""
        return _counters(lib().asx_plan_peak_repairs, self._h, 1)[0]

    @property
    def workspace_bytes(self):
        return lib().asx_plan_workspace_bytes(self._h)

    @property
    def split(self):
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib().asx_plan_split(self._h, a, b, c)
        return a.value, b.value, c.value

    @property
    def layout(self):
        """'real-column' (csrc/rlayout.hip) or 'packed' (csrc/xcorr_kernels.hip): which decomposition this plan runs"""
        return "real-column" if lib().asx_plan_layout(self._h) == 1 else "packed"

    @property
    def threads(self):
        a, b = ctypes.c_int(), ctypes.c_int()
        lib().asx_plan_threads(self._h, a, b)
        return a.value, b.value

    def xcorr_f64(self, source, sample):
        """the reference's calling convention: -> (ret, lag, coefficient)"""
        s = np.ascontiguousarray(source, dtype=np.float64)
        t = np.ascontiguousarray(sample, dtype=np.float64)
        assert t.size == self.sample_len and s.size == 2 * self.sample_len
        lag = ctypes.c_long(0)
        coef = ctypes.c_double(0.0)
        ret = lib().asx_xcorr_f64(self._h, s.ctypes.data_as(c_f64p), t.ctypes.data_as(c_f64p),
                                  ctypes.byref(lag), ctypes.byref(coef))
        return ret, lag.value, coef.value

    def xcorr_batch_f32(self, source, sample):
        """host float32 arrays [B,2N], [B,N] -> (lag int64[B], coef float64[B], ret int32[B])"""
        s = np.ascontiguousarray(source, dtype=np.float32)
        t = np.ascontiguousarray(sample, dtype=np.float32)
        n = self.sample_len
        batch = t.size // n
        assert t.size == batch * n and s.size == 2 * n * batch
        lag = np.zeros(batch, dtype=np.int64)
        coef = np.zeros(batch, dtype=np.float64)
        ret = np.zeros(batch, dtype=np.int32)
        _check(lib().asx_xcorr_batch_f32(self._h, s.ctypes.data_as(c_f32p), t.ctypes.data_as(c_f32p), batch,
                                         lag.ctypes.data_as(c_i64p), coef.ctypes.data_as(c_f64p), ret.ctypes.data_as(c_i32p)))
        return lag, coef, ret

    def xcorr_batch_dev(self, d_src, d_smp, batch, d_lag, d_coef, d_ret, stream=0):
        """raw device pointers (ints); asynchronous on `stream` (0 = the plan's own)"""
        _check(lib().asx_xcorr_batch_f32_dev(self._h, d_src, d_smp, batch, d_lag or None, d_coef, d_ret or None, stream or None))

    def xcorr_strided_dev(self, d_src, src_stride, d_smp, smp_stride, batch, d_lag, d_coef, d_ret, stream=0):
        """raw device pointers (ints), strides in floats (0 = one track for every pair; see asx_xcorr_strided_f32_dev);
        asynchronous on `stream` (0 = the plan's own)"""
        _check(lib().asx_xcorr_strided_f32_dev(self._h, d_src, int(src_stride), d_smp, int(smp_stride), int(batch), d_lag or None,
                                               d_coef, d_ret or None, stream or None))

    def xcorr_windowed_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, d_lag, d_coef, d_ret,
                           stream=0):
        """raw device pointers (ints): asx_xcorr_windowed_f32_dev -- the strided batch with pair i's lag window at
        d_windows[2 i window_stride], d_windows[2 i window_stride + 1] (int64, device memory); asynchronous on `stream`"""
        _check(lib().asx_xcorr_windowed_f32_dev(self._h, d_src, int(src_stride), d_smp, int(smp_stride), d_windows, int(window_stride),
                                                int(batch), d_lag or None, d_coef, d_ret, stream or None))

    def xcorr_phat_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, d_lag, d_coef, d_peak, d_ret,
                       stream=0):
        """raw device pointers (ints): asx_xcorr_phat_f32_dev -- the strided batch ranked by the GCC-PHAT curve; d_windows = 0: the
        plan's window applies, else per-pair rows as in xcorr_windowed_dev; d_peak (float64, may be 0) receives |r_phat[lag]| / F;
        always asynchronous on `stream`"""
        _check(lib().asx_xcorr_phat_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride), d_windows or None,
                                            int(window_stride), int(batch), d_lag or None, d_coef or None, d_peak or None,
                                            d_ret or None, stream or None))

    def xcorr_ncc_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, min_energy, d_lag, d_coef, d_peak,
                      d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_f32_dev -- the strided batch with the lags 0..N-1 ranked by the Pearson
        coefficient itself; d_windows = 0: every lag 0..N-1, else per-pair rows inside [0, N-1]; peak: |c32[lag]|"""
        _check(lib().asx_xcorr_ncc_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride), d_windows or None,
                                           int(window_stride), int(batch), float(min_energy), d_lag or None, d_coef or None,
                                           d_peak or None, d_ret or None, stream or None))

    def xcorr_ncc_topk_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, min_energy, k, min_separation,
                           d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_topk_f32_dev -- xcorr_ncc_dev with the k strongest lags of the coefficient curve
        at least min_separation apart, entry j of pair i at index i*k + j of d_lag / d_coef / d_peak / d_ret"""
        _check(lib().asx_xcorr_ncc_topk_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                d_windows or None, int(window_stride), int(batch), float(min_energy), int(k),
                                                int(min_separation), d_lag or None, d_coef or None, d_peak or None, d_ret or None,
                                                stream or None))

    def xcorr_pool_ncc_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                           window_stride, batch, min_energy, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_ncc_f32_dev -- xcorr_pool_dev's pairs ranked by the Pearson coefficient of the
        lags 0..N-1; every track's transform and moments once per call; d_windows = 0: every lag 0..N-1"""
        _check(lib().asx_xcorr_pool_ncc_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                int(window_stride), int(batch), float(min_energy), d_lag or None, d_coef or None,
                                                d_peak or None, d_ret or None, stream or None))

    def xcorr_pool_ncc_topk_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                                window_stride, batch, min_energy, k, min_separation, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_ncc_topk_f32_dev -- xcorr_pool_ncc_dev with the k strongest separated lags of
        pair i, entry j at index i*k + j"""
        _check(lib().asx_xcorr_pool_ncc_topk_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                     int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                     int(window_stride), int(batch), float(min_energy), int(k), int(min_separation),
                                                     d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def ncc_debug_c_dev(self, d_src, d_smp, min_energy, d_c, d_lag, d_coef, d_peak, d_ret, stream=0):
        """asx_xcorr_ncc_debug_c_dev: one contiguous pair, c32 of lags 0..N-1 to d_c (NaN where the lag does not compete)"""
        _check(lib().asx_xcorr_ncc_debug_c_dev(self._h, d_src or None, d_smp or None, float(min_energy), d_c or None, d_lag or None,
                                               d_coef or None, d_peak or None, d_ret or None, stream or None))

    def xcorr_ncc_full_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, min_energy, min_overlap,
                           d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_full_f32_dev -- xcorr_ncc_dev over the lags -(N-1)..N-1; a negative lag competes
        with an overlap of at least min_overlap frames; d_windows = 0: every lag, else per-pair rows inside [-(N-1), N-1]"""
        _check(lib().asx_xcorr_ncc_full_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                d_windows or None, int(window_stride), int(batch), float(min_energy), int(min_overlap),
                                                d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def xcorr_ncc_full_topk_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, min_energy, min_overlap, k,
                                min_separation, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_full_topk_f32_dev -- xcorr_ncc_full_dev with the k strongest lags of the signed
        curve at least min_separation apart, entry j of pair i at index i*k + j of d_lag / d_coef / d_peak / d_ret"""
        _check(lib().asx_xcorr_ncc_full_topk_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                     d_windows or None, int(window_stride), int(batch), float(min_energy),
                                                     int(min_overlap), int(k), int(min_separation), d_lag or None, d_coef or None,
                                                     d_peak or None, d_ret or None, stream or None))

    def ncc_full_debug_c_dev(self, d_src, d_smp, min_energy, min_overlap, d_c, d_lag, d_coef, d_peak, d_ret, stream=0):
        """asx_xcorr_ncc_full_debug_c_dev: one contiguous pair, c32 of the lags -(N-1)..N-1 to d_c (2N - 1 floats, lag l at index
        l + N - 1, NaN where the lag does not compete)"""
        _check(lib().asx_xcorr_ncc_full_debug_c_dev(self._h, d_src or None, d_smp or None, float(min_energy), int(min_overlap),
                                                    d_c or None, d_lag or None, d_coef or None, d_peak or None, d_ret or None,
                                                    stream or None))

    def xcorr_ncc_ragged_dev(self, d_src, src_stride, d_smp, smp_stride, d_lengths, length_stride, d_windows, window_stride, batch,
                             min_energy, min_overlap, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_ragged_f32_dev -- xcorr_ncc_full_dev for pairs whose row (Ls, Lm) of d_lengths says
        how many frames of their tracks count; d_lengths = 0: (2N, N) for every pair; a row that is no pair of lengths: ret = -5"""
        _check(lib().asx_xcorr_ncc_ragged_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                  d_lengths or None, int(length_stride), d_windows or None, int(window_stride),
                                                  int(batch), float(min_energy), int(min_overlap), d_lag or None, d_coef or None,
                                                  d_peak or None, d_ret or None, stream or None))

    def xcorr_ncc_ragged_topk_dev(self, d_src, src_stride, d_smp, smp_stride, d_lengths, length_stride, d_windows, window_stride, batch,
                                  min_energy, min_overlap, k, min_separation, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_ncc_ragged_topk_f32_dev -- xcorr_ncc_ragged_dev with the k strongest lags of the signed
        curve at least min_separation apart, entry j of pair i at index i*k + j of d_lag / d_coef / d_peak / d_ret"""
        _check(lib().asx_xcorr_ncc_ragged_topk_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                       d_lengths or None, int(length_stride), d_windows or None, int(window_stride),
                                                       int(batch), float(min_energy), int(min_overlap), int(k), int(min_separation),
                                                       d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def ncc_ragged_debug_c_dev(self, d_src, d_smp, source_len, sample_len, min_energy, min_overlap, d_c, d_lag, d_coef, d_peak, d_ret,
                               stream=0):
        """asx_xcorr_ncc_ragged_debug_c_dev: one contiguous pair of the lengths (source_len, sample_len), c32 of the lags -(N-1)..N-1
        to d_c (2N - 1 floats, lag l at index l + N - 1, NaN where the lag does not exist or does not compete)"""
        _check(lib().asx_xcorr_ncc_ragged_debug_c_dev(self._h, d_src or None, d_smp or None, int(source_len), int(sample_len),
                                                      float(min_energy), int(min_overlap), d_c or None, d_lag or None, d_coef or None,
                                                      d_peak or None, d_ret or None, stream or None))

    def xcorr_pool_ncc_full_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                                window_stride, batch, min_energy, min_overlap, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_ncc_full_f32_dev -- xcorr_pool_ncc_dev over the lags -(N-1)..N-1; every track's
        transforms, moments and tables once per call; d_windows = 0: every lag, else per-pair rows inside [-(N-1), N-1]"""
        _check(lib().asx_xcorr_pool_ncc_full_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                     int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                     int(window_stride), int(batch), float(min_energy), int(min_overlap),
                                                     d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def xcorr_pool_ncc_full_topk_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                                     window_stride, batch, min_energy, min_overlap, k, min_separation, d_lag, d_coef, d_peak, d_ret,
                                     stream=0):
        """raw device pointers (ints): asx_xcorr_pool_ncc_full_topk_f32_dev -- xcorr_pool_ncc_full_dev with the k strongest lags of
        the signed curve at least min_separation apart, entry j of pair i at index i*k + j"""
        _check(lib().asx_xcorr_pool_ncc_full_topk_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources),
                                                          d_samples or None, int(sample_stride), int(nsamples), d_pairs or None,
                                                          d_windows or None, int(window_stride), int(batch), float(min_energy),
                                                          int(min_overlap), int(k), int(min_separation), d_lag or None,
                                                          d_coef or None, d_peak or None, d_ret or None, stream or None))

    def phat_debug_r_dev(self, d_src, d_smp, d_r, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_phat_debug_r_dev -- one contiguous pair, r_phat of all 2N lags (times F) to d_r"""
        _check(lib().asx_xcorr_phat_debug_r_dev(self._h, d_src or None, d_smp or None, d_r or None, d_lag or None, d_coef or None,
                                                d_peak or None, d_ret or None, stream or None))

    def xcorr_phat_band_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, bin_lo, bin_hi, d_lag, d_coef,
                            d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_phat_band_f32_dev -- xcorr_phat_dev in which only bins bin_lo..bin_hi of the
        2N-point transform vote (band_bins converts from Hz); d_peak receives |r_phat[lag]| / V, V the number of bins that vote"""
        _check(lib().asx_xcorr_phat_band_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                 d_windows or None, int(window_stride), int(batch), int(bin_lo), int(bin_hi),
                                                 d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def phat_band_debug_r_dev(self, d_src, d_smp, bin_lo, bin_hi, d_r, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_phat_band_debug_r_dev -- one contiguous pair, r_phat of all 2N lags (times V) to d_r"""
        _check(lib().asx_xcorr_phat_band_debug_r_dev(self._h, d_src or None, d_smp or None, int(bin_lo), int(bin_hi), d_r or None,
                                                     d_lag or None, d_coef or None, d_peak or None, d_ret or None, stream or None))

    def xcorr_topk_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, k, min_separation, d_lag, d_coef,
                       d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_topk_f32_dev -- the k strongest lags of pair i at least min_separation apart, entry j
        at index i*k + j of d_lag / d_coef / d_ret; d_windows = 0: the plan's window applies; asynchronous on `stream`"""
        _check(lib().asx_xcorr_topk_f32_dev(self._h, d_src, int(src_stride), d_smp, int(smp_stride), d_windows or None,
                                            int(window_stride), int(batch), int(k), int(min_separation), d_lag or None, d_coef,
                                            d_ret or None, stream or None))

    def xcorr_pool_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows, window_stride,
                       batch, d_lag, d_coef, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_f32_dev -- pair i is source d_pairs[2 i] of the source pool against sample
        d_pairs[2 i + 1] of the sample pool (int32, device memory); d_pairs = 0: every combination, source-major, batch =
        nsources * nsamples; d_windows = 0: the plan's window; asynchronous on `stream`"""
        _check(lib().asx_xcorr_pool_f32_dev(self._h, d_sources, int(source_stride), int(nsources), d_samples, int(sample_stride),
                                            int(nsamples), d_pairs or None, d_windows or None, int(window_stride), int(batch),
                                            d_lag or None, d_coef, d_ret, stream or None))

    def xcorr_pool_topk_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                            window_stride, batch, k, min_separation, d_lag, d_coef, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_topk_f32_dev -- xcorr_pool_dev's pairs with the k strongest lags of pair i at
        least min_separation apart, entry j at index i*k + j of d_lag / d_coef / d_ret; asynchronous on `stream`"""
        _check(lib().asx_xcorr_pool_topk_f32_dev(self._h, d_sources, int(source_stride), int(nsources), d_samples, int(sample_stride),
                                                 int(nsamples), d_pairs or None, d_windows or None, int(window_stride), int(batch),
                                                 int(k), int(min_separation), d_lag or None, d_coef, d_ret, stream or None))

    def xcorr_pool_phat_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                            window_stride, batch, bin_lo, bin_hi, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_phat_f32_dev -- xcorr_pool_dev's pairs ranked by the GCC-PHAT curve in which
        bins bin_lo..bin_hi vote ((0, N): every bin); d_peak (float64, may be 0) receives |r_phat[lag]| / V; always asynchronous on
        `stream`"""
        _check(lib().asx_xcorr_pool_phat_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                 int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                 int(window_stride), int(batch), int(bin_lo), int(bin_hi), d_lag or None,
                                                 d_coef or None, d_peak or None, d_ret or None, stream or None))

    def xcorr_phat_sub_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, bin_lo, bin_hi, half_width,
                           d_lag, d_coef, d_peak, d_frac, d_near, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_phat_sub_f32_dev -- xcorr_phat_band_dev, plus d_near (float64 [batch][2 half_width
        + 1], may be 0): r_phat / V at the indices around each pair's peak, and d_frac (float64 [batch]): the parabolic vertex of
        the three centre values, so that the delay is lag + frac frames"""
        _check(lib().asx_xcorr_phat_sub_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                d_windows or None, int(window_stride), int(batch), int(bin_lo), int(bin_hi),
                                                int(half_width), d_lag or None, d_coef or None, d_peak or None, d_frac or None,
                                                d_near or None, d_ret or None, stream or None))

    def xcorr_pool_phat_sub_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                                window_stride, batch, bin_lo, bin_hi, half_width, d_lag, d_coef, d_peak, d_frac, d_near, d_ret,
                                stream=0):
        """raw device pointers (ints): asx_xcorr_pool_phat_sub_f32_dev -- xcorr_pool_phat_dev with d_frac and d_near as in
        xcorr_phat_sub_dev"""
        _check(lib().asx_xcorr_pool_phat_sub_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                     int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                     int(window_stride), int(batch), int(bin_lo), int(bin_hi), int(half_width),
                                                     d_lag or None, d_coef or None, d_peak or None, d_frac or None, d_near or None,
                                                     d_ret or None, stream or None))

    def xcorr_phat_topk_dev(self, d_src, src_stride, d_smp, smp_stride, d_windows, window_stride, batch, bin_lo, bin_hi, k,
                            min_separation, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_phat_topk_f32_dev -- xcorr_phat_band_dev's pairs with the k strongest lags of r_phat
        at least min_separation apart, entry j of pair i at index i*k + j of d_lag / d_coef / d_peak / d_ret (d_lag and d_peak may be
        0); always asynchronous on `stream`"""
        _check(lib().asx_xcorr_phat_topk_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride),
                                                 d_windows or None, int(window_stride), int(batch), int(bin_lo), int(bin_hi), int(k),
                                                 int(min_separation), d_lag or None, d_coef or None, d_peak or None, d_ret or None,
                                                 stream or None))

    def xcorr_pool_phat_topk_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, d_windows,
                                 window_stride, batch, bin_lo, bin_hi, k, min_separation, d_lag, d_coef, d_peak, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_phat_topk_f32_dev -- xcorr_pool_phat_dev's pairs with the entries of
        xcorr_phat_topk_dev"""
        _check(lib().asx_xcorr_pool_phat_topk_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                      int(sample_stride), int(nsamples), d_pairs or None, d_windows or None,
                                                      int(window_stride), int(batch), int(bin_lo), int(bin_hi), int(k),
                                                      int(min_separation), d_lag or None, d_coef or None, d_peak or None,
                                                      d_ret or None, stream or None))

    def xcorr_curve_dev(self, d_src, src_stride, d_smp, smp_stride, batch, entries, d_center, half_width, d_r, d_coef, d_frac, d_ret,
                        stream=0):
        """raw device pointers (ints): asx_xcorr_curve_f32_dev -- around each of the batch * entries lags of d_center (int64), the
        exact r (d_r) and the Pearson coefficient (d_coef, may be 0: not computed) at the 2 half_width + 1 neighbouring indices,
        float64 [batch * entries][2 half_width + 1], the parabolic vertex d_frac and d_ret, [batch * entries]"""
        _check(lib().asx_xcorr_curve_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride), int(batch),
                                             int(entries), d_center or None, int(half_width), d_r or None, d_coef or None,
                                             d_frac or None, d_ret or None, stream or None))

    def xcorr_pool_curve_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, batch, entries,
                             d_center, half_width, d_r, d_coef, d_frac, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_curve_f32_dev -- xcorr_curve_dev for the pairs of xcorr_pool_dev"""
        _check(lib().asx_xcorr_pool_curve_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                  int(sample_stride), int(nsamples), d_pairs or None, int(batch), int(entries),
                                                  d_center or None, int(half_width), d_r or None, d_coef or None, d_frac or None,
                                                  d_ret or None, stream or None))

    def xcorr_track_dev(self, d_src, src_stride, d_smp, smp_stride, batch, entries, d_center, half_width, segments, d_r, d_seg, d_fit,
                        d_used, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_track_f32_dev -- around each of the batch * entries lags of d_center (int64), r per
        time segment (d_r, float64 [batch * entries][segments][2 half_width + 1]), each segment's {offset, weight} (d_seg, [..][segments]
        [2], may be 0), the drift line {drift, lag0, rms} (d_fit, [..][3]), the used segments (d_used, int32) and d_ret"""
        _check(lib().asx_xcorr_track_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride), int(batch),
                                             int(entries), d_center or None, int(half_width), int(segments), d_r or None,
                                             d_seg or None, d_fit or None, d_used or None, d_ret or None, stream or None))

    def xcorr_pool_track_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, batch, entries,
                             d_center, half_width, segments, d_r, d_seg, d_fit, d_used, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_track_f32_dev -- xcorr_track_dev for the pairs of xcorr_pool_dev"""
        _check(lib().asx_xcorr_pool_track_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                  int(sample_stride), int(nsamples), d_pairs or None, int(batch), int(entries),
                                                  d_center or None, int(half_width), int(segments), d_r or None, d_seg or None,
                                                  d_fit or None, d_used or None, d_ret or None, stream or None))

    def xcorr_warp_dev(self, d_src, src_stride, d_smp, smp_stride, batch, entries, d_center, d_line, line_stride, half_width, d_r,
                       d_frac, d_coef, d_len, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_warp_f32_dev -- along each entry's line {drift, lag0} (d_line, float64, entry e's at
        e * line_stride; 0: one line for all) through its lag of d_center (int64): r at the 2 half_width + 1 offsets across the line
        (d_r, float64), the vertex across it (d_frac), the Pearson coefficient of the frames that line up (d_coef), their number
        (d_len, int64, may be 0) and d_ret"""
        _check(lib().asx_xcorr_warp_f32_dev(self._h, d_src or None, int(src_stride), d_smp or None, int(smp_stride), int(batch),
                                            int(entries), d_center or None, d_line or None, int(line_stride), int(half_width),
                                            d_r or None, d_frac or None, d_coef or None, d_len or None, d_ret or None, stream or None))

    def xcorr_pool_warp_dev(self, d_sources, source_stride, nsources, d_samples, sample_stride, nsamples, d_pairs, batch, entries,
                            d_center, d_line, line_stride, half_width, d_r, d_frac, d_coef, d_len, d_ret, stream=0):
        """raw device pointers (ints): asx_xcorr_pool_warp_f32_dev -- xcorr_warp_dev for the pairs of xcorr_pool_dev"""
        _check(lib().asx_xcorr_pool_warp_f32_dev(self._h, d_sources or None, int(source_stride), int(nsources), d_samples or None,
                                                 int(sample_stride), int(nsamples), d_pairs or None, int(batch), int(entries),
                                                 d_center or None, d_line or None, int(line_stride), int(half_width), d_r or None,
                                                 d_frac or None, d_coef or None, d_len or None, d_ret or None, stream or None))

    def debug_prune(self, pair=0):
        """diagnostic: (upper bounds of |r| per column tile, the largest-bound tile) of `pair` of the last pruned group"""
        n = (self.split[1] + self.split[2] - 1) // self.split[2]
        ub = (ctypes.c_float * n)()
        best = ctypes.c_int(-1)
        _check(lib().asx_plan_debug_prune(self._h, int(pair), ub, ctypes.byref(best), n), "asx_plan_debug_prune failed")
        return np.frombuffer(ub, dtype=np.float32).copy(), int(best.value)

    def debug_peak(self, pair=0):
        """diagnostic: the peak-search state of `pair` of the last group on lane 0 (asx_plan_debug_peak) -- bound2 (2B in the
        device's scale, F times the plain sum), cand_n, refine_n, the float32 maximum's (key, index) decoded from pairmax (None,
        None when nothing competed), and the near-tie list refine_idx[:refine_n] with its exact values refine_val[:refine_n]"""
        cap = self.peak_capacity
        b2, cn, rn, pm = ctypes.c_float(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        vals, idxs = np.zeros(cap, dtype=np.float64), np.zeros(cap, dtype=np.uint32)
        _check(lib().asx_plan_debug_peak(self._h, int(pair), ctypes.byref(b2), ctypes.byref(cn), ctypes.byref(rn), ctypes.byref(pm),
                                         vals.ctypes.data, idxs.ctypes.data, cap), "asx_plan_debug_peak failed")
        key = index = None
        if pm.value:   # peak_pack_key (csrc/xcorr_dev.h): an order-preserving key in the high word, ~index in the low word
            hi = pm.value >> 32
            hi = (hi & 0x7FFFFFFF) if hi & 0x80000000 else (~hi & 0xFFFFFFFF)
            key = float(np.array([hi], dtype=np.uint32).view(np.float32)[0])
            index = 0xFFFFFFFF - (pm.value & 0xFFFFFFFF)
        n = min(int(rn.value), cap)
        return {"bound2": float(b2.value), "cand_n": int(cn.value), "refine_n": int(rn.value), "key": key, "index": index,
                "refine_idx": idxs[:n].astype(np.int64), "refine_val": vals[:n].copy()}

    def debug_spectral(self, pair=0):
        """diagnostic (real-column plans): what the spectral Pearson form built the coefficient of `pair` of the last group on lane 0
        from (asx_plan_debug_spectral) -- band: float32 [2][ntiles][nbands][2], {sum, sum of squares} of every band x tile cell of
        the source (0) and the sample (1: only bands < nbands / 2 exist); nbands, band_rows, prep_blocks; the header r, rb, direct,
        mode; seg: the pair's segment; pick: asx_spec_pick as a one-thread kernel evaluates it from that state"""
        ntiles = (self.split[1] + self.split[2] - 1) // self.split[2]
        f = lib().asx_plan_debug_spectral
        dims, hdr, seg, pick = (ctypes.c_int * 4)(), (ctypes.c_double * 4)(), (ctypes.c_longlong * 6)(), (ctypes.c_double * 8)()
        _check(f(self._h, int(pair), dims, None, 0, hdr, seg, pick),
               "asx_plan_debug_spectral failed (a real-column plan that has run a group?)")
        assert dims[0] == ntiles, (dims[0], ntiles)
        band = np.zeros((2, dims[0], dims[1], 2), dtype=np.float32)
        _check(f(self._h, int(pair), dims, band.ctypes.data, band.size, hdr, seg, pick), "asx_plan_debug_spectral failed")
        return {"band": band, "nbands": dims[1], "band_rows": dims[2], "prep_blocks": dims[3],
                "r": hdr[0], "rb": hdr[1], "direct": hdr[2] != 0.0, "mode": int(hdr[3]),
                "seg": dict(zip(("lag", "src_off", "smp_off", "len", "peak", "flags"), (int(v) for v in seg))),
                "pick": dict(zip(("mode", "n", "Sx", "Sxx", "Sy", "Syy", "r", "bound"),
                                 (int(pick[0]),) + tuple(float(v) for v in pick[1:])))}

    def debug_kernels(self):
        """the kernels this plan runs, as planmath_kernels spells them: the record made when the plan was built"""
        f = lib().asx_plan_debug_kernels
        return _kernel_choice(lambda *a: f(self._h, *a))

    def debug_bank(self):
        """(source tracks, sample tracks) the plan's pool bank holds, and how many pool calls have filled it"""
        return _counters(lib().asx_plan_debug_bank, self._h, 3, "asx_plan_debug_bank failed")

    def debug_ncc(self):
        """(source tracks, sample tracks) the plan's NCC track set holds, and the source tables and sample moment sets every NCC call
        on this plan has built so far"""
        c = (ctypes.c_uint64 * 4)()
        _check(lib().asx_plan_debug_ncc(self._h, c), "asx_plan_debug_ncc failed")
        return tuple(int(v) for v in c)

    def debug_ncc_full(self):
        """(source tracks, sample tracks) the plan's full-range pool track set holds, and the sources staged (x_lo and its prefix
        table) and the sample suffix tables built by the pool full-range calls on this plan so far"""
        c = (ctypes.c_uint64 * 4)()
        _check(lib().asx_plan_debug_ncc_full(self._h, c), "asx_plan_debug_ncc_full failed")
        return tuple(int(v) for v in c)

    def debug_ncc_ragged(self):
        """(pairs per group, bytes) of the plan's ragged NCC set; (0, 0) until the plan's first ragged call"""
        c = (ctypes.c_uint64 * 2)()
        _check(lib().asx_plan_debug_ncc_ragged(self._h, c), "asx_plan_debug_ncc_ragged failed")
        return tuple(int(v) for v in c)

    NCC_TABLE_SETS = {"strided": 0, "pool": 1, "full": 2}
    # the track sets that hold the full-range tables of a pool's tracks (tests/test_ncc_exact.py holds NCC_TABLE_SETS to its three)
    NCC_POOL_TABLE_SETS = {"pool_full": 3}

    def debug_ncc_tables(self, which, source_track=0, sample_track=0):
        """diagnostic: the float64 tables behind the coefficient as the last call left them (asx_plan_debug_ncc_tables).  which:
        "strided" (the tracks of the last NCC group; one track where the stride was 0), "pool" (the plan's track set), "full" (the
        full-range set) or "pool_full" (the pool full-range calls' track set, indexed by pool track).  -> {"mu", "vmax" of the source
        track; "mean_y", "sy", "vy" of the sample track; "table": float64 [N, 2], {Sx' (mu-shifted), Vx} per lag; and for "full" and
        "pool_full" "ptab", "ttab": [N, 2] at the overlaps m = 1..N-1, row 0 NaN (never written)}.  AsxError where the set does not
        exist or a track is outside it."""
        n = self.sample_len
        sstat, ystat = np.zeros(2, dtype=np.float64), np.zeros(3, dtype=np.float64)
        table = np.zeros((n, 2), dtype=np.float64)
        full = which in ("full", "pool_full")
        ptab, ttab = (np.full((n, 2), np.nan, dtype=np.float64) for _ in range(2)) if full else (None, None)
        sets = dict(self.NCC_TABLE_SETS, **self.NCC_POOL_TABLE_SETS)
        _check(lib().asx_plan_debug_ncc_tables(self._h, sets[which], int(source_track), int(sample_track),
                                               sstat.ctypes.data, ystat.ctypes.data, table.ctypes.data,
                                               ptab.ctypes.data if full else None, ttab.ctypes.data if full else None))
        out = {"mu": float(sstat[0]), "vmax": float(sstat[1]), "mean_y": float(ystat[0]), "sy": float(ystat[1]), "vy": float(ystat[2]),
               "table": table}
        if full:
            out["ptab"], out["ttab"] = ptab, ttab
        return out

    def debug_over_list(self):
        """diagnostic: the plan's list of overflowed pairs as it stands, (count on the device, count of the host's mirror), read
        without emptying it"""
        d, h = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().asx_plan_debug_over_list(self._h, ctypes.byref(d), ctypes.byref(h)), "asx_plan_debug_over_list failed")
        return d.value, h.value

    def debug_stamps(self, cap):
        """diagnostic (a -DASX_STAMPS build run under ASX_STAMPS): the cycle stamps the last stamped kernel's blocks wrote, at most
        `cap` of them, as a uint64 array of 8 per block"""
        buf = np.zeros(int(cap), dtype=np.uint64)
        got = lib().asx_plan_debug_stamps(self._h, buf.ctypes.data, buf.size)
        if got < 0:
            raise AsxError("asx_plan_debug_stamps failed (a plan created under ASX_STAMPS?)")
        return buf[:got]

    def _staged(self, inputs, shape, dtypes, launch):
        """host arrays `inputs` (None: a null pointer) -> device copies; launch(*input pointers, *output pointers) makes the _dev
        call; -> the outputs, one host array of `shape` per dtype of `dtypes`"""
        with _Staging(self) as st:
            d_in = [st.upload(a) for a in inputs]
            d_out = [st.output(shape, dt) for dt in dtypes]
            launch(*d_in, *d_out)
            return st.fetch()

    def xcorr_pool_f32(self, sources, samples, pairs=None, windows=None):
        """Many tracks against many (asx_xcorr_pool_f32_dev): sources float32 [S, 2N], samples [R, N]; pairs None (every combination)
        or integers [B, 2] rows (source index, sample index); windows None (the plan's window) or integers [2] / [B, 2] as in
        xcorr_windowed_f32.  Every track is transformed once per call.  Shapes are checked on the host (ValueError) before anything is
        uploaded; an index outside its pool gives that pair (0, NaN, -4).  Returns (lag int64, coef float64, ret int32) of shape [B],
        or [S, R] when pairs is None."""
        n = self.sample_len
        s, t, pr, w, batch, ws = pool_args(n, sources, samples, pairs, windows)
        shape = (batch,) if pr is not None else (s.shape[0], t.shape[0])
        return self._staged((s, t, pr, w), shape, _RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, *d_out))

    def xcorr_pool_topk_f32(self, sources, samples, k, min_separation, pairs=None, windows=None):
        """The k strongest separated lags per pair of two pools (asx_xcorr_pool_topk_f32_dev): the pools, pairs and windows of
        xcorr_pool_f32, k and min_separation of xcorr_topk_f32.  Every track is transformed once per call, whatever k is.  Arguments
        are checked on the host (ValueError) before anything is uploaded.  Returns (lag int64, coef float64, ret int32) of shape
        [B, k], or [S, R, k] when pairs is None; ret = -3 where no lag was left, -4 in all k entries of a pair with an index outside
        its pool."""
        n = self.sample_len
        s, t, pr, w, batch, ws, k, sep = pool_topk_args(n, sources, samples, k, min_separation, pairs, windows)
        shape = ((batch,) if pr is not None else (s.shape[0], t.shape[0])) + (k,)
        return self._staged((s, t, pr, w), shape, _RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_topk_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, k, sep, *d_out))

    def xcorr_pool_phat_f32(self, sources, samples, pairs=None, windows=None, band=None):
        """Pairs of two pools ranked by the GCC-PHAT curve (asx_xcorr_pool_phat_f32_dev): the pools, pairs and windows of
        xcorr_pool_f32; band None (every bin votes) or (bin_lo, bin_hi) as in xcorr_phat_band_f32.  Every track is transformed once
        per call.  Arguments are checked on the host (ValueError) before anything is uploaded.  Returns (lag int64, coef float64,
        peak float64, ret int32) of shape [B], or [S, R] when pairs is None; a pair with an index outside its pool gets
        (0, NaN, NaN, -4)."""
        n = self.sample_len
        s, t, pr, w, batch, ws, lo, hi = pool_phat_args(n, sources, samples, pairs, windows, band)
        shape = (batch,) if pr is not None else (s.shape[0], t.shape[0])
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_phat_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, lo, hi, *d_out))

    def xcorr_phat_topk_f32(self, source, sample, k, min_separation, windows=None, band=None):
        """The k strongest separated lags per pair by the GCC-PHAT curve (asx_xcorr_phat_topk_f32_dev).  source, sample, windows and
        band as in xcorr_phat_f32; k and min_separation as in xcorr_topk_f32.  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag int64[B, k], coef float64[B, k], peak float64[B, k], ret int32[B, k]); ret = -3 (and a NaN
        peak) where no lag was left.  Entry 0 is xcorr_phat_f32's result."""
        s, t, w, batch, ss, ts, ws, lo, hi, k, sep = phat_topk_args(self.sample_len, source, sample, k, min_separation, windows, band)
        return self._staged((s, t, w), (batch, k), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_phat_topk_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, lo, hi, k, sep, *d_out))

    def xcorr_pool_phat_topk_f32(self, sources, samples, k, min_separation, pairs=None, windows=None, band=None):
        """The k strongest separated lags per pair of two pools by the GCC-PHAT curve (asx_xcorr_pool_phat_topk_f32_dev): the pools,
        pairs, windows and band of xcorr_pool_phat_f32, k and min_separation of xcorr_topk_f32.  Every track is transformed once per
        call, whatever k is.  Returns (lag, coef, peak, ret) of shape [B, k], or [S, R, k] when pairs is None -- the tables
        pool_closure takes; ret = -3 where no lag was left, -4 in all k entries of a pair with an index outside its pool."""
        n = self.sample_len
        s, t, pr, w, batch, ws, lo, hi, k, sep = pool_phat_topk_args(n, sources, samples, k, min_separation, pairs, windows, band)
        shape = ((batch,) if pr is not None else (s.shape[0], t.shape[0])) + (k,)
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_phat_topk_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, lo, hi, k, sep, *d_out))

    def _staged_sub(self, inputs, shape, h, launch):
        """_staged for the sub-sample PHAT calls: outputs (lag, coef, peak, frac, near, ret), near of shape + (2h + 1,)"""
        with _Staging(self) as st:
            d_in = [st.upload(a) for a in inputs]
            d_out = [st.output(shape, np.int64), st.output(shape, np.float64), st.output(shape, np.float64),
                     st.output(shape, np.float64), st.output(tuple(shape) + (2 * h + 1,), np.float64), st.output(shape, np.int32)]
            launch(*d_in, *d_out)
            return st.fetch()

    def xcorr_phat_sub_f32(self, source, sample, windows=None, band=None, half_width=1):
        """xcorr_phat_f32 with the curve around each peak and a fractional lag (asx_xcorr_phat_sub_f32_dev).  source, sample,
        windows and band as in xcorr_phat_f32; half_width h in [1, NEAR_MAX].  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag, coef, peak, frac float64[B], near float64[B, 2h + 1], ret): near[i, d + h] is r_phat /
        V at index (peak index + d) mod 2N, signed; frac the vertex of the parabola through near[i, h - 1 : h + 2], so that the delay
        estimate is lag + frac frames."""
        s, t, w, batch, ss, ts, ws, lo, hi, h = phat_sub_args(self.sample_len, source, sample, windows, band, half_width)
        return self._staged_sub((s, t, w), (batch,), h, lambda d_s, d_t, d_w, *d_out: self.xcorr_phat_sub_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, lo, hi, h, *d_out))

    def xcorr_pool_phat_sub_f32(self, sources, samples, pairs=None, windows=None, band=None, half_width=1):
        """xcorr_pool_phat_f32 with the curve around each peak and a fractional lag (asx_xcorr_pool_phat_sub_f32_dev): half_width,
        frac and near as in xcorr_phat_sub_f32.  Returns (lag, coef, peak, frac, near, ret) of shape [B] (near: [B, 2h + 1]), or
        [S, R] (near: [S, R, 2h + 1]) when pairs is None; a pair with ret -2 or -4 has NaN in frac and near."""
        n = self.sample_len
        s, t, pr, w, batch, ws, lo, hi, h = pool_phat_sub_args(n, sources, samples, pairs, windows, band, half_width)
        shape = (batch,) if pr is not None else (s.shape[0], t.shape[0])
        return self._staged_sub((s, t, pr, w), shape, h, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_phat_sub_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, lo, hi, h, *d_out))

    def _staged_curve(self, inputs, shape, h, coef, launch):
        """_staged for the curve calls: outputs (r, coef, frac, ret), r and coef of shape + (2h + 1,); coef False: a null d_coef, and
        None in its place"""
        with _Staging(self) as st:
            d_in = [st.upload(a) for a in inputs]
            wide = tuple(shape) + (2 * h + 1,)
            d_r = st.output(wide, np.float64)
            d_coef = st.output(wide, np.float64) if coef else 0
            launch(*d_in, d_r, d_coef, st.output(shape, np.float64), st.output(shape, np.int32))
            out = st.fetch()
            return out if coef else (out[0], None) + out[1:]

    def xcorr_curve_f32(self, source, sample, centers, half_width=1, entries=1, coef=True):
        """The exact correlation curve around given lags (asx_xcorr_curve_f32_dev), behind any call on the lags it returned.  source:
        float32 [2N] or [B, 2N]; sample: [N] or [B, N]; centers: integers [B, entries] (or [B] when entries == 1), the lag output of
        xcorr_topk_f32 with k = entries as it is.  Arguments are checked on the host (ValueError) before anything is uploaded.
        Returns (r, coef, frac, ret): r[..., d + h] the time-domain sum at index (centre's index + d) mod 2N in float64, coef the
        reference's Pearson coefficient at that lag in the direct form (None with coef=False: no Pearson pass), both of the shape of
        centers + (2h + 1,); frac the vertex of the parabola through r[..., h - 1 : h + 2] and ret (0, or -2 for a centre outside
        [-N, N-1], whose values are NaN) of the shape of centers."""
        s, t, c, batch, ss, ts, h, entries = curve_args(self.sample_len, source, sample, centers, half_width, entries)
        return self._staged_curve((s, t, c), c.shape, h, coef, lambda d_s, d_t, d_c, *d_out: self.xcorr_curve_dev(
            d_s, ss, d_t, ts, batch, entries, d_c, h, *d_out))

    def xcorr_pool_curve_f32(self, sources, samples, centers, pairs=None, half_width=1, entries=1, coef=True):
        """xcorr_curve_f32 for pairs of two pools (asx_xcorr_pool_curve_f32_dev): the pools and pairs of xcorr_pool_f32, centers
        integers [B, entries] (or [B] when entries == 1) with pairs, [S, R, entries] (or [S, R]) without.  Returns (r, coef, frac,
        ret) as xcorr_curve_f32; every entry of a pair with an index outside its pool has ret -4 and NaN values."""
        n = self.sample_len
        s, t, pr, c, batch, h, entries = pool_curve_args(n, sources, samples, centers, pairs, half_width, entries)
        return self._staged_curve((s, t, pr, c), c.shape, h, coef, lambda d_s, d_t, d_pr, d_c, *d_out: self.xcorr_pool_curve_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, batch, entries, d_c, h, *d_out))

    def _staged_track(self, inputs, shape, h, segs, launch):
        """_staged for the track calls: outputs (r, seg, fit, used, ret) of shape + (S, 2h + 1), (S, 2), (3,), () and ()"""
        with _Staging(self) as st:
            d_in = [st.upload(a) for a in inputs]
            shape = tuple(shape)
            launch(*d_in, st.output(shape + (segs, 2 * h + 1), np.float64), st.output(shape + (segs, 2), np.float64),
                   st.output(shape + (3,), np.float64), st.output(shape, np.int32), st.output(shape, np.int32))
            return st.fetch()

    def xcorr_track_f32(self, source, sample, centers, half_width, segments, entries=1):
        """A lag track around given lags (asx_xcorr_track_f32_dev), behind any call on the lags it returned: the curve's sum kept
        apart per time segment, and the drift line through the segments' peaks.  source, sample, centers and entries as in
        xcorr_curve_f32; half_width h in [1, TRACK_HALF_MAX]; segments S in [1, min(TRACK_SEG_MAX, N)].  Arguments are checked on the
        host (ValueError) before anything is uploaded.  Returns (r, seg, fit, used, ret): r[..., s, d + h] the sum over segment s
        (the sample's frames floor(s N / S) .. floor((s + 1) N / S) - 1) at index (centre's index + d) mod 2N, seg[..., s, :] =
        (offset of the segment's peak from the centre, its weight |r|), fit[..., :] = (drift in frames per frame, lag0, rms) of the
        weighted line through the used segments (NaN with fewer than two), used their number, ret 0 or -2 (a centre outside
        [-N, N-1]: NaN values, used 0) -- of the shape of centers plus the trailing axes named."""
        s, t, c, batch, ss, ts, h, segs, entries = track_args(self.sample_len, source, sample, centers, half_width, segments, entries)
        return self._staged_track((s, t, c), c.shape, h, segs, lambda d_s, d_t, d_c, *d_out: self.xcorr_track_dev(
            d_s, ss, d_t, ts, batch, entries, d_c, h, segs, *d_out))

    def xcorr_pool_track_f32(self, sources, samples, centers, half_width, segments, pairs=None, entries=1):
        """xcorr_track_f32 for pairs of two pools (asx_xcorr_pool_track_f32_dev): the pools, pairs and centers of
        xcorr_pool_curve_f32.  Returns (r, seg, fit, used, ret) as xcorr_track_f32; every entry of a pair with an index outside its
        pool has ret -4, NaN values and used 0."""
        n = self.sample_len
        s, t, pr, c, batch, h, segs, entries = pool_track_args(n, sources, samples, centers, half_width, segments, pairs, entries)
        return self._staged_track((s, t, pr, c), c.shape, h, segs, lambda d_s, d_t, d_pr, d_c, *d_out: self.xcorr_pool_track_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, batch, entries, d_c, h, segs, *d_out))

    def _staged_warp(self, inputs, shape, h, launch):
        """_staged for the warp calls: outputs (r, frac, coef, length, ret), r of shape + (2h + 1,)"""
        with _Staging(self) as st:
            d_in = [st.upload(a) for a in inputs]
            shape = tuple(shape)
            launch(*d_in, st.output(shape + (2 * h + 1,), np.float64), st.output(shape, np.float64), st.output(shape, np.float64),
                   st.output(shape, np.int64), st.output(shape, np.int32))
            return st.fetch()

    def xcorr_warp_f32(self, source, sample, centers, lines, half_width=1, entries=1):
        """The correlation along a drift line (asx_xcorr_warp_f32_dev), behind the track call on the line it fitted: sample frame n
        meets source frame n + centre + k_n, k_n = floor((lag0 + drift * n) + 0.5).  source, sample, centers, half_width and entries as
        in xcorr_curve_f32; lines: float64 {drift, lag0} -- [2] or [3] (one line for every entry), or of the shape of centers + (2,)
        or + (3,) (xcorr_track_f32's fit as it is).  Arguments are checked on the host (ValueError) before anything is uploaded.
        Returns (r, frac, coef, length, ret): r[..., d + h] the sum at the offset d across the line, frac the vertex of the parabola
        through r[..., h - 1 : h + 2], coef the reference's Pearson coefficient of the frames that line up at d = 0 and length their
        number, ret 0, -1 (a NaN coefficient), -2 (a centre outside [-N, N-1]) or -5 (a line that is not valid: not finite, |drift| >
        WARP_DRIFT_MAX or |lag0| > N), the last two with NaN values and length 0 -- of the shape of centers, r + (2h + 1,)."""
        s, t, c, ln, batch, ss, ts, ls, h, entries = warp_args(self.sample_len, source, sample, centers, lines, half_width, entries)
        return self._staged_warp((s, t, c, ln), c.shape, h, lambda d_s, d_t, d_c, d_ln, *d_out: self.xcorr_warp_dev(
            d_s, ss, d_t, ts, batch, entries, d_c, d_ln, ls, h, *d_out))

    def xcorr_pool_warp_f32(self, sources, samples, centers, lines, pairs=None, half_width=1, entries=1):
        """xcorr_warp_f32 for pairs of two pools (asx_xcorr_pool_warp_f32_dev): the pools, pairs and centers of xcorr_pool_curve_f32.
        Returns (r, frac, coef, length, ret) as xcorr_warp_f32; every entry of a pair with an index outside its pool has ret -4, NaN
        values and length 0."""
        n = self.sample_len
        s, t, pr, c, ln, batch, ls, h, entries = pool_warp_args(n, sources, samples, centers, lines, pairs, half_width, entries)
        return self._staged_warp((s, t, pr, c, ln), c.shape, h, lambda d_s, d_t, d_pr, d_c, d_ln, *d_out: self.xcorr_pool_warp_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, batch, entries, d_c, d_ln, ls, h, *d_out))

    def xcorr_topk_f32(self, source, sample, k, min_separation, windows=None):
        """The k strongest separated lags per pair (asx_xcorr_topk_f32_dev).  source: float32 [2N] or [B, 2N]; sample: [N] or [B, N];
        windows: None (the plan's window), or integers [2] / [B, 2] as in xcorr_windowed_f32.  Entry j is the largest |r| among the
        window's lags farther than min_separation from entries 0..j-1.  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag int64 [B, k], coef float64 [B, k], ret int32 [B, k]); ret = -3 where no lag was left."""
        s, t, w, batch, ss, ts, ws, k, sep = topk_args(self.sample_len, source, sample, k, min_separation, windows)
        return self._staged((s, t, w), (batch, k), _RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_topk_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, k, sep, *d_out))

    def xcorr_ncc_f32(self, source, sample, windows=None, min_energy=1e-3):
        """Pairs ranked by the normalised cross-correlation (asx_xcorr_ncc_f32_dev): the Pearson coefficient of every lag 0..N-1.
        source: float32 [2N] or [B, 2N]; sample: [N] or [B, N]; a 1-D operand serves every pair.  windows: None (every lag 0..N-1),
        or integers [2] / [B, 2] rows inside [0, N-1].  min_energy: the share of the loudest window's energy below which a lag does
        not compete.  Arguments are checked on the host (ValueError) before anything is uploaded.  Returns (lag int64[B], coef
        float64[B], peak float64[B], ret int32[B]): peak is |c32[lag]|, coef the reference's coefficient of the samples there."""
        s, t, w, batch, ss, ts, ws, me = ncc_args(self.sample_len, source, sample, windows, min_energy)
        return self._staged((s, t, w), (batch,), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_ncc_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, me, *d_out))

    def xcorr_ncc_topk_f32(self, source, sample, k, min_separation, windows=None, min_energy=1e-3):
        """The k strongest separated lags per pair of the coefficient curve (asx_xcorr_ncc_topk_f32_dev): source, sample, windows and
        min_energy as in xcorr_ncc_f32, k and min_separation as in xcorr_topk_f32.  Arguments are checked on the host (ValueError)
        before anything is uploaded.  Returns (lag int64[B, k], coef float64[B, k], peak float64[B, k], ret int32[B, k]); ret = -3 (and
        NaN for coef and peak) where no lag was left.  Entry 0 is xcorr_ncc_f32's result."""
        s, t, w, batch, ss, ts, ws, me, k, sep = ncc_topk_args(self.sample_len, source, sample, k, min_separation, windows, min_energy)
        return self._staged((s, t, w), (batch, k), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_ncc_topk_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, me, k, sep, *d_out))

    def xcorr_ncc_full_f32(self, source, sample, windows=None, min_energy=1e-3, min_overlap=None):
        """Pairs ranked by the full-range normalised cross-correlation (asx_xcorr_ncc_full_f32_dev): the Pearson coefficient of every
        lag -(N-1)..N-1.  source, sample and min_energy as in xcorr_ncc_f32; windows: None (every lag), or integers [2] / [B, 2] rows
        inside [-(N-1), N-1]; min_overlap: the fewest frames a negative lag must overlap in to compete, 1..N (None: (N + 1) // 2).
        Arguments are checked on the host (ValueError) before anything is uploaded.  Returns (lag, coef, peak, ret) as xcorr_ncc_f32."""
        s, t, w, batch, ss, ts, ws, me, mo = ncc_full_args(self.sample_len, source, sample, windows, min_energy, min_overlap)
        return self._staged((s, t, w), (batch,), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_ncc_full_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, me, mo, *d_out))

    def xcorr_ncc_full_topk_f32(self, source, sample, k, min_separation, windows=None, min_energy=1e-3, min_overlap=None):
        """The k strongest separated lags per pair of the full-range curve (asx_xcorr_ncc_full_topk_f32_dev): the arguments of
        xcorr_ncc_full_f32, k and min_separation as in xcorr_topk_f32.  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag, coef, peak, ret) of shape [B, k]; ret = -3 (and NaN for coef and peak) where no lag was
        left.  Entry 0 is xcorr_ncc_full_f32's result."""
        s, t, w, batch, ss, ts, ws, me, mo, k, sep = ncc_full_topk_args(self.sample_len, source, sample, k, min_separation, windows,
                                                                        min_energy, min_overlap)
        return self._staged((s, t, w), (batch, k), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_ncc_full_topk_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, me, mo, k, sep, *d_out))

    def xcorr_ncc_ragged_f32(self, source, sample, lengths=None, windows=None, min_energy=1e-3, min_overlap=None):
        """Pairs of tracks of differing lengths ranked by the normalised cross-correlation over what they really share
        (asx_xcorr_ncc_ragged_f32_dev).  source, sample, windows, min_energy and min_overlap as in xcorr_ncc_full_f32 (ragged_pack
        pads tracks to the plan's shape); lengths: None (every pair (2N, N)), or integers [2] / [B, 2] rows (Ls, Lm) -- frames at and
        beyond them are ignored whatever they hold.  Arguments are checked on the host (ValueError) before anything is uploaded.
        Returns (lag, coef, peak, ret) as xcorr_ncc_f32; ret = -5 for a row outside 1 <= Ls <= 2N, 1 <= Lm <= N."""
        s, t, v, w, batch, ss, ts, vs, ws, me, mo = ncc_ragged_args(self.sample_len, source, sample, lengths, windows, min_energy,
                                                                    min_overlap)
        return self._staged((s, t, v, w), (batch,), _PHAT_RESULTS, lambda d_s, d_t, d_v, d_w, *d_out: self.xcorr_ncc_ragged_dev(
            d_s, ss, d_t, ts, d_v, vs, d_w, ws, batch, me, mo, *d_out))

    def xcorr_ncc_ragged_topk_f32(self, source, sample, k, min_separation, lengths=None, windows=None, min_energy=1e-3,
                                  min_overlap=None):
        """The k strongest separated lags per pair of the ragged curve (asx_xcorr_ncc_ragged_topk_f32_dev): the arguments of
        xcorr_ncc_ragged_f32, k and min_separation as in xcorr_topk_f32.  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag, coef, peak, ret) of shape [B, k]; ret = -3 (and NaN for coef and peak) where no lag was
        left, -5 in all k entries for a row that is no pair of lengths.  Entry 0 is xcorr_ncc_ragged_f32's result."""
        s, t, v, w, batch, ss, ts, vs, ws, me, mo, k, sep = ncc_ragged_topk_args(self.sample_len, source, sample, k, min_separation,
                                                                                 lengths, windows, min_energy, min_overlap)
        return self._staged((s, t, v, w), (batch, k), _PHAT_RESULTS, lambda d_s, d_t, d_v, d_w, *d_out: self.xcorr_ncc_ragged_topk_dev(
            d_s, ss, d_t, ts, d_v, vs, d_w, ws, batch, me, mo, k, sep, *d_out))

    def xcorr_pool_ncc_f32(self, sources, samples, pairs=None, windows=None, min_energy=1e-3):
        """Pairs of two pools ranked by the normalised cross-correlation (asx_xcorr_pool_ncc_f32_dev): the pools and pairs of
        xcorr_pool_f32, windows and min_energy of xcorr_ncc_f32.  Every track is transformed, and its moments are formed, once per
        call.  Arguments are checked on the host (ValueError) before anything is uploaded.  Returns (lag int64, coef float64, peak
        float64, ret int32) of shape [B], or [S, R] when pairs is None; a pair with an index outside its pool gets (0, NaN, NaN, -4)."""
        n = self.sample_len
        s, t, pr, w, batch, ws, me = pool_ncc_args(n, sources, samples, pairs, windows, min_energy)
        shape = (batch,) if pr is not None else (s.shape[0], t.shape[0])
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_ncc_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, me, *d_out))

    def xcorr_pool_ncc_topk_f32(self, sources, samples, k, min_separation, pairs=None, windows=None, min_energy=1e-3):
        """The k strongest separated lags of the coefficient curve per pair of two pools (asx_xcorr_pool_ncc_topk_f32_dev): the
        arguments of xcorr_pool_ncc_f32, k and min_separation of xcorr_topk_f32.  Returns (lag, coef, peak, ret) of shape [B, k], or
        [S, R, k] when pairs is None; ret = -3 where no lag was left, -4 in all k entries of a pair with an index outside its pool."""
        n = self.sample_len
        s, t, pr, w, batch, ws, me, k, sep = pool_ncc_topk_args(n, sources, samples, k, min_separation, pairs, windows, min_energy)
        shape = ((batch,) if pr is not None else (s.shape[0], t.shape[0])) + (k,)
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_ncc_topk_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, me, k, sep, *d_out))

    def xcorr_pool_ncc_full_f32(self, sources, samples, pairs=None, windows=None, min_energy=1e-3, min_overlap=None):
        """Pairs of two pools ranked by the full-range normalised cross-correlation (asx_xcorr_pool_ncc_full_f32_dev): the pools and
        pairs of xcorr_pool_f32, windows (rows inside [-(N-1), N-1]), min_energy and min_overlap of xcorr_ncc_full_f32.  Every
        track's transforms, moments and tables are formed once per call.  Arguments are checked on the host (ValueError) before
        anything is uploaded.  Returns (lag, coef, peak, ret) of shape [B], or [S, R] when pairs is None; a pair with an index
        outside its pool gets (0, NaN, NaN, -4)."""
        n = self.sample_len
        s, t, pr, w, batch, ws, me, mo = pool_ncc_full_args(n, sources, samples, pairs, windows, min_energy, min_overlap)
        shape = (batch,) if pr is not None else (s.shape[0], t.shape[0])
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_ncc_full_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, me, mo, *d_out))

    def xcorr_pool_ncc_full_topk_f32(self, sources, samples, k, min_separation, pairs=None, windows=None, min_energy=1e-3,
                                     min_overlap=None):
        """The k strongest separated lags of the full-range curve per pair of two pools (asx_xcorr_pool_ncc_full_topk_f32_dev): the
        arguments of xcorr_pool_ncc_full_f32, k and min_separation of xcorr_topk_f32.  Returns (lag, coef, peak, ret) of shape
        [B, k], or [S, R, k] when pairs is None -- with one recording as both pools, the tables pool_closure takes; ret = -3 where no
        lag was left, -4 in all k entries of a pair with an index outside its pool."""
        n = self.sample_len
        s, t, pr, w, batch, ws, me, mo, k, sep = pool_ncc_full_topk_args(n, sources, samples, k, min_separation, pairs, windows,
                                                                         min_energy, min_overlap)
        shape = ((batch,) if pr is not None else (s.shape[0], t.shape[0])) + (k,)
        return self._staged((s, t, pr, w), shape, _PHAT_RESULTS, lambda d_s, d_t, d_pr, d_w, *d_out: self.xcorr_pool_ncc_full_topk_dev(
            d_s, 2 * n, s.shape[0], d_t, n, t.shape[0], d_pr, d_w, ws, batch, me, mo, k, sep, *d_out))

    def xcorr_phat_band_f32(self, source, sample, bin_lo, bin_hi, windows=None):
        """xcorr_phat_f32 in which only bins bin_lo..bin_hi of the 2N-point transform vote (asx_xcorr_phat_band_f32_dev; band_bins
        converts from Hz).  peak is |r_phat[lag]| / V, V the number of bins that vote.  The full band (0, N) is xcorr_phat_f32."""
        return self.xcorr_phat_f32(source, sample, windows, band=(int(bin_lo), int(bin_hi)))

    def xcorr_phat_f32(self, source, sample, windows=None, band=None):
        """Pairs ranked by the GCC-PHAT curve (asx_xcorr_phat_f32_dev).  source: float32 [2N] or [B, 2N]; sample: [N] or [B, N]; a
        1-D operand serves every pair.  windows: None (the plan's window), or integers [2] / [B, 2] as in xcorr_windowed_f32.
        Returns (lag int64[B], coef float64[B], peak float64[B], ret int32[B]): the float32 argmax of r_phat, the reference's
        Pearson coefficient of the samples at that lag, and the peak height |r_phat[lag]| / F in [0, 1].  band: xcorr_phat_band_f32's."""
        s, t, w, batch, ss, ts, ws = _strided_args(self.sample_len, source, sample, None if windows is None else _window_rows(windows))
        if band is None:
            return self._staged((s, t, w), (batch,), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_phat_dev(
                d_s, ss, d_t, ts, d_w, ws, batch, *d_out))
        return self._staged((s, t, w), (batch,), _PHAT_RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_phat_band_dev(
            d_s, ss, d_t, ts, d_w, ws, batch, band[0], band[1], *d_out))

    def _strided_f32(self, src, src_stride, smp, smp_stride, batch, windows=None, window_stride=0):
        """checked host float32 buffers -> asx_xcorr_strided_f32_dev (with int64 window rows: asx_xcorr_windowed_f32_dev) ->
        (lag, coef, ret) of [batch]"""
        if windows is None:
            return self._staged((src, smp), (batch,), _RESULTS, lambda d_s, d_t, *d_out: self.xcorr_strided_dev(
                d_s, src_stride, d_t, smp_stride, batch, *d_out))
        return self._staged((src, smp, windows), (batch,), _RESULTS, lambda d_s, d_t, d_w, *d_out: self.xcorr_windowed_dev(
            d_s, src_stride, d_t, smp_stride, d_w, window_stride, batch, *d_out))

    def xcorr_broadcast_f32(self, source, sample):
        """One track against many.  source: float32 [2N] (one source for every pair) or [B, 2N]; sample: [N] (one sample for every
        pair) or [B, N].  At least one may be 1-D; with both 1-D there is one pair.  The 1-D track is transformed once per call
        (real-column plans).  Returns (lag int64[B], coef float64[B], ret int32[B]) like xcorr_batch_f32."""
        s, t, ss, ts = _operands(self.sample_len, source, sample)
        return self._strided_f32(s, ss, t, ts, _shared_batch(s, t))

    def xcorr_windowed_f32(self, source, sample, windows):
        """Pairs with a lag window each (asx_xcorr_windowed_f32_dev).  source: float32 [2N] or [B, 2N]; sample: [N] or [B, N];
        windows: integers [2] (one window for every pair) or [B, 2], rows (lag_min, lag_max).  A 1-D operand serves every pair; all
        1-D is one pair.  Shapes are checked on the host (ValueError) before anything is uploaded; a row that is not a window
        inside [-N, N-1] gives that pair (0, NaN, -2).  The plan's own window is not used.  Returns (lag, coef, ret) like
        xcorr_batch_f32."""
        s, t, w, batch, ss, ts, ws = windowed_args(self.sample_len, source, sample, windows)
        return self._strided_f32(s, ss, t, ts, batch, w, ws)

    def xcorr_windows_f32(self, recording, sample, hop, positions=None):
        """Windows recording[k*hop : k*hop + 2N] (k = 0 .. (len - 2N) // hop) of one long float32 recording, each correlated with
        the one float32 sample [N]: one (lag, coef, ret) per window, arrays like xcorr_batch_f32's.  The recording and the sample
        are uploaded once and the sample is transformed once.  Which window holds the sample is the caller's decision (for
        instance the largest |coef| with ret == 0); a clip that straddles two windows shows in both with lower coefficients, so a
        hop of at most N keeps every clip of length N whole in some window.  On real-column plans hop must be a multiple of 4.
        positions=(p_lo, p_hi): the sample is known to start between recording frames p_lo and p_hi.  Window k then searches only
        lags [p_lo - k*hop, p_hi - k*hop] clipped to [-N, N-1] (position_rows), in one asx_xcorr_windowed_f32_dev call over the
        windows where that is not empty; the others are not correlated and come back (0, NaN, -2).  A window's lag l is the start
        frame k*hop + l.  positions=None: every lag of every window, the plan's own window applies."""
        n = self.sample_len
        r = np.ascontiguousarray(recording, dtype=np.float32).ravel()
        t = np.ascontiguousarray(sample, dtype=np.float32).ravel()
        hop = int(hop)
        if t.size != n:
            raise ValueError("sample must have N = %d frames" % n)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        if r.size < 2 * n:
            raise ValueError("recording shorter than one window of 2N = %d frames" % (2 * n))
        batch = (r.size - 2 * n) // hop + 1
        if positions is None:
            return self._strided_f32(r, hop, t, 0, batch)
        p_lo, p_hi = (int(v) for v in positions)
        k0, k1, rows = position_rows(n, hop, batch, p_lo, p_hi)
        lag = np.zeros(batch, dtype=np.int64)
        coef = np.full(batch, np.nan, dtype=np.float64)
        ret = np.full(batch, -2, dtype=np.int32)
        if k1 > k0:
            part = self._strided_f32(np.ascontiguousarray(r[k0 * hop:(k1 - 1) * hop + 2 * n]), hop, t, 0, k1 - k0, rows, 1)
            for whole, got in zip((lag, coef, ret), part):
                whole[k0:k1] = got
        return lag, coef, ret

    def debug_r_dev(self, d_src, d_smp, d_r, d_lag, d_coef, d_ret, stream=0):
        _check(lib().asx_xcorr_debug_r_dev(self._h, d_src, d_smp, d_r, d_lag, d_coef, d_ret, stream or None))

    def set_profiling(self, depth):
        """depth > 0: keep the kernel events of the last `depth` batch calls; 0 / False: off"""
        lib().asx_plan_set_profiling(self._h, int(depth))

    def last_timings_ms(self, calls_back=0):
        out = (ctypes.c_float * 6)()
        _check(lib().asx_plan_timings_ms(self._h, int(calls_back), out))
        return dict(zip(("fwd_cols", "rows", "inv_cols", "finalize", "pearson", "total"), list(out)))

    def sync(self, stream=0):
        _check(lib().asx_stream_sync(self._h, stream or None))
