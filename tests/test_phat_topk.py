"""Top-k GCC-PHAT (asx_xcorr_phat_topk_f32_dev, asx_xcorr_pool_phat_topk_f32_dev), the parts that need no GPU: the float64 model of
tests/phat_topk_model.py on the multipath pair -- the five planted lags in order, and the gaps that the GPU comparison rests on --
the model's zones and seeds against a plain loop, the binding's host checks, the prototypes, and what the header says."""
import ctypes
import os
import re

import numpy as np
import pytest

import phat_band_model
import phat_topk_model
import topk_model
from util import ROOT, asx, graft

N = 144000
SEEDS = (1, 2, 3)
SEP = 64
NEW = ("asx_xcorr_phat_topk_f32_dev", "asx_xcorr_pool_phat_topk_f32_dev")
# the smallest gap between an entry and the best lag its pass left that the GPU tests rely on: thousands of times the float32
# resolution of r_phat / V (2.2e-8 at this length, include/audiosync/xcorr_hip.h)
MIN_GAP = 1e-4

_cache = {}


def multipath(seed, band):
    """the multipath pair of `seed` under band (bin_lo, bin_hi): (source, sample, r_phat / V, the model's five entries, their
    margins, the sixth candidate's height); computed once"""
    if (seed, band) not in _cache:
        src, smp = phat_topk_model.multipath_pair(seed, N)
        r = phat_band_model.r_phat_band(src, smp, *band)
        six = phat_topk_model.model(src, smp, *band, 6, SEP, r=r)
        _cache[seed, band] = (src, smp, r, six[:5], phat_topk_model.margins(r, N, six[:5], SEP), six[5][3])
    return _cache[seed, band]


@pytest.mark.parametrize("band", [(0, N), (1, N // 6)])
@pytest.mark.parametrize("seed", SEEDS)
def test_the_model_returns_the_planted_paths_in_order(seed, band):
    """the five planted lags by falling gain, every entry at least MIN_GAP above the best lag its pass left, and so above the next
    entry and above the sixth candidate: the precondition of the GPU comparison, checked and not assumed"""
    _, _, r, five, gaps, sixth = multipath(seed, band)
    print("phat top-k multipath seed", seed, "band", band, "heights", [round(e[3], 4) for e in five], "margins", gaps, "sixth", sixth)
    assert [e[1] for e in five] == list(phat_topk_model.MULTIPATH_LAGS), five
    assert all(e[0] == 0 and abs(e[2]) < 1.0 for e in five), five
    heights = [e[3] for e in five]
    assert all(a - b >= MIN_GAP for a, b in zip(heights, heights[1:] + [sixth])), (heights, sixth)
    assert min(gaps) >= MIN_GAP, gaps
    assert heights[4] > 2 * sixth, (heights, sixth)


def test_the_model_is_the_plain_loop_on_a_small_curve():
    """zones by linear lag distance, the signed seed and exhaustion: topk_model's vector form, which the model runs on r_phat,
    against the rule written out lag by lag"""
    rng = np.random.default_rng(5)
    n = 24
    for trial in range(40):
        r = rng.standard_normal(2 * n)
        lo = int(rng.integers(-n, n))
        hi = int(rng.integers(lo, n))
        sep = int(rng.integers(0, 9))
        r[lo % (2 * n)] = -5.0            # a large negative seed: it competes signed, so any positive value beats it
        assert topk_model.topk_peaks(r, n, 6, sep, lo, hi) == topk_model.brute_peaks(r, n, 6, sep, lo, hi), (trial, lo, hi, sep)


def test_an_exhausted_window_and_a_silent_pair_in_the_model():
    src, smp = phat_topk_model.multipath_pair(1, 64)
    out = phat_topk_model.model(src, smp, 0, 64, 4, 3, lo=-2, hi=8)        # 11 lags, zones of 7: exhausted part-way
    rets = [e[0] for e in out]
    first = rets.index(-3)                 # zones of 7 lags: two entries can use the window up, three always do
    assert 2 <= first <= 3 and rets[first:] == [-3] * (4 - first), out
    assert all(e[1] == 0 and np.isnan(e[2]) and np.isnan(e[3]) for e in out if e[0] == -3), out
    quiet = phat_topk_model.model(src, np.zeros(64, np.float32), 0, 64, 3, 5, lo=10, hi=40)
    assert [(e[0], e[1], e[3]) for e in quiet] == [(-1, 10, 0.0), (-1, 16, 0.0), (-1, 22, 0.0)], quiet   # the successive seeds


def test_the_models_alone_place_the_clips_of_the_end_to_end_test():
    """the premise of tests/test_gpu_pool_phat_topk.py's end-to-end test, from this model into tests/closure_model.py: with the pinned
    seed every pair's first entry is the planted lag, an echo decoy is among the others, and closure places the four clips at the
    planted offsets.  Seeds 20270, 20271 and 20272 were looked at; all three do, and the planted entry stands at least 0.09 above
    the pair's second entry in each."""
    import closure_model
    clips = phat_topk_model.e2e_clips()
    lag, coef, peak, ret = phat_topk_model.e2e_tables(clips)
    assert (peak[:, :, 0] - peak[:, :, 1]).min() > 0.05, peak
    out = closure_model.closure(lag, coef, ret, phat_topk_model.E2E_TOL, 1)
    phat_topk_model.check_e2e(lag, ret, out)
    assert out["root"] == 0 and out["offset"].tolist() == list(phat_topk_model.E2E_OFFSETS)
    assert (out["confirm"][~np.eye(4, dtype=bool)] == 3).all()


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    m = asx()
    from audiosync_amd import hipxcorr
    L = ctypes.CDLL(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hipxcorr.ABI_SYMBOLS and name in hipxcorr.SIGNATURES, name
        assert hasattr(L, name), name
    assert m.abi_version() == 2 and m.lib().asx_abi_version() == 2
    for name in ("xcorr_phat_topk_dev", "xcorr_pool_phat_topk_dev", "xcorr_phat_topk_f32", "xcorr_pool_phat_topk_f32"):
        assert callable(getattr(m.Plan, name)), name
    assert callable(m.phat_topk_args) and callable(m.pool_phat_topk_args)


def test_the_binding_and_the_header_prototypes_agree():
    """parameter for parameter: the signature table against the header, and the header against the definitions"""
    from test_binding_signatures import c_kind, csrc_definitions, ctypes_kind, header_prototypes
    asx()
    from audiosync_amd import hipxcorr
    header, defs = header_prototypes(), csrc_definitions()
    for name in NEW:
        ret, params = header[name]
        restype, argtypes = hipxcorr.SIGNATURES[name]
        assert ctypes_kind(restype) == c_kind(ret, True) == ctypes.c_int, name
        assert [ctypes_kind(t) for t in argtypes] == [c_kind(p) for p in params] == [c_kind(p) for p in defs[name][1]], name
    # the band, k and min_separation sit between batch and the outputs, in this order
    strided = [p.split()[-1].lstrip("*") for p in header[NEW[0]][1]]
    assert strided[7:12] == ["batch", "bin_lo", "bin_hi", "k", "min_separation"] and strided[12:] == ["d_lag", "d_coef", "d_peak", "d_ret", "stream"]
    pool = [p.split()[-1].lstrip("*") for p in header[NEW[1]][1]]
    assert pool[10:15] == ["batch", "bin_lo", "bin_hi", "k", "min_separation"] and pool[15:] == strided[12:]


def test_the_header_and_the_documents_offer_top_k_with_phat():
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    flat = re.sub(r"[\s*]+", " ", hdr)
    for text in ("Not offered with PHAT: top-k", "Not offered: top-k with PHAT"):
        assert text not in flat, text
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert "so that they can take it later" not in design and "a band per pair, top-k, streams" not in design
    at = flat.index("Top-k GCC-PHAT:")
    text = flat[at:flat.index("int asx_xcorr_phat_topk_f32_dev", at)]
    for phrase in ("i k + j of d_lag, d_coef, d_peak and d_ret", "d_lag and d_peak may be NULL", "linear lag distance", "SIGNED",
                   "(0, NaN, peak NaN, -3)", "(0, NaN, NaN, -2)", "ret is never 1", "k = 1 launches exactly that call",
                   "never synchronises the host", "asx_plan_workspace_bytes does not change", "capturable",
                   "min_separation < 0", "batch == 0 returns 0", "no pass does any exact re-evaluation", "a band per pair"):
        assert re.sub(r"[\s*]+", " ", phrase) in text, phrase
    at = flat.index("Top-k GCC-PHAT over two track pools")
    text = flat[at:flat.index("int asx_xcorr_pool_phat_topk_f32_dev", at)]
    for phrase in ("(0, NaN, NaN, -4)", "over -2 and -3", "bit for bit", "filled ONCE per call", "asx_pool_closure_dev"):
        assert phrase in text, phrase
    top = flat[:flat.index("#ifndef AUDIOSYNC_XCORR_HIP_H")]
    minus3 = top[top.index("ret = -3"):top.index("ret = -4")]
    minus4 = top[top.index("ret = -4"):top.index("ret = -5")]
    assert all(name in minus3 for name in NEW) and NEW[1] in minus4 and NEW[0] not in minus4
    for path in ("README.md", "INTEGRATION.md", os.path.join("tools", "README.md")):
        assert "phat_topk" in open(os.path.join(ROOT, path)).read(), path


def test_host_checks_return_the_checked_arguments():
    asx()
    from audiosync_amd.hipxcorr import TOPK_MAX, phat_topk_args, pool_phat_topk_args
    n = 16
    src, smp = np.zeros((3, 2 * n), np.float32), np.zeros(n, np.float64)
    s, t, w, batch, ss, ts, ws, lo, hi, k, sep = phat_topk_args(n, src, smp, np.int64(TOPK_MAX), 0)
    assert w is None and (batch, ss, ts, ws, lo, hi, k, sep) == (3, 2 * n, 0, 0, 0, n, TOPK_MAX, 0) and s.dtype == t.dtype == np.float32
    assert all(type(v) is int for v in (lo, hi, k, sep))
    out = phat_topk_args(n, src[0], np.zeros((2, n)), 2, 5, [[-3, 3], [0, 0]], (np.int64(2), 5))
    assert out[2].tolist() == [[-3, 3], [0, 0]] and out[3:] == (2, 0, n, 1, 2, 5, 2, 5)
    src3, smp2 = np.zeros((3, 2 * n), np.float32), np.zeros((2, n), np.float64)
    s, t, p, w, batch, ws, lo, hi, k, sep = pool_phat_topk_args(n, src3, smp2, 3, 7)
    assert p is None and w is None and (batch, ws, lo, hi, k, sep) == (6, 0, 0, n, 3, 7)
    out = pool_phat_topk_args(n, src3, smp2, 2, 5, [[0, 1], [7, -1]], (-3, 3), (2, 5))
    assert out[2].tolist() == [[0, 1], [7, -1]] and out[3].tolist() == [-3, 3] and out[4:] == (2, 0, 2, 5, 2, 5)


class NoDevice:
    """a stand-in plan: touching the device, or reaching a _dev call, is the failure"""
    sample_len = 16

    @property
    def device(self):
        raise AssertionError("uploaded")

    def __getattr__(self, name):
        raise AssertionError("reached %s" % name)


BAD_OPTIONS = [dict(k=0), dict(k=9), dict(k=2.0), dict(k=True), dict(min_separation=-1), dict(min_separation=1.0),
               dict(min_separation=False), dict(band=(5, 4)), dict(band=(-1, 3)), dict(band=(0, 17)), dict(band=(0.0, 4)),
               dict(band=(True, 4)), dict(windows=(1.5, 2)), dict(windows=(0, 1, 2))]


def test_the_strided_form_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(source=np.zeros((2, 32), np.float32), sample=np.zeros((2, 16), np.float32), k=2, min_separation=10)
    bad = BAD_OPTIONS + [dict(source=np.zeros(31, np.float32)), dict(sample=np.zeros((2, 15), np.float32)),
                         dict(sample=np.zeros((3, 16), np.float32)), dict(windows=[[0, 1]] * 3)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_phat_topk_f32(NoDevice(), **args)


def test_the_pool_form_checks_before_it_uploads():
    asx()
    from audiosync_amd import hipxcorr
    good = dict(sources=np.zeros((2, 32), np.float32), samples=np.zeros((2, 16), np.float32), k=2, min_separation=10)
    bad = BAD_OPTIONS + [dict(sources=np.zeros(32, np.float32)), dict(samples=np.zeros((2, 15), np.float32)),
                         dict(sources=np.zeros((0, 32), np.float32)), dict(pairs=[[0, 1, 2]]), dict(pairs=[[0.0, 0.0]]),
                         dict(pairs=[[2 ** 31, 0]]), dict(pairs=np.zeros((0, 2), np.int32)), dict(windows=[[0, 1]] * 3),
                         dict(pairs=[[0, 1]] * 3, windows=[[0, 1]] * 2)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            hipxcorr.Plan.xcorr_pool_phat_topk_f32(NoDevice(), **args)


def test_the_new_kernels_meet_the_budgets():
    """the PHAT tail's top-k instance, the peak writer in front of the step and the k-entry writer for pairs outside their pools:
    one instance each, plain kernels without LDS or scratch"""
    from test_kernel_resources import READELF, demangled, kernels_of
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf in this image")
    asx()
    kernels = {demangled(k): v for k, v in kernels_of(os.path.join(graft.PKG_DIR, "libaudiosync_hip.so")).items()}
    found = {}
    for k, r in kernels.items():
        m = re.match(r"(?:void )?(k_phat_finalize_x|k_topk_peak|k_invalid_pairs_kp)(?![A-Za-z0-9_])", k)
        if m:
            found.setdefault(m.group(1), []).append((k, r))
    assert {k: len(v) for k, v in found.items()} == {"k_phat_finalize_x": 1, "k_topk_peak": 1, "k_invalid_pairs_kp": 1}, found
    assert len([k for k in kernels if k.startswith("void k_phat_finalize<")]) == 2   # the one-entry call's instances, as they were
    for ks in found.values():
        for k, r in ks:
            assert r["vgpr_count"] <= 64 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
