"""Fixture F of the full-range NCC pool calls (asx_xcorr_pool_ncc_full_topk_f32_dev) and the float64 model tables an all-pairs call
over it has to return: four clips of one recording at known offsets, two loud private events (a burst that two clips share at a
false lag) and a private level step per clip.  The raw top-k tables lose every true lag to the level step, the NCC tables of the lags
0..N-1 have no entry where the true lag is negative, the full-range NCC tables hold every true lag -- behind a decoy in three pairs,
which triangle closure (tests/closure_model.py) sorts out.  Plain module: no fixtures, nothing happens on import; the tables are
built once per process."""
import functools

import numpy as np

import closure_model
import ncc_full_model as fm
import ncc_model
import ncc_topk_model
import topk_model

N = 144000
C = 4
K = 3
SEP = 1000
TOL = 2
OFFSETS = (0, 20000, 45000, 70000)
BURST = 30000
# (a, b): (pa, pb) -- the burst sits at frame pa of clip a and at frame pb of clip b: in pair (a, b) it lines up at lag pa - pb
EVENTS = (((0, 1), (150000, 100000)), ((3, 0), (40000, 100000)))
# the pairs whose entry 0 is the burst's decoy: pair -> decoy lag (pair (0, 3) sees the event of (3, 0) from the other side)
DECOYS = {(0, 1): 50000, (0, 3): 60000, (3, 0): -60000}


@functools.lru_cache(maxsize=None)
def clips():
    """-> float32 [C, 2N], read-only; pair (a, b) is clips[a] against clips[b, :N]"""
    rng = np.random.default_rng(20262)
    rec = rng.standard_normal(OFFSETS[-1] + 2 * N).astype(np.float32)
    out = np.stack([rec[o:o + 2 * N].copy() for o in OFFSETS])
    for (a, b), (pa, pb) in EVENTS:
        burst = (3.0 * rng.standard_normal(BURST)).astype(np.float32)
        out[a, pa:pa + BURST] += burst
        out[b, pb:pb + BURST] += burst
    out += np.float32(0.5)
    for a in range(C):
        out[a, int(1.2 * N) + 1000 * a:] += np.float32(4.0)
    out.setflags(write=False)
    return out


def true_lags():
    """-> int64 [C, C]: o_b - o_a"""
    o = np.array(OFFSETS, dtype=np.int64)
    return o[None, :] - o[:, None]


def pools():
    """-> (sources [C, 2N], samples [C, N]) as the staged calls take them"""
    x = clips()
    return x, np.ascontiguousarray(x[:, :N])


def _tables(entries):
    """entries(a, b) -> K tuples (ret, lag, coef, peak) => dict of [C, C, K] arrays"""
    lag = np.zeros((C, C, K), dtype=np.int64)
    coef = np.zeros((C, C, K), dtype=np.float64)
    peak = np.zeros((C, C, K), dtype=np.float64)
    ret = np.zeros((C, C, K), dtype=np.int32)
    for a in range(C):
        for b in range(C):
            for j, (r, l, c, p) in enumerate(entries(a, b)):
                ret[a, b, j], lag[a, b, j], coef[a, b, j], peak[a, b, j] = r, l, c, p
    out = {"lag": lag, "coef": coef, "peak": peak, "ret": ret}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def curves():
    """{(a, b): ncc_full_model.curve of the pair}, each computed once"""
    srcs, smps = pools()
    return {(a, b): fm.curve(srcs[a], smps[b]) for a in range(C) for b in range(C)}


@functools.lru_cache(maxsize=None)
def full_tables():
    """the [C, C, K] tables of ncc_full_model.topk: what asx_xcorr_pool_ncc_full_topk_f32_dev returns for fixture F"""
    srcs, smps = pools()
    cv = curves()
    return _tables(lambda a, b: fm.topk(srcs[a], smps[b], K, SEP, cv=cv[(a, b)]))


@functools.lru_cache(maxsize=None)
def half_tables():
    """the tables of the NCC model of the lags 0..N-1 (ncc_topk_model.topk), the coefficient being the reference's at the entry's lag"""
    srcs, smps = pools()

    def entries(a, b):
        c, vx, vy = ncc_model.curve(srcs[a], smps[b])
        out = []
        for status, lag, peak in ncc_topk_model.topk(c, vx, vy, K, SEP):
            coef = fm.coefficient(srcs[a], smps[b], lag) if status == 0 else float("nan")
            out.append((status if status else (-1 if coef != coef else 0), lag, coef, peak))
        return out
    return _tables(entries)


@functools.lru_cache(maxsize=None)
def raw_tables():
    """the tables of the raw top-k rule over r (topk_model.model); peak: unused, 0"""
    srcs, smps = pools()
    return _tables(lambda a, b: [e + (0.0,) for e in topk_model.model(srcs[a], smps[b], K, SEP)])


def close(t):
    """closure_model.closure over one set of tables, with fixture F's tolerance"""
    return closure_model.closure(t["lag"], t["coef"], t["ret"], TOL)


def right_picks(closed):
    """how many of the C * C picked lags are the true ones"""
    return int((closed["best_lag"] == true_lags()).sum())


def check_premise(t):
    """What "the full-range tables carry every true lag" means, asserted on a set of [C, C, K] tables (the model's or the device's):
    entry 0 is the decoy in the three pairs of DECOYS, with a peak at least 0.1 above the true entry's, and the true lag everywhere
    else; every true entry's peak is at least 0.15; every other entry is noise, at most 0.03."""
    want = true_lags()
    for a in range(C):
        for b in range(C):
            lag, peak, ret = t["lag"][a, b], t["peak"][a, b], t["ret"][a, b]
            assert ret.tolist() == [0] * K, (a, b, ret)
            at = [j for j in range(K) if lag[j] == want[a, b]]
            assert len(at) == 1, (a, b, lag, want[a, b])
            true_at = at[0]
            if a == b:
                assert true_at == 0 and peak[0] > 0.99, (a, b, peak)
                rest = [j for j in range(1, K)]
            elif (a, b) in DECOYS:
                assert lag[0] == DECOYS[(a, b)] and true_at == 1, (a, b, lag)
                assert peak[0] - peak[1] >= 0.1, (a, b, peak)
                rest = [2]
            else:
                assert true_at == 0, (a, b, lag)
                rest = [1, 2]
            assert peak[true_at] >= 0.15, (a, b, peak)
            assert all(peak[j] <= 0.03 for j in rest), (a, b, peak)
