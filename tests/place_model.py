"""numpy model of asx_pool_place_dev (include/audiosync/xcorr_hip.h): the rule in int64 arithmetic (|offset| < 2^52 by the header's
bound, so nothing wraps), layer by layer and sweep by sweep as the header states it, vectorised over the clips a layer can reach.
place(L, R, F, root, ...) takes closure's picked tables (best_lag, best_ret, confirm, [C, C]) and returns every output of the call
as the device must produce it, bit for bit.  band(...) builds the tables of a long event: clips about `spacing` apart, the true lag
only between clips closer than `reach`, garbage or nothing between the others."""
import numpy as np

LAG_MAX = 1 << 40       # ASX_CLOSURE_LAG_MAX
HOPS_MAX = 1024         # ASX_PLACE_HOPS_MAX
SWEEPS_MAX = 64         # ASX_PLACE_SWEEPS_MAX
OUTPUTS = (("offset", np.int64), ("hops", np.int32), ("support", np.int32), ("degree", np.int32), ("step", np.int64),
           ("resid", np.int64), ("state", np.int32))
GARBAGE = 100000        # band(): decoys and out-of-band lags are uniform in [-GARBAGE, GARBAGE)


def usable_pairs(L, R, F, min_confirm):
    """-> bool [C, C]: closure's usable(x, y)"""
    C = L.shape[0]
    return (R == 0) & (L >= -LAG_MAX) & (L <= LAG_MAX) & (F >= min_confirm) & ~np.eye(C, dtype=bool)


def lower_median(values):
    """the element at index (n - 1) // 2 of the sorted multiset"""
    v = np.sort(np.asarray(values, dtype=np.int64))
    return int(v[(len(v) - 1) // 2])


def estimates(L, U, o, among, b):
    """E_b over the clips of the mask `among`: o[c] + L_cb where (c, b) is usable, o[c] - L_bc where (b, c) is"""
    fwd, bwd = among & U[:, b], among & U[b, :]
    return np.concatenate([o[fwd] + L[fwd, b], o[bwd] - L[b, bwd]])


def place(L, R, F, root, tolerance, min_confirm=1, max_hops=64, sweeps=0):
    """every output of asx_pool_place_dev as a dict of arrays"""
    L = np.ascontiguousarray(L, dtype=np.int64)
    R = np.ascontiguousarray(R, dtype=np.int32)
    F = np.ascontiguousarray(F, dtype=np.int32)
    C = L.shape[0]
    assert L.shape == R.shape == F.shape == (C, C) and C >= 1
    assert 0 <= tolerance <= LAG_MAX and min_confirm >= 0 and 1 <= max_hops <= HOPS_MAX and 0 <= sweeps <= SWEEPS_MAX
    U = usable_pairs(L, R, F, min_confirm)
    linked = U | U.T
    o = np.zeros(C, dtype=np.int64)
    hops = np.full(C, -1, dtype=np.int32)
    step = np.zeros(C, dtype=np.int64)
    if 0 <= root < C:
        hops[root] = 0
        for h in range(1, max_hops + 1):
            placed = hops >= 0                                      # all of them below h
            todo = np.flatnonzero(~placed & linked[placed].any(axis=0))
            if len(todo) == 0:
                break                                               # nothing joins a later layer either
            new = {int(b): lower_median(estimates(L, U, o, placed, b)) for b in todo}
            for b, v in new.items():
                o[b], hops[b] = v, h
    reached = hops >= 0
    for _ in range(sweeps):
        nxt = o.copy()
        for b in np.flatnonzero(hops > 0):
            nxt[b] = lower_median(estimates(L, U, o, reached, b))
        step, o = nxt - o, nxt
    support = np.zeros(C, dtype=np.int32)
    degree = np.zeros(C, dtype=np.int32)
    for b in np.flatnonzero(reached):
        E = estimates(L, U, o, reached, b)
        degree[b], support[b] = len(E), int((np.abs(E - o[b]) <= tolerance).sum())
    ok = U & reached[:, None] & reached[None, :]
    resid = np.where(ok, L - (o[None, :] - o[:, None]), 0).astype(np.int64)
    state = np.where(ok, np.where(np.abs(resid) <= tolerance, 1, 2), 0).astype(np.int32)
    return {"offset": o, "hops": hops, "support": support, "degree": degree, "step": step.astype(np.int64), "resid": resid,
            "state": state}


def chain(C, step=100):
    """picked tables of C clips in which only the pairs (a, a + 1) were computed, each with lag `step`: (L, R, F), confirm 0"""
    L = np.zeros((C, C), dtype=np.int64)
    R = np.full((C, C), -3, dtype=np.int32)
    for a in range(C):
        R[a, a] = 0
    for a in range(C - 1):
        L[a, a + 1], R[a, a + 1] = step, 0
    return L, R, np.zeros((C, C), dtype=np.int32)


def band(C, k, seed, spacing=40000, reach=100000, bad_pairs=0, masked=False):
    """The [C, C, k] tables of one long event.  Clip i starts at about spacing * i (noise of a tenth of the spacing either way); the
    clips are then shuffled, so the order of the indices says nothing.  A pair is in band when |T_b - T_a| < reach: it holds the true
    lag T_b - T_a with +-1 frame of jitter at a random entry, carrying a LOWER coefficient (0.3 .. 0.5) than its decoys (0.6 .. 0.9,
    random lags), as closure_model.planted does; `bad_pairs` of the in-band pairs hold a decoy in place of the true lag.  A pair out
    of band holds random lags in every entry -- or, when `masked`, (0, NaN, -3) in every entry, what a caller writes for a pair that
    was not computed or is not believed.  The diagonal is what the pool call returns.
    -> dict(lag, coef, ret [C, C, k]; T [C]; true_lag [C, C]; true_entry [C, C], -1 where the pair has none; in_band [C, C])"""
    rng = np.random.default_rng(seed)
    T = spacing * np.arange(C, dtype=np.int64) + rng.integers(-(spacing // 10), spacing // 10 + 1, size=C)
    T = T[rng.permutation(C)].astype(np.int64)
    true_lag = T[None, :] - T[:, None]
    eye = np.eye(C, dtype=bool)
    in_band = (np.abs(true_lag) < reach) & ~eye
    lag = rng.integers(-GARBAGE, GARBAGE, size=(C, C, k)).astype(np.int64)
    coef = rng.uniform(0.6, 0.9, size=(C, C, k))
    ret = np.zeros((C, C, k), dtype=np.int32)
    at = rng.integers(0, k, size=(C, C))
    jitter = rng.integers(-1, 2, size=(C, C))
    weak = rng.uniform(0.3, 0.5, size=(C, C))
    cand = np.argwhere(in_band)
    bad = np.zeros((C, C), dtype=bool)
    if len(cand):
        for a, b in cand[rng.permutation(len(cand))[:min(bad_pairs, len(cand) // 4)]]:
            bad[a, b] = True
    holds = in_band & ~bad
    true_entry = np.where(holds, at, -1).astype(np.int32)
    a_i, b_i = np.nonzero(holds)
    lag[a_i, b_i, at[a_i, b_i]] = (true_lag + jitter)[a_i, b_i]
    coef[a_i, b_i, at[a_i, b_i]] = weak[a_i, b_i]
    if masked:
        out = ~in_band & ~eye
        lag[out], coef[out], ret[out] = 0, np.nan, -3
    d = np.arange(C)
    lag[d, d], coef[d, d] = rng.integers(3000, 140000, size=(C, k)), rng.uniform(0.0, 0.05, size=(C, k))
    lag[d, d, 0], coef[d, d, 0] = 0, 1.0
    return {"lag": lag, "coef": coef, "ret": ret, "T": T, "true_lag": true_lag, "true_entry": true_entry, "in_band": in_band}


def cut(p, at):
    """band()'s tables with every pair between a clip whose T is below T sorted[at] and one at or above it set to (0, NaN, -3): two
    components -> (lag, coef, ret, low), low the mask of the clips of the first"""
    lag, coef, ret = p["lag"].copy(), p["coef"].copy(), p["ret"].copy()
    low = p["T"] < np.sort(p["T"])[at]
    across = low[:, None] != low[None, :]
    lag[across], coef[across], ret[across] = 0, np.nan, -3
    return lag, coef, ret, low
