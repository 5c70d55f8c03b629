"""numpy model of asx_pool_closure_dev (include/audiosync/xcorr_hip.h): the rule in int64 arithmetic, the pick scanning j upwards as
the header states it, vectorised over the third clip and the entries of both legs.  closure(lag, coef, ret, ...) takes the [C, C, k]
tables of an all-pairs top-k call over one pool and returns every output of the call as the device must produce it, bit for bit.
planted(...) builds pools with known clip offsets, decoys that carry the higher coefficient, and a few pairs that miss the truth."""
import numpy as np

LAG_MAX = 1 << 40       # ASX_CLOSURE_LAG_MAX


def valid_entries(lag, ret):
    return (ret == 0) & (lag >= -LAG_MAX) & (lag <= LAG_MAX)


def votes(lag, ret, tolerance):
    """-> int32 [C, C, k]: the clips that support each valid entry off the diagonal"""
    C, _, k = lag.shape
    v = valid_entries(lag, ret)
    L = np.where(v, lag, 0).astype(np.int64)            # a lag that is not valid takes part in no sum that counts
    out = np.zeros((C, C, k), dtype=np.int32)
    eye = np.eye(C, dtype=bool)
    for a in range(C):
        # s[c, b, p, q] = lag(a, c, p) + lag(c, b, q), for c outside {a, b}
        s = L[a][:, None, :, None] + L[:, :, None, :]
        ok = v[a][:, None, :, None] & v[:, :, None, :] & ~eye[:, :, None, None]
        ok[a] = False
        # the reverse pair: rev[b, j, q] = lag(a, b, j) + lag(b, a, q)
        rev = L[a][:, :, None] + L[:, a][:, None, :]
        rev_ok = v[:, a][:, None, :]
        for j in range(k):
            hit = ok & (np.abs(s - L[a, :, j][None, :, None, None]) <= tolerance)
            n = hit.any(axis=(2, 3)).sum(axis=0)
            n = n + ((np.abs(rev[:, j, :]) <= tolerance) & rev_ok[:, 0, :]).any(axis=1)
            out[a, :, j] = np.where(v[a, :, j], n, 0)
        out[a, a] = 0
    return out


def pick(lag, coef, ret, vote):
    """-> the entry of each pair [C, C] int32: j upwards over the valid entries, more votes, then the strictly larger coefficient"""
    C, _, k = lag.shape
    v = valid_entries(lag, ret)
    bj = np.full((C, C), -1, dtype=np.int32)
    bv = np.zeros((C, C), dtype=np.int32)
    bc = np.zeros((C, C), dtype=np.float64)
    for j in range(k):
        take = v[:, :, j] & ((bj < 0) | (vote[:, :, j] > bv) | ((vote[:, :, j] == bv) & (coef[:, :, j] > bc)))
        bj = np.where(take, j, bj).astype(np.int32)
        bv = np.where(take, vote[:, :, j], bv)
        bc = np.where(take, coef[:, :, j], bc)
    return np.where(bj < 0, 0, bj).astype(np.int32)


def confirm(L, good, tolerance):
    """-> int32 [C, C]: the clips that confirm each good pair's picked lag, by picked lags alone"""
    C = L.shape[0]
    G = np.where(good, L, 0).astype(np.int64)
    out = np.zeros((C, C), dtype=np.int32)
    for a in range(C):
        d = G[a][:, None] + G - G[a][None, :]                       # [c, b]: L_ac + L_cb - L_ab; good is False on the diagonal
        n = (good[a][:, None] & good & (np.abs(d) <= tolerance)).sum(axis=0)
        n = n + (good[:, a] & (np.abs(G[a] + G[:, a]) <= tolerance))
        out[a] = np.where(good[a], n, 0)
    return out


def closure(lag, coef, ret, tolerance, min_confirm=1, root=-1):
    """every output of asx_pool_closure_dev as a dict of arrays (root: an int)"""
    return place(picked(lag, coef, ret, tolerance), tolerance, min_confirm, root)


def picked(lag, coef, ret, tolerance):
    """the outputs that do not depend on min_confirm and root (the expensive part): votes, best_*, confirm"""
    lag = np.ascontiguousarray(lag, dtype=np.int64)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    ret = np.ascontiguousarray(ret, dtype=np.int32)
    C, C2, k = lag.shape
    assert C == C2 and coef.shape == lag.shape == ret.shape and 0 <= tolerance <= LAG_MAX
    vote = votes(lag, ret, tolerance)
    entry = pick(lag, coef, ret, vote)
    at = entry[:, :, None].astype(np.int64)
    L = np.take_along_axis(lag, at, axis=2)[:, :, 0]
    best_coef = np.take_along_axis(coef.view(np.int64), at, axis=2)[:, :, 0].view(np.float64)      # the bits
    best_ret = np.take_along_axis(ret, at, axis=2)[:, :, 0]
    good = valid_entries(L, best_ret) & ~np.eye(C, dtype=bool)
    conf = confirm(L, good, tolerance)
    return {"votes": vote, "best_lag": np.ascontiguousarray(L), "best_coef": np.ascontiguousarray(best_coef),
            "best_ret": np.ascontiguousarray(best_ret), "best_entry": entry, "confirm": conf}


def place(first, tolerance, min_confirm=1, root=-1):
    """picked()'s dict plus root, offset, support and placed"""
    L, conf = first["best_lag"], first["confirm"]
    C = L.shape[0]
    assert min_confirm >= 0 and -1 <= root < C
    good = valid_entries(L, first["best_ret"]) & ~np.eye(C, dtype=bool)
    usable = good & (conf >= min_confirm)
    if root < 0:
        score = usable.sum(axis=1) + usable.sum(axis=0)
        root = int(np.argmax(score))                                # the first of the largest
    offset = np.zeros(C, dtype=np.int64)
    support = np.zeros(C, dtype=np.int32)
    placed = np.zeros(C, dtype=np.int32)
    placed[root] = 1
    r = root
    for b in range(C):
        if b == r:
            continue
        E = []
        if usable[r, b]:
            E.append(int(L[r, b]))
        if usable[b, r]:
            E.append(-int(L[b, r]))
        fwd = usable[r] & usable[:, b]
        bwd = usable[b] & usable[:, r]
        fwd[[r, b]] = False
        bwd[[r, b]] = False
        E += (L[r][fwd] + L[:, b][fwd]).tolist()
        E += (-(L[b][bwd] + L[:, r][bwd])).tolist()
        if E:
            E.sort()
            med = E[(len(E) - 1) // 2]
            offset[b], support[b], placed[b] = med, sum(1 for x in E if abs(x - med) <= tolerance), 1
    return dict(first, root=root, offset=offset, support=support, placed=placed)


def by_coefficient(coef, ret):
    """asx_topk_best_dev's entry per pair: among ret == 0 the largest signed coefficient, the smallest j among equals; none: 0"""
    C, _, k = coef.shape
    bj = np.full((C, C), -1, dtype=np.int32)
    bc = np.zeros((C, C))
    for j in range(k):
        take = (ret[:, :, j] == 0) & ((bj < 0) | (coef[:, :, j] > bc))
        bj = np.where(take, j, bj).astype(np.int32)
        bc = np.where(take, coef[:, :, j], bc)
    return np.where(bj < 0, 0, bj).astype(np.int32)


def bad_count(C, bad_pairs):
    """the pairs of planted() that miss the true lag: bad_pairs of them, but never more than a quarter of the C (C - 1) ordered ones"""
    return min(bad_pairs, C * (C - 1) // 4)


def planted(C, k, seed, period=None, bad_pairs=2):
    """A pool of C clips with offsets T.  Every ordered pair a != b holds the true lag T_b - T_a with +-1 frame of jitter at a random
    entry j, carrying a LOWER coefficient (0.3 .. 0.5) than its decoys (0.6 .. 0.9); the decoys are random lags, or the true lag plus
    distinct non-zero multiples of `period`.  bad_count(C, bad_pairs) pairs have a decoy in place of the true lag, one further
    entry is (0, NaN, -3) -- a decoy where k > 1, the entry of a bad pair where k == 1 and there is one -- and the diagonal is what
    the pool call returns: lag 0 with coefficient 1 in entry 0, weak far lags behind it.
    -> dict(lag, coef, ret [C, C, k]; T [C]; true_lag [C, C] (T_b - T_a); true_entry [C, C], -1 where the pair has none)"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 100000, size=C).astype(np.int64)
    lag = np.zeros((C, C, k), dtype=np.int64)
    coef = np.zeros((C, C, k), dtype=np.float64)
    ret = np.zeros((C, C, k), dtype=np.int32)
    true_entry = np.full((C, C), -1, dtype=np.int32)
    true_lag = T[None, :] - T[:, None]
    off = [(a, b) for a in range(C) for b in range(C) if a != b]
    bad = set(tuple(off[i]) for i in rng.permutation(len(off))[:bad_count(C, bad_pairs)]) if off else set()
    for a in range(C):
        for b in range(C):
            if a == b:
                lag[a, a] = [0] + [int(x) for x in rng.integers(3000, 140000, size=k - 1) * rng.choice([-1, 1], size=k - 1)]
                coef[a, a] = [1.0] + list(rng.uniform(0.0, 0.05, size=k - 1))
                continue
            t = int(true_lag[a, b])
            if period is None:
                lag[a, b] = rng.integers(-200000, 200000, size=k)
            else:
                m = rng.permutation(np.array([-4, -3, -2, -1, 1, 2, 3, 4, 5, 6]))[:k]
                lag[a, b] = t + m * period
            coef[a, b] = rng.uniform(0.6, 0.9, size=k)
            j = int(rng.integers(0, k))
            jitter = int(rng.integers(-1, 2))
            if (a, b) not in bad:
                lag[a, b, j], coef[a, b, j], true_entry[a, b] = t + jitter, rng.uniform(0.3, 0.5), j
    if k > 1 and off:
        a, b = off[int(rng.integers(0, len(off)))]
        j = (int(true_entry[a, b]) + 1) % k                         # never the true entry
        lag[a, b, j], coef[a, b, j], ret[a, b, j] = 0, np.nan, -3
    elif bad:
        a, b = sorted(bad)[0]
        lag[a, b, 0], coef[a, b, 0], ret[a, b, 0] = 0, np.nan, -3
    return {"lag": lag, "coef": coef, "ret": ret, "T": T, "true_lag": true_lag, "true_entry": true_entry}
