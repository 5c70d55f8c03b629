"""Where a track and a buffer begin and end, for every device-pointer entry point (include/audiosync/xcorr_hip.h).

One rule: on one plan, the call on poisoned, strided, guarded buffers (tests/edges.py) returns byte for byte what the same call
returns on the materialised clean buffers; every guard keeps its sentinel; every input buffer keeps its bytes; and the plan's
counters (peak_overflows, peak_repairs, pearson_modes, prune_stats, qstore_stats) move by the same amounts in both runs.  Both
poisons run: a quiet NaN, and +-1e30.  Index and row arrays are poisoned by value: window rows at window_stride = 2 with rows in
between that exclude the pair's lag, pool pair rows with an index outside the pool ahead and behind, centres outside [-N, N-1] ahead
and behind, lines at line_stride = 3 with NaN in the third double.  The clean run is anchored once per length against
oracle.cross_correlation (lag and ret equal, coefficient within the project's 1e-5), so that equality of two wrong answers cannot pass.

Placement.  Real-column plans (N = 144 000: the 300-row column kernel, 288 000: 600 rows, 480 000: 400 rows): a 16-byte aligned
base 64 floats into the buffer, source stride 2N + 68, sample stride N + 36, and N + 64 floats of poison behind the last sample (the
zero half a wrong loader would read).  Packed plans (N = 1000 as 25x40x8, 999, 45, 6): 5 floats in front, so that the base is
float-aligned only, source stride 2N + 3, sample stride N + 1 -- the 4-byte fall-back of the loads -- and once with a 16-byte aligned
base and strides that are multiples of 4, the 16-byte loads.  Batch 3; max_batch = 2 once per family, so that the call runs in more
than one launch group.  All three real-column lengths run for the strided and the pool call, which share their loaders with the
rest; every other entry point runs at 144 000, and at 1000 where a packed plan is accepted.  Curve, track and warp also run at
N = 999: a sweep of 3 mod 4 frames, whose last 16-byte load of the sample would take the poison behind it if it were one too wide.

Every path that reads the inputs has a case of its own, with the counter that shows that the path was taken: the direct Pearson
reduction; the second look (k_refine_dots) on a periodic pair and, through the DC kernels, on a pair with a large offset in both
tracks; the spectral form handing a pair to the direct form; true lags N - 1, -N + 1 and -N; the partial-store redo at N = 960 000;
the unpruned kernels.  Rows outside the contract keep the values the other tests pin (-2, -4, -5) and leave their neighbours alone.

Shown to fail, on builds with one line changed each (this file and test_gpu_sweep_lengths.py; nothing of them is kept):
    sweep_samples `t4 + 3u <= cnt` (one sample frame too many): test_curve_track_and_warp at N = 999, curve and warp, both poisons;
        in test_gpu_sweep_lengths.py the track at N = 7, 1027, 4099, 1 440 000, the warp at 3, 7, 1023, 1027, the batch invariant
        at seven lengths and the misaligned pair at five
    k_fwd_cols_r `m < M1` (the sample's zero half is loaded): every test of this file that runs a transform on a real-column plan,
        76 cases from test_strided to test_the_partial_store_redo (this file only: the other one stages its samples through the
        library's own allocations of exactly N frames, which such a kernel would leave by N frames)
    curve_write `tid <= n` (one value of r too many): the back guard of d_r in test_curve_track_and_warp (curve, every length and
        poison) and over pools; in test_gpu_sweep_lengths.py the curve, the track's S = 1 equality, the warp's equality, the batch
        invariant and the misaligned pair
Measured worst |coef - oracle| of the anchors (printed as "track edges: anchor"): 0.019 of the 1e-5 allowed, at N = 480 000.
"""
import collections

import numpy as np
import pytest

import edges
import guards_ref
import oracle
from test_gpu_curve import delays, pair
from util import asx

pytestmark = pytest.mark.gpu

REAL = (144000, 288000, 480000)
PACKED = {1000: "25x40x8", 999: None, 45: None, 6: None}
B = 3
COEF_TOL = 1e-5

Place = collections.namedtuple("Place", "front ss ts back")      # strides in floats, 0 = one track for every pair
Aux = collections.namedtuple("Aux", "rows stride dirty_rows dirty_row_stride dirty_stride filler")


def up4(v):
    return (v + 3) // 4 * 4


def place_of(n, which="both", aligned=None):
    """the poisoned placement of the table above; which: both / source0 / sample0 / both0 / contiguous"""
    real = n in REAL
    aligned = real if aligned is None else aligned
    front = 64 if real else (8 if aligned else 5)
    ss, ts = (2 * n + 68, n + 36) if real else ((up4(2 * n) + 4, up4(n) + 4) if aligned else (2 * n + 3, n + 1))
    if which == "contiguous":
        ss, ts = 2 * n, n
    if which in ("source0", "both0"):
        ss = 0
    if which in ("sample0", "both0"):
        ts = 0
    return Place(front, ss, ts, n + 64 if real else None)


def tracks(n, count=B):
    """(sources [count, 2N], samples [count, N]): pair(n, seed), whose strongest lag is delays(n)[0] + 5 * seed"""
    return np.stack([pair(n, s)[0] for s in range(count)]), np.stack([pair(n, s)[1] for s in range(count)])


def true_lag(n, seed):
    return delays(n)[0] + 5 * seed


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch(mod):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def plans(mod):
    """one plan per (length, max_batch), kept for the module"""
    cache = {}

    def get(n, max_batch=4):
        if (n, max_batch) not in cache:
            plan = mod.Plan(n, max_batch, 0, PACKED.get(n))
            assert plan.layout == ("real-column" if n in REAL else "packed"), (n, plan.layout)
            cache[n, max_batch] = plan
        return cache[n, max_batch]
    yield get
    for plan in cache.values():
        plan.close()


# ---- the engine -------------------------------------------------------------------------------------------------------------------

def counters(plan):
    if plan is None:
        return ()
    return (plan.peak_overflows(), plan.peak_repairs()) + tuple(plan.pearson_modes()) + tuple(plan.prune_stats()) + tuple(plan.qstore_stats())


def ptr(buffer, offset):
    return buffer.data_ptr() + offset * buffer.element_size()


def windows_aux(rows, n):
    """window rows at window_stride = 2 (clean: 1); the rows in between hold [-N, -N], which excludes every pair's lag"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    return Aux(rows, 1, rows, 2, 2, [-n, -n])


def pairs_aux(rows, ns, nm):
    """pool pair rows (int32, contiguous by definition): an index outside both pools ahead of the first and behind the last row"""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return Aux(rows, None, rows, 1, None, [ns + 5, nm + 5])


def centres_aux(cs, n):
    """centres (int64, contiguous by definition): a lag outside [-N, N-1] ahead and behind"""
    rows = np.asarray(cs, dtype=np.int64).reshape(-1, 1)
    return Aux(rows, None, rows, 1, None, [n + 5])


def lines_aux(lines):
    """lines at line_stride = 3 with NaN in the third double (clean: a packed array, line_stride = 2), NaN rows ahead and behind"""
    rows = np.asarray(lines, dtype=np.float64).reshape(-1, 2)
    return Aux(rows, 2, np.concatenate([rows, np.full((len(rows), 1), np.nan)], axis=1), 1, 3, [np.nan] * 3)


def call_once(torch, plan, launch, src, smp, place, auxes, outs, poison):
    """one call -> (the outputs as host arrays, what the plan's counters moved by).  poison None: dense clean buffers and outputs of
    the documented size filled with 7s, as the other tests build them (behind each, outside the view the call gets, the allocation
    goes on for a few elements that nobody checks, so that a wrong kernel's stray access stays inside memory the test owns); else:
    the placement `place` in poison, guarded outputs, and the checks on both."""
    n = smp.shape[1]
    held = []
    if poison is None:
        d_s, so, ss = edges.materialise(src[:1] if place.ss == 0 else src, torch, slack=64), 0, (0 if place.ss == 0 else 2 * n)
        d_t, to, ts = edges.materialise(smp[:1] if place.ts == 0 else smp, torch, slack=place.back or 64), 0, (0 if place.ts == 0 else n)
    else:
        d_s, so, ss = edges.embed(src, place.front, place.ss, poison, torch)
        d_t, to, ts = edges.embed(smp, place.front, place.ts, poison, torch, back=place.back)
    held += [d_s, d_t]
    ax = []
    for a in auxes:
        if a is None:
            ax.append((0, 0))
            continue
        if poison is None:
            buf, off = edges.embed_rows(a.rows, 1, a.filler[:a.rows.shape[1]], front=0, torch=torch)   # dense: no filler is left
            ax.append((ptr(buf, off), a.stride))
        else:
            buf, off = edges.embed_rows(a.dirty_rows, a.dirty_row_stride, a.filler, front=2, torch=torch)
            ax.append((ptr(buf, off), a.dirty_stride))
        held.append(buf)
    wholes, views = [], []
    for o in outs:
        if o is None:
            wholes.append(None)
            views.append(None)
        elif poison is None:
            w = torch.full((o[1] + 8,), edges.PAYLOAD, dtype=getattr(torch, o[0]), device="cuda")[:o[1]]   # (eight spare elements behind)
            wholes.append(w)
            views.append(w)
        else:
            w, v = edges.guarded(torch, o[0], o[1])
            wholes.append(w)
            views.append(v)
    before = [edges.snapshot(b) for b in held]
    torch.cuda.synchronize()
    c0 = counters(plan)
    launch(plan, ptr(d_s, so), ss, ptr(d_t, to), ts, ax, [0 if v is None else v.data_ptr() for v in views])
    if plan is not None:
        plan.sync()
    torch.cuda.synchronize()
    moved = tuple(b - a for a, b in zip(c0, counters(plan)))
    for k, (b, was) in enumerate(zip(held, before)):
        assert edges.unchanged(b, was), "input buffer %d was written to" % k
    if poison is not None:
        for k, (w, o) in enumerate(zip(wholes, outs)):
            if w is not None:
                assert edges.check_guards(w, o[1]) == [], (k, o)
    return [None if v is None else v.cpu().numpy() for v in views], moved


def both(torch, plan, launch, src, smp, place, auxes, outs, poison):
    """the rule: the clean run and the poisoned run -> (the clean run's outputs, the counters' movement)"""
    clean, moved = call_once(torch, plan, launch, src, smp, place, auxes, outs, None)
    dirty, moved_dirty = call_once(torch, plan, launch, src, smp, place, auxes, outs, poison)
    assert moved == moved_dirty, ("counters", moved, moved_dirty)
    for k, (a, b) in enumerate(zip(clean, dirty)):
        if a is not None:
            assert a.tobytes() == b.tobytes(), ("output %d" % k, np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[:8].tolist(),
                                                a.reshape(-1)[:6].tolist(), b.reshape(-1)[:6].tolist())
    return clean, moved


_oracle = {}


def oracle_of(src, smp, key):
    if key not in _oracle:
        _oracle[key] = [oracle.cross_correlation(s, t) for s, t in zip(src, smp)]
    return _oracle[key]


def anchored(lag, coef, ret, src, smp, key):
    """(lag, coef, ret) of a clean run against the oracle, pair by pair"""
    worst = 0.0
    for i, (o_ret, o_lag, o_coef) in enumerate(oracle_of(src, smp, key)):
        assert (int(ret[i]), int(lag[i])) == (o_ret, o_lag), (key, i, int(ret[i]), int(lag[i]), o_ret, o_lag)
        if np.isnan(o_coef):
            assert np.isnan(coef[i]), (key, i, float(coef[i]))
        else:
            worst = max(worst, abs(float(coef[i]) - o_coef))
            assert abs(float(coef[i]) - o_coef) < COEF_TOL, (key, i, float(coef[i]), o_coef)
    print("track edges: anchor", key, "worst |coef - oracle| / 1e-5", worst / COEF_TOL)


LCR = [("int64", B), ("float64", B), ("int32", B)]


def strided(plan, S, ss, T, ts, ax, o):
    plan.xcorr_strided_dev(S, ss, T, ts, B, *o)


def which_tracks(src, smp, which):
    """the pairs a placement correlates: a stride of 0 broadcasts track 0"""
    s = np.stack([src[0]] * len(src)) if which in ("source0", "both0") else src
    t = np.stack([smp[0]] * len(smp)) if which in ("sample0", "both0") else smp
    return s, t


# ---- 1. the strided call: every placement, every length ------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("which", ["both", "source0", "sample0", "both0"])
@pytest.mark.parametrize("n", list(REAL) + list(PACKED))
def test_strided(torch, plans, n, which, poison):
    src, smp = tracks(n)
    plan = plans(n)
    (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place_of(n, which), [], LCR, poison)
    anchored(lag, coef, ret, *which_tracks(src, smp, which), key=(n, which))
    if n in REAL and which == "both":
        assert moved[6] > 0, moved                               # the pruned inverse pass ran (tiles in all)
    if n in PACKED:                                              # ... and the 16-byte loads: an aligned base, strides in fours
        got, _ = both(torch, plan, strided, src, smp, place_of(n, which, aligned=True), [], LCR, poison)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (lag, coef, ret)))


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_strided_in_more_than_one_launch_group(torch, plans, n, poison):
    src, smp = tracks(n)
    (lag, coef, ret), _ = both(torch, plans(n, 2), strided, src, smp, place_of(n), [], LCR, poison)
    anchored(lag, coef, ret, src, smp, key=(n, "both"))


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_batch(torch, plans, n, poison):
    """contiguous by definition: poison ahead of pair 0 and behind the last pair"""
    src, smp = tracks(n)

    def launch(plan, S, ss, T, ts, ax, o):
        assert (ss, ts) == (2 * n, n)
        plan.xcorr_batch_dev(S, T, B, *o)
    (lag, coef, ret), _ = both(torch, plans(n), launch, src, smp, place_of(n, "contiguous"), [], LCR, poison)
    anchored(lag, coef, ret, src, smp, key=(n, "both"))


# ---- 2. windows, top-k, PHAT ---------------------------------------------------------------------------------------------------------

def window_rows(n):
    return [[-n, n - 1], [true_lag(n, 1) - 10, true_lag(n, 1) + 10], [0, n - 1]]


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_windowed(torch, plans, n, poison):
    src, smp = tracks(n)

    def launch(plan, S, ss, T, ts, ax, o):
        plan.xcorr_windowed_dev(S, ss, T, ts, ax[0][0], ax[0][1], B, *o)
    (lag, coef, ret), _ = both(torch, plans(n), launch, src, smp, place_of(n), [windows_aux(window_rows(n), n)], LCR, poison)
    anchored(lag, coef, ret, src, smp, key=(n, "both"))           # every window holds its pair's peak
    # a row that is not a window: -2, its neighbours unaffected
    rows = window_rows(n)
    rows[1] = [5, 3]
    (lag2, coef2, ret2), _ = both(torch, plans(n), launch, src, smp, place_of(n), [windows_aux(rows, n)], LCR, poison)
    assert (int(lag2[1]), int(ret2[1])) == (0, -2) and np.isnan(coef2[1])
    for k in (0, 2):
        assert (lag2[k], coef2[k].tobytes(), ret2[k]) == (lag[k], coef[k].tobytes(), ret[k]), k


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_topk(torch, plans, n, poison):
    src, smp = tracks(n)
    outs = [("int64", 3 * B), ("float64", 3 * B), ("int32", 3 * B)]

    def launch(plan, S, ss, T, ts, ax, o):
        plan.xcorr_topk_dev(S, ss, T, ts, ax[0][0], ax[0][1], B, 3, 8, *o)
    (lag, coef, ret), _ = both(torch, plans(n), launch, src, smp, place_of(n), [windows_aux([[-n, n - 1]] * B, n)], outs, poison)
    assert ret.tolist() == [0] * (3 * B)
    assert lag.reshape(B, 3).tolist() == [[d + 5 * s for d in delays(n)] for s in range(B)]      # the three planted delays, in order
    both(torch, plans(n), launch, src, smp, place_of(n), [None], outs, poison)                    # ... and with the plan's window


def band_of(n):
    return n // 8, n // 2


PHAT = {
    "phat": (lambda p, S, ss, T, ts, W, ws, n, o: p.xcorr_phat_dev(S, ss, T, ts, W, ws, B, *o),
             [("int64", B), ("float64", B), ("float64", B), ("int32", B)]),
    "phat_band": (lambda p, S, ss, T, ts, W, ws, n, o: p.xcorr_phat_band_dev(S, ss, T, ts, W, ws, B, *band_of(n), *o),
                  [("int64", B), ("float64", B), ("float64", B), ("int32", B)]),
    "phat_sub": (lambda p, S, ss, T, ts, W, ws, n, o: p.xcorr_phat_sub_dev(S, ss, T, ts, W, ws, B, *band_of(n), 8, *o),
                 [("int64", B), ("float64", B), ("float64", B), ("float64", B), ("float64", B * 17), ("int32", B)]),
    "phat_topk": (lambda p, S, ss, T, ts, W, ws, n, o: p.xcorr_phat_topk_dev(S, ss, T, ts, W, ws, B, *band_of(n), 3, 8, *o),
                  [("int64", 3 * B), ("float64", 3 * B), ("float64", 3 * B), ("int32", 3 * B)]),
}


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("name", list(PHAT))
def test_phat(torch, plans, name, poison):
    """real-column plans only.  The lag is the whitened curve's float32 argmax: it is anchored to the planted delay"""
    n = 144000
    src, smp = tracks(n)
    call, outs = PHAT[name]

    def launch(plan, S, ss, T, ts, ax, o):
        call(plan, S, ss, T, ts, ax[0][0], ax[0][1], n, o)
    got, moved = both(torch, plans(n), launch, src, smp, place_of(n), [windows_aux(window_rows(n), n)], outs, poison)
    k = 3 if name == "phat_topk" else 1
    assert got[0].reshape(B, k)[:, 0].tolist() == [true_lag(n, s) for s in range(B)] and got[-1].tolist() == [0] * (B * k)
    assert moved == (0,) * len(moved), moved                      # the PHAT calls touch no counter
    both(torch, plans(n), launch, src, smp, place_of(n, "source0"), [None], outs, poison)


# ---- 3. the pool forms ---------------------------------------------------------------------------------------------------------------

NS, NM = 2, 3
LISTED = [[1, 1], [0, 0], [1, 2]]          # two pairs of matching tracks (lags delays(n)[0] + 5, + 0) and an unrelated one


def pools(n):
    src, smp = tracks(n, NM)
    return src[:NS], smp


def pool_launch(name, n, batch, k=1):
    def launch(plan, S, ss, T, ts, ax, o):
        head = (S, ss, NS, T, ts, NM, ax[0][0], ax[1][0], ax[1][1], batch)
        if name == "pool":
            plan.xcorr_pool_dev(*head, *o)
        elif name == "pool_topk":
            plan.xcorr_pool_topk_dev(*head, k, 8, *o)
        elif name == "pool_phat":
            plan.xcorr_pool_phat_dev(*head, *band_of(n), *o)
        elif name == "pool_phat_sub":
            plan.xcorr_pool_phat_sub_dev(*head, *band_of(n), 8, *o)
        else:
            plan.xcorr_pool_phat_topk_dev(*head, *band_of(n), k, 8, *o)
    return launch


def pool_outs(name, batch):
    if name == "pool":
        return [("int64", batch), ("float64", batch), ("int32", batch)]
    if name == "pool_topk":
        return [("int64", 3 * batch), ("float64", 3 * batch), ("int32", 3 * batch)]
    if name == "pool_phat":
        return [("int64", batch), ("float64", batch), ("float64", batch), ("int32", batch)]
    if name == "pool_phat_sub":
        return [("int64", batch), ("float64", batch), ("float64", batch), ("float64", batch), ("float64", batch * 17), ("int32", batch)]
    return [("int64", 3 * batch), ("float64", 3 * batch), ("float64", 3 * batch), ("int32", 3 * batch)]


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", REAL)
def test_pool(torch, plans, n, poison):
    """listed pairs, every combination, and a pair outside its pool, at every real-column length"""
    src, smp = pools(n)
    launch = pool_launch("pool", n, B)
    (lag, coef, ret), _ = both(torch, plans(n), launch, src, smp, place_of(n), [pairs_aux(LISTED, NS, NM), None], pool_outs("pool", B), poison)
    anchored(lag, coef, ret, [src[a] for a, _ in LISTED], [smp[b] for _, b in LISTED], key=(n, "listed"))
    every, _ = both(torch, plans(n), pool_launch("pool", n, NS * NM), src, smp, place_of(n), [None, None], pool_outs("pool", NS * NM), poison)
    for k, (a, b) in enumerate(LISTED):                           # d_pairs = NULL: source-major
        assert all(x[a * NM + b].tobytes() == y[k].tobytes() for x, y in zip(every, (lag, coef, ret))), (a, b)
    rows = [LISTED[0], [NS, 0], LISTED[2]]                        # row 1 names a source outside its pool: -4 (with full window rows)
    (lag2, coef2, ret2), _ = both(torch, plans(n), launch, src, smp, place_of(n), [pairs_aux(rows, NS, NM), windows_aux([[-n, n - 1]] * B, n)],
                                  pool_outs("pool", B), poison)
    assert (int(lag2[1]), int(ret2[1])) == (0, -4) and np.isnan(coef2[1])
    for k in (0, 2):
        assert (lag2[k], coef2[k].tobytes(), ret2[k]) == (lag[k], coef[k].tobytes(), ret[k]), k


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("name", ["pool_topk", "pool_phat", "pool_phat_sub", "pool_phat_topk"])
def test_pool_forms(torch, plans, name, poison):
    n = 144000
    src, smp = pools(n)
    k = 3 if name.endswith("topk") else 1
    got, _ = both(torch, plans(n), pool_launch(name, n, B, k), src, smp, place_of(n), [pairs_aux(LISTED, NS, NM), None], pool_outs(name, B), poison)
    assert got[-1].tolist() == [0] * (B * k)
    every, _ = both(torch, plans(n), pool_launch(name, n, NS * NM, k), src, smp, place_of(n), [None, windows_aux([[-n, n - 1]] * (NS * NM), n)],
                    pool_outs(name, NS * NM), poison)
    for i, (a, b) in enumerate(LISTED):
        for x, y in zip(every, got):
            w = x.size // (NS * NM)
            assert x[(a * NM + b) * w:(a * NM + b + 1) * w].tobytes() == y[i * w:(i + 1) * w].tobytes(), (name, a, b)


@pytest.mark.parametrize("poison", edges.POISONS)
def test_pool_in_more_than_one_launch_group(torch, plans, poison):
    n = 144000
    src, smp = pools(n)
    (lag, coef, ret), _ = both(torch, plans(n, 2), pool_launch("pool", n, NS * NM), src, smp, place_of(n), [None, None],
                               pool_outs("pool", NS * NM), poison)
    anchored(lag, coef, ret, [src[i // NM] for i in range(NS * NM)], [smp[i % NM] for i in range(NS * NM)], key=(n, "every"))


# ---- 4. curve, track and warp --------------------------------------------------------------------------------------------------------

def warp_lines(n):
    """as far from the centre as a valid line allows"""
    return [[0.0, 0.0], [2.0 ** -6, n / 2], [-(2.0 ** -6), -(n / 2)]]


def sweep_case(name, n, batch, pool, coef=True):
    """(launch, outputs) of curve / track / warp (h = 8; the track: S = 8, h = 16), strided or over the pools"""
    if name == "curve":
        outs = [("float64", batch * 17), ("float64", batch * 17) if coef else None, ("float64", batch), ("int32", batch)]
    elif name == "track":
        outs = [("float64", batch * 8 * 33), ("float64", batch * 8 * 2), ("float64", batch * 3), ("int32", batch), ("int32", batch)]
    else:
        outs = [("float64", batch * 17), ("float64", batch), ("float64", batch), ("int64", batch), ("int32", batch)]

    def launch(plan, S, ss, T, ts, ax, o):
        head = (S, ss, NS, T, ts, NM, ax[1][0]) if pool else (S, ss, T, ts)
        fn = getattr(plan, "xcorr_%s%s_dev" % ("pool_" if pool else "", name))
        if name == "curve":
            fn(*head, batch, 1, ax[0][0], 8, *o)
        elif name == "track":
            fn(*head, batch, 1, ax[0][0], 16, 8, *o)
        else:
            fn(*head, batch, 1, ax[0][0], ax[2][0], ax[2][1], 8, *o)
    return launch, outs


def sweep_centres(n):
    return [true_lag(n, 0), -n, n - 1]


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("name", ["curve", "curve_r_only", "track", "warp"])
@pytest.mark.parametrize("n", [144000, 1000, 999])
def test_curve_track_and_warp(torch, plans, n, name, poison):
    src, smp = tracks(n)
    coef = name != "curve_r_only"
    name = name.split("_")[0]
    launch, outs = sweep_case(name, n, B, False, coef)
    auxes = [centres_aux(sweep_centres(n), n), None, lines_aux(warp_lines(n))]
    got, moved = both(torch, plans(n), launch, src, smp, place_of(n), auxes, outs, poison)
    assert set(got[-1].tolist()) <= {0, -1} and int(got[-1][0]) == 0, got[-1]
    assert moved == (0,) * len(moved)
    assert float(got[0].reshape(B, -1)[0, 8 if name != "track" else 16]) > 0.5 * n / (8 if name == "track" else 1)   # the planted delay
    both(torch, plans(n), launch, src, smp, place_of(n, "sample0"), auxes, outs, poison)
    both(torch, plans(n, 2), launch, src, smp, place_of(n), auxes, outs, poison)          # three entries in slices of two
    # entries outside the contract: a centre outside [-N, N-1] (-2) and, for the warp, a line that is not valid (-5)
    bad = [centres_aux([true_lag(n, 0), n, n - 1], n), None, lines_aux([[0.0, 0.0], [0.0, 0.0], [np.nan, 0.0]])]
    worse, _ = both(torch, plans(n), launch, src, smp, place_of(n), bad, outs, poison)
    assert worse[-1].tolist() == ([0, -2, -5] if name == "warp" else [0, -2, 0]), worse[-1]
    w = got[0].size // B
    assert worse[0][:w].tobytes() == got[0][:w].tobytes() and np.isnan(worse[0][w:2 * w]).all()
    if name != "warp":
        assert worse[0][2 * w:].tobytes() == got[0][2 * w:].tobytes()


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("name", ["curve", "track", "warp"])
def test_curve_track_and_warp_over_pools(torch, plans, name, poison):
    n = 144000
    src, smp = pools(n)
    cs = [true_lag(n, 1), -n, n - 1]
    launch, outs = sweep_case(name, n, B, True)
    auxes = [centres_aux(cs, n), pairs_aux(LISTED, NS, NM), lines_aux(warp_lines(n))]
    got, _ = both(torch, plans(n), launch, src, smp, place_of(n), auxes, outs, poison)
    # ... is the strided form entry by entry
    for k, (a, b) in enumerate(LISTED):
        one_launch, one_outs = sweep_case(name, n, 1, False)
        one, _ = call_once(torch, plans(n), one_launch, src[a:a + 1], smp[b:b + 1], place_of(n),
                           [centres_aux(cs[k:k + 1], n), None, lines_aux(warp_lines(n)[k:k + 1])], one_outs, None)
        for x, y in zip(got, one):
            w = y.size
            assert x[k * w:(k + 1) * w].tobytes() == y.tobytes(), (name, k)
    launch, outs = sweep_case(name, n, NS * NM, True)                # d_pairs = NULL: every combination
    auxes = [centres_aux([0, -1, 1, n - 1, -n, 5], n), None, lines_aux(warp_lines(n) * 2)]
    both(torch, plans(n), launch, src, smp, place_of(n), auxes, outs, poison)
    rows = [LISTED[0], [0, NM], LISTED[2]]                            # row 1 names a sample outside its pool: -4
    launch, outs = sweep_case(name, n, B, True)
    worse, _ = both(torch, plans(n), launch, src, smp, place_of(n), [centres_aux(cs, n), pairs_aux(rows, NS, NM), lines_aux(warp_lines(n))],
                    outs, poison)
    assert int(worse[-1][1]) == -4 and worse[-1][0] == got[-1][0] and worse[-1][2] == got[-1][2]
    w = got[0].size // B
    assert worse[0][:w].tobytes() == got[0][:w].tobytes() and np.isnan(worse[0][w:2 * w]).all() and worse[0][2 * w:].tobytes() == got[0][2 * w:].tobytes()


# ---- 5. the debug calls: the whole of r -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n, name", [(144000, "debug_r"), (1000, "debug_r"), (144000, "phat_debug_r"), (144000, "phat_band_debug_r")])
def test_debug_r(torch, plans, n, name, poison):
    src, smp = tracks(n, 1)
    outs = [("float32", 2 * n), ("int64", 1), ("float64", 1)] + ([("float64", 1)] if name != "debug_r" else []) + [("int32", 1)]

    def launch(plan, S, ss, T, ts, ax, o):
        if name == "debug_r":
            plan.debug_r_dev(S, T, *o)
        elif name == "phat_debug_r":
            plan.phat_debug_r_dev(S, T, *o)
        else:
            plan.phat_band_debug_r_dev(S, T, *band_of(n), *o)
    got, _ = both(torch, plans(n), launch, src, smp, place_of(n, "contiguous"), [], outs, poison)
    assert int(got[1][0]) == true_lag(n, 0) and int(got[-1][0]) == 0
    assert int(np.argmax(np.abs(got[0]))) == true_lag(n, 0) and np.isfinite(got[0]).all()


# ---- 6. every path that reads the inputs ------------------------------------------------------------------------------------------------

def with_pairs(n, *others):
    """pair(n, 0), the given pairs, pair(n, 1): a batch of three or more with ordinary neighbours"""
    (s0, t0), (s1, t1) = pair(n, 0), pair(n, 1)
    return np.stack([s0] + [o[0] for o in others] + [s1]), np.stack([t0] + [o[1] for o in others] + [t1])


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_the_direct_pearson_reduction(torch, plans, n, poison):
    src, smp = tracks(n)
    plan = plans(n)
    plan.set_pearson(False)
    try:
        (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place_of(n), [], LCR, poison)
    finally:
        if n in REAL:
            plan.set_pearson(True)
    anchored(lag, coef, ret, src, smp, key=(n, "both"))
    assert moved[2:5] == (0, 0, 0), moved                          # under the direct setting the mode counters count nothing


def periodic(n):
    """a source periodic in 8 frames: 2N / 8 exactly tied peaks overflow the near-tie list (tests/test_gpu_exact_peak.py)"""
    per = np.tile(np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32), 2 * n // 8)
    return per, per[:n].copy()


def offset_pair(n):
    """an offset of a thousand deviations in both tracks: every lag is a near-tie, and the second look runs on the mean-removed
    source (the DC kernels; tests/test_gpu_exact_peak.py)"""
    rng = np.random.default_rng(41)
    d = int(rng.integers(-n // 2, n // 2))
    x = rng.normal(size=3 * n)
    return (1e3 + x[n:3 * n]).astype(np.float32), (700.0 + 0.5 * x[n + d:2 * n + d] + 0.3 * rng.normal(size=n)).astype(np.float32)


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("kind", ["periodic", "offset"])
def test_the_second_look(torch, plans, kind, poison):
    n = 144000
    plan = plans(n)
    assert plan.peak_capacity < 2 * n // 8
    src, smp = with_pairs(n, periodic(n) if kind == "periodic" else offset_pair(n))
    (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place_of(n), [], LCR, poison)
    assert moved[:2] == (1, 1), moved                              # one pair overflowed and was looked at again
    anchored(lag, coef, ret, src, smp, key=(n, kind))
    if kind == "periodic":
        assert (int(lag[1]), float(coef[1]), int(ret[1])) == (0, 1.0, 0)


@pytest.mark.parametrize("poison", edges.POISONS)
def test_a_pair_the_spectral_form_hands_to_the_direct_form(torch, plans, poison):
    n = 144000
    v, s, t, lag0 = guards_ref.sweep_pairs(n, "surround")[-1]      # the source outside the matching window three times as loud
    assert guards_ref.predict(s.astype(np.float64), t.astype(np.float64), lag0, 2 * n)[1] == guards_ref.DIRECT
    plan = plans(n)
    _, usual = both(torch, plan, strided, *tracks(n), place_of(n), [], LCR, poison)
    src, smp = with_pairs(n, (s, t))
    (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place_of(n), [], LCR, poison)
    assert sum(usual[2:5]) == sum(moved[2:5]) == B and moved[4] == usual[4] + 1, (usual, moved)
    anchored(lag, coef, ret, src, smp, key=(n, "surround"))
    assert int(lag[1]) == lag0


def edge_pairs(n):
    """true lags N - 1 (the source's segment ends on its last frame but one), -N + 1 (one frame lines up: the source's first with
    the sample's last) and -N (the empty segment)"""
    rng = np.random.default_rng(7)
    a_src = rng.standard_normal(2 * n).astype(np.float32)
    a_smp = (a_src[n - 1:2 * n - 1] + 0.1 * rng.standard_normal(n)).astype(np.float32)
    b_src = (0.01 * rng.standard_normal(2 * n)).astype(np.float32)
    b_smp = (0.01 * rng.standard_normal(n)).astype(np.float32)
    b_src[0] = b_smp[n - 1] = 100.0
    c_src = rng.standard_normal(2 * n).astype(np.float32)
    c_smp = c_src[n:].copy()
    return np.stack([a_src, b_src, c_src]), np.stack([a_smp, b_smp, c_smp])


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("n", [144000, 1000])
def test_lags_at_the_ends_of_the_track(torch, plans, n, poison):
    src, smp = edge_pairs(n)
    (lag, coef, ret), _ = both(torch, plans(n), strided, src, smp, place_of(n), [], LCR, poison)
    assert lag.tolist() == [n - 1, -n + 1, -n], lag
    assert int(ret[2]) == -1 and np.isnan(coef[2])                  # lag -N reads nothing: NaN and -1 in both runs
    anchored(lag, coef, ret, src, smp, key=(n, "edges"))
    plan = plans(n)
    plan.set_pearson(False)                                        # ... and through the direct reduction
    try:
        (lag, coef, ret), _ = both(torch, plan, strided, src, smp, place_of(n), [], LCR, poison)
    finally:
        if n in REAL:
            plan.set_pearson(True)
    anchored(lag, coef, ret, src, smp, key=(n, "edges"))


@pytest.mark.parametrize("poison", edges.POISONS)
def test_the_unpruned_kernels(torch, plans, poison):
    n = 144000
    src, smp = tracks(n)
    plan = plans(n)
    plan.set_prune(False)
    try:
        (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place_of(n), [], LCR, poison)
    finally:
        plan.set_prune(True)
    assert moved[5:7] == (0, 0), moved
    anchored(lag, coef, ret, src, smp, key=(n, "both"))


@pytest.mark.parametrize("poison", edges.POISONS)
def test_the_partial_store_redo(mod, torch, poison):
    """N = 960 000, the smallest length with partial storing: the comb pair of tests/test_gpu_qstore.py, whose prediction is wrong,
    is run again through the full-store kernels"""
    from test_qstore_model import comb_pair
    n, m2 = 960000, 2400
    m1 = n // m2
    comb = comb_pair(n, m1, m1 // 3, 8, 123456, 300700, 77)
    src, smp = with_pairs(n, comb)
    place = Place(64, 2 * n + 68, n + 36, n + 64)
    with mod.Plan(n, B, 0) as plan:
        assert plan.layout == "real-column"
        plan.set_qstore(2)
        (lag, coef, ret), moved = both(torch, plan, strided, src, smp, place, [], LCR, poison)
    assert moved[7] + moved[8] == B and moved[9] >= 1, moved         # (a list, everything, run again, tiles stored)
    assert ret.tolist() == [0, 0, 0]
    anchored(lag, coef, ret, src, smp, key=(n, "comb"))


# ---- 7. the epilogues and the generator -------------------------------------------------------------------------------------------------

def rows_in_poison(torch, values, filler, poisoned):
    """a contiguous input array of an epilogue: dense, or with two fillers ahead and behind -> (buffer, pointer)"""
    rows = np.asarray(values).reshape(-1, 1)
    buf, off = edges.embed_rows(rows, 1, [filler], front=2 if poisoned else 0, torch=torch)
    return buf, ptr(buf, off)


def c_round(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


@pytest.mark.parametrize("batch", [1, 255, 256, 257])
def test_results_to_ms(mod, torch, batch):
    rng = np.random.default_rng(batch)
    lag = rng.integers(-144000, 144000, batch).astype(np.int64)
    lag += (lag % 48 == 24)                                         # no exact halves of a millisecond: lag * (1000 / rate) need not round them alike
    coef = rng.uniform(0.8, 1.0, batch)
    coef[::7] = np.nan
    ret = np.where(np.isnan(coef), -1, rng.integers(0, 2, batch) * -2).astype(np.int32)
    got = []
    for poisoned in (False, True):
        ins = [rows_in_poison(torch, lag, 10 ** 9, poisoned), rows_in_poison(torch, coef, 2.0, poisoned), rows_in_poison(torch, ret, 0, poisoned)]
        before = [edges.snapshot(b) for b, _ in ins]
        ms, ms_view = edges.guarded(torch, "int64", batch)
        ok, ok_view = edges.guarded(torch, "int32", batch)
        torch.cuda.synchronize()
        mod.results_to_ms_dev(ins[0][1], ins[1][1], ins[2][1], batch, ms_view.data_ptr(), ok_view.data_ptr(), 0.95, 48000.0)
        torch.cuda.synchronize()
        assert edges.check_guards(ms, batch) == [] and edges.check_guards(ok, batch) == []
        assert all(edges.unchanged(b, was) for (b, _), was in zip(ins, before))
        got.append((ms_view.cpu().numpy(), ok_view.cpu().numpy()))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert got[0][0].tolist() == c_round(lag * 1000.0 / 48000.0).tolist()
    assert got[0][1].tolist() == ((ret == 0) & (coef >= 0.95)).astype(np.int32).tolist()


@pytest.mark.parametrize("batch", [1, 255, 256, 257])
def test_topk_best(mod, torch, batch):
    k = 3
    rng = np.random.default_rng(1000 + batch)
    lag = rng.integers(-1000, 1000, batch * k).astype(np.int64)
    coef = rng.uniform(-1.0, 1.0, batch * k)
    coef[::5] = np.nan
    ret = np.where(np.isnan(coef), -1, np.where(rng.uniform(size=batch * k) < 0.2, -3, 0)).astype(np.int32)
    ret[:k] = -3                                                    # pair 0: no entry with ret == 0
    got = []
    for poisoned in (False, True):
        ins = [rows_in_poison(torch, lag, 10 ** 9, poisoned), rows_in_poison(torch, coef, 2.0, poisoned), rows_in_poison(torch, ret, 0, poisoned)]
        before = [edges.snapshot(b) for b, _ in ins]
        outs = [edges.guarded(torch, t, batch) for t in ("float64", "int32", "int64", "int32")]
        torch.cuda.synchronize()
        mod.topk_best_dev(ins[0][1], ins[1][1], ins[2][1], batch, k, *(v.data_ptr() for _, v in outs))
        torch.cuda.synchronize()
        assert all(edges.check_guards(w, batch) == [] for w, _ in outs)
        assert all(edges.unchanged(b, was) for (b, _), was in zip(ins, before))
        got.append([v.cpu().numpy() for _, v in outs])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*got))
    best_coef, best_ret, best_lag, best_entry = got[0]
    for i in range(batch):                                          # the header's rule
        ok = [j for j in range(k) if ret[i * k + j] == 0]
        j = max(ok, key=lambda j: (coef[i * k + j], -j)) if ok else 0
        assert (int(best_entry[i]), int(best_lag[i]), int(best_ret[i])) == (j, int(lag[i * k + j]), int(ret[i * k + j])), i
        assert best_coef[i].tobytes() == coef[i * k + j].tobytes(), i


@pytest.mark.parametrize("n", [999, 1000])
def test_synth_pairs(mod, torch, n):
    count = 3
    plain = [torch.full((count * 2 * n,), 7.0, dtype=torch.float32, device="cuda"), torch.full((count * n,), 7.0, dtype=torch.float32, device="cuda"),
             torch.full((count,), 7, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    mod.synth_pairs_dev(2024, 5, count, n, 1, *(a.data_ptr() for a in plain))
    held = [edges.guarded(torch, t, c) for t, c in (("float32", count * 2 * n), ("float32", count * n), ("int64", count))]
    torch.cuda.synchronize()
    mod.synth_pairs_dev(2024, 5, count, n, 1, *(v.data_ptr() for _, v in held))
    torch.cuda.synchronize()
    for (w, v), a, c in zip(held, plain, (count * 2 * n, count * n, count)):
        assert edges.check_guards(w, c) == []
        assert v.cpu().numpy().tobytes() == a.cpu().numpy().tobytes()
    for i in range(count):                                          # ... and it is the oracle's generator
        s, t, l = oracle.synth_pair(2024, 5 + i, n, 1)
        assert plain[0].cpu().numpy()[i * 2 * n:(i + 1) * 2 * n].tobytes() == s.tobytes() and int(plain[2][i]) == l
