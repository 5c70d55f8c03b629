"""Integer-valued inputs and an exact reference for the float64 tables behind the normalised cross-correlation (csrc/ncc.hip): the
per-lag table {Sx', Vx} of k_ncc_table, the track's Vmax, Sy and Vy of the sample, the prefix table {P1, Vx} and the suffix table
{T1, Vy[l]} of k_nccfull_prefix, as Plan.debug_ncc_tables returns them.

Every input value is an integer of magnitude at most 2^15, so its float32 is exact, every sum of the reference is an exact integer
and every variance an exact rational n Sxx - Sx^2 over n, rounded once.  The tables can therefore be held to the reference at the
rounding error of float64 instead of the float32 error of r32 under which the curve tests see them.  compare() states the
assertions once: tests/test_gpu_ncc_tables.py applies them to the device's tables, tests/test_ncc_exact.py to a float64 restatement
and to deliberately wrong references.  Plain module: numpy and Python integers, no fixtures, nothing happens on import."""
import numpy as np

KINDS = "ABCDE"
SAMPLE_KIND = {"A": "A", "B": "B", "C": "A", "D": "A", "E": "E"}   # the sample that goes with a source of each kind
OFFSET = 20000      # input B
STEP = 16000        # input C
FADE = 1e-4         # input E: the envelope falls to this over N frames
LIMIT = 1 << 15

# The competing-set tests (GPU) and the margin test that makes them sound (CPU) run over the same cases.
ENERGIES = (1e-6, 1e-3, 0.5, 1.0)
COMPETE_KINDS = "DE"
COMPETE_LENGTHS = (2049, 5000, 144000)
MARGIN = 1e-9       # no lag's exact energy lies within this relative distance of the threshold
# (kind, n) -> seed, where the default seed puts a lag within MARGIN of a threshold (tests/test_ncc_exact.py says so)
SEEDS = {}
DEFAULT_SEED = 1


def overlaps(n):
    """the min_overlap values of the full-range competing-set tests"""
    return (1, max(1, n // 2))


def _signed(rng, lo, hi, size):
    """integers of magnitude lo..hi with a random sign"""
    return rng.integers(lo, hi + 1, size) * rng.choice(np.array([-1, 1]), size)


def step_at(n, prefix):
    """input C: the first frame of the upper level"""
    return (6 * n) // 10 if prefix else (12 * n) // 10


def zero_run(n, prefix):
    """input D: (first frame, frames) of the silent stretch"""
    return (0, n // 3) if prefix else (n // 3, n + max(1, n // 8))


def track(kind, frames, n, seed, prefix=False):
    """-> int64 [frames] (2N for a source, N for a sample) of one of the five inputs at sample length n.
    A "pcm": magnitudes uniform in [3000, 12000], random sign -- no small values, so one wrong frame moves a sum by at least 3000 and
       a window's sum of squares by at least 9e6.
    B "offset": 20000 + d, 10 <= |d| <= 50 -- mu removes the 20000 and leaves deviations 400 times smaller.
    C "step": d with 100 <= |d| <= 300, plus 16000 from frame 1.2 N on (prefix: 0.6 N, inside the first N frames) -- a window inside
       one level cancels about three digits of s2 - s1^2 / N.
    D "silence": A with more than N consecutive zeros from frame N / 3 on (prefix: A with its first N / 3 frames zero) -- an exact
       Vx = 0 over a stretch.
    E "fade": A times a geometric envelope that falls from 1 to 1e-4 over N frames, rounded to integers.  A sample is N frames,
       so that is the whole track; a source goes on falling at the same rate over its second half, so the window of lag l holds about
       10^(-8 l / N) of the first window's energy: Vx / Vmax passes every min_energy from 1 down to below 1e-6 (a fade to 1e-4 over
       all 2N frames would stop at 1e-4, above the smallest threshold)."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n, frames])
    if kind == "B":
        x = OFFSET + _signed(rng, 10, 50, frames)
    elif kind == "C":
        x = _signed(rng, 100, 300, frames)
        x[step_at(n, prefix):] += STEP
    else:
        x = _signed(rng, 3000, 12000, frames)
        if kind == "D":
            at, run = zero_run(n, prefix)
            x[at:at + run] = 0
        elif kind == "E":
            x = np.rint(x * FADE ** (np.arange(frames) / n)).astype(np.int64)
    x = x.astype(np.int64)
    assert np.abs(x).max() <= LIMIT
    return x


def pair(kind, n, prefix=False, seed=None):
    """-> (source int64 [2N], sample int64 [N]) of input `kind`; prefix: the variant for the full-range tables"""
    seed = SEEDS.get((kind, n), DEFAULT_SEED) if seed is None else seed
    return track(kind, 2 * n, n, seed, prefix), track(SAMPLE_KIND[kind], n, n, seed + 1000 * (1 + KINDS.index(kind)))


def f32(x):
    """the float32 track of an integer one: exact"""
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.int64), x)
    return y


def _ratio(num, den):
    """num / den of two exact integers as one correctly rounded float64"""
    return int(num) / int(den)


def _variance(s1, s2, count):
    """(count s2 - s1^2) / count per element, the numerator an exact Python integer and the division rounded once.  s1, s2: int64
    arrays (sums and sums of squares: both fit), count: an integer or an integer array"""
    c = np.asarray(count).astype(object)
    num = c * s2.astype(object) - s1.astype(object) ** 2
    return (num / c).astype(np.float64)


def exact(src, smp, full=False):
    """The reference of one pair (int64 tracks of 2N and N frames) -> a dict:
    mu, mean_y   the means, rounded once
    Sx [N] int64, Vx [N], S2 [N]   of every window [l, l + N): the exact sum, the variance sum, and the scale sum (x - mu)^2
    Sy, Vy, S2y  of the sample (about its own mean)
    full: P [N] int64, Vxp [N], S2p [N] of the source's prefixes x[0, m) and T [N], Vyp [N], S2t [N] of the sample's suffixes
    y[N - m, N), at index m = 1..N-1 (index 0: 0, NaN, NaN).
    The scales are plain float64: they only scale an error."""
    n = smp.size
    assert src.size == 2 * n and src.dtype == smp.dtype == np.int64
    e1 = np.concatenate([[0], np.cumsum(src)])
    e2 = np.concatenate([[0], np.cumsum(src * src)])
    sx, sxx = e1[n:2 * n] - e1[:n], e2[n:2 * n] - e2[:n]
    out = {"n": n, "mu": _ratio(e1[-1], 2 * n), "mean_y": _ratio(smp.sum(), n), "Sx": sx, "Vx": _variance(sx, sxx, n),
           "Sy": int(smp.sum()), "Vy": float(_variance(np.array([smp.sum()]), np.array([(smp * smp).sum()]), n)[0])}
    a, b = src - out["mu"], smp - out["mean_y"]
    f2 = np.concatenate([[0.0], np.cumsum(a * a)])
    out["S2"] = f2[n:2 * n] - f2[:n]
    out["S2y"] = float((b * b).sum())
    if full:
        m = np.arange(n)
        m[0] = 1    # (index 0 is nobody's: kept out of the division)
        rs, rss = np.concatenate([[0], np.cumsum(smp[::-1])]), np.concatenate([[0], np.cumsum((smp * smp)[::-1])])
        for key, s1, s2, scale in (("P", "Vxp", "S2p"), e1[:n], e2[:n], f2[:n]), \
                                  (("T", "Vyp", "S2t"), rs[:n], rss[:n], np.concatenate([[0.0], np.cumsum((b * b)[::-1])])[:n]):
            v = _variance(s1, s2, m)
            v[0] = np.nan
            scale = scale.copy()
            scale[0] = np.nan
            out[key[0]], out[key[1]], out[key[2]] = s1, v, scale
    return out


def float64_tables(src, smp, full=False):
    """The kernels' formulas in numpy float64 with sequential sums, in the shape of Plan.debug_ncc_tables: what a correct device
    returns up to the order of its sums.  It stands in for the device where the assertions are tried on the CPU."""
    n = smp.size
    x, y = src.astype(np.float64), smp.astype(np.float64)
    mu, my = x.sum() / (2 * n), y.sum() / n
    a, b = x - mu, y - my
    e1, e2 = np.concatenate([[0.0], np.cumsum(a)]), np.concatenate([[0.0], np.cumsum(a * a)])
    s1, s2 = e1[n:2 * n] - e1[:n], e2[n:2 * n] - e2[:n]
    vx = s2 - s1 * s1 / n
    out = {"mu": float(mu), "vmax": float(max(0.0, np.nanmax(vx))), "mean_y": float(my), "sy": float(b.sum() + n * my),
           "vy": float((b * b).sum() - b.sum() ** 2 / n), "table": np.stack([s1, vx], axis=1)}
    if full:
        m = np.arange(n, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            for key, d in (("ptab", a[:n]), ("ttab", b[::-1])):
                t1, t2 = np.concatenate([[0.0], np.cumsum(d)])[:n], np.concatenate([[0.0], np.cumsum(d * d)])[:n]
                out[key] = np.stack([t1, t2 - t1 * t1 / m], axis=1)
                out[key][0] = np.nan
    return out


def compare(dev, ex, relative=False):
    """The assertions on one pair's tables.  dev: Plan.debug_ncc_tables' dict (with ptab and ttab where ex holds the full-range
    entries), ex: exact()'s.  Asserted here, because they are exact: the means (an exact integer sum and one division); every sum
    -- the true sums are integers, float64 holds the mu-shifted ones within 1e-5 of them at these sizes, and a wrong frame moves a sum
    by at least 10 in every input --; Vmax as the maximum, NaN ignored, of the Vx returned.  Returned for the caller to hold to its
    tolerance, {name: figure}:
    vx      max |Vx_dev[l] - Vx[l]| over max S2[l]           vy      |Vy_dev - Vy| / S2y
    vmax    |Vmax_dev - max Vx| / max Vx                     vx_rel  relative: max |Vx_dev[l] - Vx[l]| / Vx[l] over the lags with Vx > 0
    ptab, ttab   max over m = 1..N-1 of |V_dev[m] - V[m]| / S2[m] (sums of positive terms only)
    A NaN in a device table makes its figure NaN, which no tolerance admits."""
    n = ex["n"]
    assert dev["table"].shape == (n, 2)
    assert dev["mu"] == ex["mu"] and dev["mean_y"] == ex["mean_y"], (dev["mu"], ex["mu"], dev["mean_y"], ex["mean_y"])

    def sums(name, shifted, count, mean, want):
        got = np.rint(shifted + count * mean)
        bad = np.flatnonzero(~(got == want))
        assert bad.size == 0, (name, "sums differ at", bad[:8], got[bad[:8]], want[bad[:8]])

    sx, vx = dev["table"][:, 0], dev["table"][:, 1]
    sums("Sx", sx, n, dev["mu"], ex["Sx"])
    assert np.rint(dev["sy"]) == ex["Sy"], (dev["sy"], ex["Sy"])
    top = max(0.0, float(np.nanmax(vx))) if not np.isnan(vx).all() else 0.0
    assert dev["vmax"] == top, ("Vmax is not the maximum of the Vx returned", dev["vmax"], top)
    fig = {"vx": float(np.max(np.abs(vx - ex["Vx"])) / np.max(ex["S2"])),
           "vy": abs(dev["vy"] - ex["Vy"]) / ex["S2y"] if ex["S2y"] > 0 else abs(dev["vy"]),
           "vmax": float(abs(dev["vmax"] - ex["Vx"].max()) / ex["Vx"].max()) if ex["Vx"].max() > 0 else abs(dev["vmax"])}
    if relative:
        pos = ex["Vx"] > 0
        fig["vx_rel"] = float(np.max(np.abs(vx[pos] - ex["Vx"][pos]) / ex["Vx"][pos])) if pos.any() else 0.0
    if "P" in ex and n > 1:
        m = np.arange(1, n)
        for name, mean, s, v, scale in (("ptab", dev["mu"], "P", "Vxp", "S2p"), ("ttab", dev["mean_y"], "T", "Vyp", "S2t")):
            tab = dev[name]
            assert tab.shape == (n, 2)
            sums(name, tab[1:, 0], m, mean, ex[s][1:])
            err, sc = np.abs(tab[1:, 1] - ex[v][1:]), ex[scale][1:]
            # (a scale of exactly 0: every frame equals the mean, and the variance sum must be 0 too)
            fig[name] = float(np.max(np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), err)))
    return fig


def threshold_gap(ex, min_energy):
    """How close the exact energies come to the competing rules' thresholds, relative to the threshold: (the lags 0..N-1 against
    min_energy Vmax, the overlaps 1..N-1 against min_energy Vmax Vy -- NaN unless ex is full).  At min_energy = 1 the window that
    holds Vmax meets its threshold exactly and is left out: it has to be the only one."""
    vmax = ex["Vx"].max()
    thr = min_energy * vmax
    d = np.abs(ex["Vx"] - thr) / thr
    if min_energy == 1.0:
        assert np.count_nonzero(ex["Vx"] == vmax) == 1
        d = np.delete(d, int(np.argmax(ex["Vx"])))
    lo = float("nan")
    if "P" in ex and ex["n"] > 1:
        thr2 = thr * ex["Vy"]
        lo = float(np.min(np.abs(ex["Vxp"][1:] * ex["Vyp"][1:] - thr2) / thr2))
    return (float(d.min()) if d.size else float("inf")), lo


def competing(ex, min_energy):
    """the exact rule for the lags 0..N-1: Vy > 0 and Vx[l] >= min_energy Vmax (c is finite wherever that holds)"""
    return (ex["Vy"] > 0) & (ex["Vx"] >= min_energy * ex["Vx"].max())


def competing_low(ex, min_energy, min_overlap):
    """the exact rule for the lags -(N-1)..-1, index m - 1 = l + N - 1: m >= min_overlap, Vy > 0, Vx[l] Vy[l] >= min_energy Vmax Vy"""
    m = np.arange(1, ex["n"])
    return (m >= min_overlap) & (ex["Vy"] > 0) & (ex["Vxp"][1:] * ex["Vyp"][1:] >= min_energy * ex["Vx"].max() * ex["Vy"])
