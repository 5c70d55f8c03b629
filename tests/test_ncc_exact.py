"""The exact reference of tests/ncc_exact.py on the CPU: it agrees with the float64 models' moments, its inputs keep their rules, no
lag of a competing-set case sits at a threshold, the assertions of compare() pass on a float64 restatement of the kernels and fail
by orders of magnitude on deliberately wrong references, and the diagnostic that returns the tables stays outside the ABI."""
import os

import numpy as np
import pytest

import ncc_exact as ex
import ncc_full_model
import ncc_model
from util import ROOT, asx

CAP = 1e-9   # the hard cap of tests/test_gpu_ncc_tables.py's TABLE_TOL


@pytest.mark.parametrize("n", [16, 1000, 2049])
@pytest.mark.parametrize("kind", ex.KINDS)
def test_the_reference_agrees_with_the_models(kind, n):
    """within 1e-9 relative: the sliding table of the models' scale, the loudest window's (their cumulative sums run over the whole
    track, so a quiet window of input E carries the loud ones' rounding), the prefix and suffix sums -- positive terms only -- of
    the value itself (of the scale sum where the exact variance is 0: input D's silent frames)"""
    for prefix in (False, True):
        src, smp = ex.pair(kind, n, prefix)
        e = ex.exact(src, smp, full=True)
        mu, sx, vx, sy, vy = ncc_model.moments(ex.f32(src), ex.f32(smp))
        assert abs(mu - e["mu"]) <= 1e-9 * max(1.0, abs(e["mu"]))
        assert np.all(np.abs(sx - e["Sx"]) <= 1e-9 * np.maximum(n * abs(mu), np.abs(e["Sx"])))   # (a silent window: N mu - N mu)
        assert np.all(np.abs(vx - e["Vx"]) <= 1e-9 * e["S2"].max())
        assert abs(sy - e["Sy"]) <= 1e-9 * max(1.0, abs(e["Sy"])) and abs(vy - e["Vy"]) <= 1e-9 * e["Vy"]
        c, energy, vmax, vy2, vx2 = ncc_full_model.curve(ex.f32(src), ex.f32(smp))
        assert abs(vmax - e["Vx"].max()) <= 1e-9 * vmax and abs(vy2 - e["Vy"]) <= 1e-9 * vy2
        want = e["Vxp"][1:] * e["Vyp"][1:]
        assert np.all(np.abs(energy[:n - 1] - want) <= 1e-9 * np.where(want > 0, want, e["S2p"][1:] * e["S2t"][1:]))
        assert np.all(np.abs(energy[n - 1:] - e["Vx"] * e["Vy"]) <= 1e-9 * e["S2"].max() * e["Vy"])


@pytest.mark.parametrize("n", [1, 2, 3, 16, 1023, 2049, 5000])
def test_the_inputs_keep_their_rules(n):
    for prefix in (False, True):
        for kind in ex.KINDS:
            src, smp = ex.pair(kind, n, prefix)
            assert src.dtype == smp.dtype == np.int64 and src.shape == (2 * n,) and smp.shape == (n,)
            for x in (src, smp):
                assert np.abs(x).max() <= ex.LIMIT and np.array_equal(ex.f32(x).astype(np.float64), x.astype(np.float64))
            assert ex.SAMPLE_KIND[kind] in "ABE"
        a = np.abs(ex.pair("A", n, prefix)[0])
        assert a.min() >= 3000 and a.max() <= 12000
        for x in ex.pair("B", n, prefix):
            d = np.abs(x - ex.OFFSET)
            assert d.min() >= 10 and d.max() <= 50
        c = ex.pair("C", n, prefix)[0]
        d = np.abs(c - ex.STEP * (np.arange(2 * n) >= ex.step_at(n, prefix)))
        assert d.min() >= 100 and d.max() <= 300
        assert ex.step_at(n, prefix) < n if prefix else n <= ex.step_at(n, prefix) < 2 * n
        d_src = ex.pair("D", n, prefix)[0]
        at, run = ex.zero_run(n, prefix)
        assert not d_src[at:at + run].any() and at + run <= 2 * n and np.count_nonzero(d_src) == 2 * n - run
        assert run > n and at == n // 3 if not prefix else (at, run) == (0, n // 3)
    if n >= 1000:
        # D: an exact Vx = 0 over a stretch; E: Vx / Vmax from 1 down to below the smallest min_energy, the sample faded to 1e-4
        e = ex.exact(*ex.pair("D", n))
        assert np.count_nonzero(e["Vx"] == 0.0) == max(1, n // 8) + 1
        src, smp = ex.pair("E", n)
        e = ex.exact(src, smp)
        ratio = e["Vx"] / e["Vx"].max()
        assert ratio.max() == 1.0 and ratio.min() < ex.ENERGIES[0] and np.all(ratio[1:] < ratio[:-1] * 1.05)
        assert 0.5 * ex.FADE * 3000 <= np.abs(smp[-50:]).max() <= 2 * ex.FADE * 12000


_cases = {}


def case(kind, n):
    """the competing-set case (kind, n): the exact reference of its full-range variant and of its plain one"""
    if (kind, n) not in _cases:
        _cases[kind, n] = tuple(ex.exact(*ex.pair(kind, n, prefix), full=prefix) for prefix in (False, True))
    return _cases[kind, n]


@pytest.mark.parametrize("n", ex.COMPETE_LENGTHS)
@pytest.mark.parametrize("kind", ex.COMPETE_KINDS)
def test_no_lag_sits_at_a_threshold(kind, n):
    """For every (input, min_energy) of the GPU tests no lag's exact energy lies within a relative 1e-9 of its threshold, so a device
    whose tables are within TABLE_TOL <= 1e-9 must return the exact competing set: no lag is left out.  A seed that puts a lag
    there is replaced in ncc_exact.SEEDS."""
    plain, full = case(kind, n)
    for me in ex.ENERGIES:
        hi, _ = ex.threshold_gap(plain, me)
        hi2, lo = ex.threshold_gap(full, me)
        print("threshold gap", kind, n, me, "sliding", hi, "full-range l >= 0", hi2, "l < 0", lo)
        assert min(hi, hi2, lo) > ex.MARGIN, (kind, n, me, hi, hi2, lo)
        # ... and the case tests something: lags on both sides of the rule (at 1e-6 input D's silent windows are the ones left out)
        ok = ex.competing(plain, me)
        assert ok.any() and not ok.all(), (kind, n, me)
        assert me < 1.0 or ok.sum() == 1
        for mo in ex.overlaps(n):
            low = ex.competing_low(full, me, mo)
            assert not low.all(), (kind, n, me, mo)
    assert ex.competing_low(full, ex.ENERGIES[0], 1).any() and ex.competing_low(full, ex.ENERGIES[1], n // 2).any()


def wrong_window(e):
    """the reference of windows placed one frame late"""
    w = dict(e)
    for key in ("Sx", "Vx"):
        w[key] = np.roll(e[key], -1)
    return w


def wrong_variance(e, src, smp):
    """the reference without the - Sx^2 / n term: the plain sums of squares"""
    n = e["n"]
    e2 = np.concatenate([[0], np.cumsum(src * src)])
    w = dict(e)
    w["Vx"] = (e2[n:2 * n] - e2[:n]).astype(np.float64)
    w["Vy"] = float((smp * smp).sum())
    if "P" in e:
        w["Vxp"] = np.concatenate([[np.nan], e2[1:n].astype(np.float64)])
        w["Vyp"] = np.concatenate([[np.nan], np.cumsum((smp * smp)[::-1])[:n - 1].astype(np.float64)])
    return w


@pytest.mark.parametrize("n", [3, 1025, 5000])
@pytest.mark.parametrize("kind", ex.KINDS)
def test_the_assertions_pass_on_a_restatement_and_fail_on_wrong_references(kind, n):
    src, smp = ex.pair(kind, n, prefix=True)
    e = ex.exact(src, smp, full=True)
    dev = ex.float64_tables(ex.f32(src), ex.f32(smp), full=True)
    fig = ex.compare(dev, e, relative=kind in "AB")
    print("restatement", kind, n, fig)
    assert all(v <= CAP for v in fig.values()), fig
    # a window one frame late: the sums differ (a wrong frame moves a sum by at least 10 in A, B and C; D and E hold zeros)
    if kind in "ABC":
        with pytest.raises(AssertionError, match="sums differ"):
            ex.compare(dev, wrong_window(e))
    # ... and past the sums, the variances differ by far more than the cap (input C is there for the cancellation: its single
    # frames are not pinned; input E's loud windows are, its quiet ones not)
    if kind in "AD" and n >= 1025:
        late = dict(dev, table=np.roll(dev["table"], -1, axis=0))
        late["table"][:, 0] = dev["table"][:, 0]
        late["vmax"] = max(0.0, float(late["table"][:, 1].max()))
        assert ex.compare(late, e)["vx"] >= 100 * CAP
    # one frame dropped from every prefix and suffix
    short = dict(dev, ptab=np.concatenate([dev["ptab"][:1], dev["ptab"][:-1]]), ttab=np.concatenate([dev["ttab"][:1], dev["ttab"][:-1]]))
    with pytest.raises(AssertionError, match="sums differ"):
        ex.compare(short, e)
    # the - Sx^2 / n term dropped
    w = ex.compare(dev, wrong_variance(e, src, smp), relative=True)
    print("without - Sx^2 / n", kind, n, w)
    # (the term is Sx'^2 / n on top of n mean^2: about 1 / n of the scale where the mean is 0, as in a sample of kind A -- the share
    # a test can see there depends on the draw, so Vy and the suffix table are held to it where the tracks carry an offset)
    assert w["vx"] >= 100 * CAP and w["vmax"] >= 100 * CAP and w["vx_rel"] >= 100 * CAP and w["ptab"] >= 100 * CAP, w
    if kind == "B":
        assert min(w.values()) >= 0.5, w
    # a stale Vmax (the maximum of another call's table), a wrong mean, a wrong Sy
    for key, value in (("vmax", dev["vmax"] * 4.0), ("mu", np.nextafter(dev["mu"], np.inf)), ("sy", dev["sy"] + 10.0)):
        with pytest.raises(AssertionError):
            ex.compare(dict(dev, **{key: value}), e)


def test_the_diagnostic_is_outside_the_abi():
    mod = asx()
    from audiosync_amd import hipxcorr
    name = "asx_plan_debug_ncc_tables"
    hdr = open(os.path.join(ROOT, "include", "audiosync", "xcorr_hip.h")).read()
    assert hasattr(mod.lib(), name) and name in hipxcorr.SIGNATURES
    assert name not in hipxcorr.ABI_SYMBOLS and name not in hdr
    assert set(mod.Plan.NCC_TABLE_SETS) == {"strided", "pool", "full"}
