"""Top-k GCC-PHAT on the MI355X (asx_xcorr_phat_topk_f32_dev, Plan.xcorr_phat_topk_f32) against the float64 model of
tests/phat_topk_model.py and against the calls it extends: k = 1 and entry 0 are the banded PHAT call, bit for bit; the multipath
pair's five paths in order; zones, exhaustion, invalid rows; the signed seed; a silent pair; broadcast, strides and lanes; the state
the call shares with its neighbours; refusals.  Entries are compared with the model only where the model's margin is far above the
float32 resolution, and the margins are asserted here."""
import numpy as np
import pytest

import oracle
import phat_band_model
import phat_topk_model
from test_phat_topk import MIN_GAP, SEEDS, SEP, multipath
from util import asx

pytestmark = pytest.mark.gpu

N = 144000
COEF_TOL = 1e-5
# the peak height against the float64 model: what tests/test_gpu_phat.py asserts with every bin voting (CURVE_TOL there) and
# tests/test_gpu_phat_band.py under a band
PEAK_TOL = {"full": 2e-7, "band": 3e-6}
BANDS = {"full": (0, N), "band": (1, N // 6)}
SYNTH_SEED = 77

_pairs = {}


def synth(k, n=N):
    if (n, k) not in _pairs:
        _pairs[n, k] = oracle.synth_pair(SYNTH_SEED, k, n, (3, 0)[k % 2])
    return _pairs[n, k]


def stacked(ks):
    return np.stack([synth(k)[0] for k in ks]), np.stack([synth(k)[1] for k in ks])


def all_bits(out):
    return [np.ascontiguousarray(a).tobytes() for a in out]


def pair_bits(out, p):
    return [np.ascontiguousarray(np.asarray(a)[p]).tobytes() for a in out]


def check_against_model(got, p, want, gaps, tol, what):
    """pair p of `got` (lag, coef, peak, ret of shape [B, k]) against the model's entries, each of which must stand MIN_GAP clear"""
    for j, ((ret, lag, coef, peak), gap) in enumerate(zip(want, gaps)):
        g = tuple(a[p][j] for a in got)
        print("phat top-k", what, "pair", p, "entry", j, "gpu", g, "model", (lag, coef, peak, ret), "margin", gap)
        if ret == -3:
            assert (int(g[0]), int(g[3])) == (0, -3) and np.isnan(g[1]) and np.isnan(g[2]), (what, p, j, g)
            continue
        assert gap >= MIN_GAP, (what, p, j, gap)
        assert (int(g[0]), int(g[3])) == (lag, ret), (what, p, j, g, want[j])
        assert abs(float(g[2]) - peak) <= tol, (what, p, j, g, want[j])
        if ret == 0:
            assert abs(float(g[1]) - coef) < COEF_TOL, (what, p, j, g, want[j])
        else:
            assert np.isnan(g[1]), (what, p, j, g)


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


def outputs(torch, b):
    return (torch.full((b,), -99, dtype=torch.int64, device="cuda"), torch.full((b,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((b,), 7.0, dtype=torch.float64, device="cuda"), torch.full((b,), 7, dtype=torch.int32, device="cuda"))


def untouched(torch, out):
    torch.cuda.synchronize()
    b = out[0].numel()
    return [a.cpu().tolist() for a in out] == [[-99] * b, [7.0] * b, [7.0] * b, [7] * b]


@pytest.mark.parametrize("band", sorted(BANDS))
def test_k1_is_the_banded_call_and_entry_0_at_k4(mod, band):
    """five pairs on a plan of max_batch 2 (three launch groups), per-pair rows (one of them not a window) and the plan's window: all
    four outputs of k = 1, and entry 0 of k = 4, are the bits of asx_xcorr_phat_band_f32_dev"""
    lo, hi = BANDS[band]
    src, smp = stacked(range(5))
    rows = np.array([(-N, N - 1), (-N // 3, -5), (7, 6), (100, 5000), (-N, -N)], dtype=np.int64)
    with mod.Plan(N, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        for windows in (None, rows):
            want = plan.xcorr_phat_f32(src, smp, windows, band=(lo, hi))
            one = plan.xcorr_phat_topk_f32(src, smp, 1, 500, windows, (lo, hi))
            assert one[0].shape == (5, 1) and all_bits(one) == all_bits(want), (band, windows is None)
            four = plan.xcorr_phat_topk_f32(src, smp, 4, 500, windows, (lo, hi))
            assert all_bits([a[:, 0] for a in four]) == all_bits(want), (band, windows is None)
        plan.set_lag_window(-3000, 40000)
        want = plan.xcorr_phat_f32(src, smp, band=(lo, hi))
        assert all_bits(plan.xcorr_phat_topk_f32(src, smp, 1, 0, band=(lo, hi))) == all_bits(want)
        assert all_bits([a[:, 0] for a in plan.xcorr_phat_topk_f32(src, smp, 3, 9, band=(lo, hi))]) == all_bits(want)
        assert plan.lag_window == (-3000, 40000)


@pytest.mark.parametrize("band", sorted(BANDS))
def test_multipath_against_the_model(mod, band):
    """the three multipath pairs in one batch over two launch groups, k = 5: the planted paths in order, peaks and coefficients
    within tolerance; under set_pearson(0) every entry's coefficient is the windowed call's at the row [lag, lag], bit for bit"""
    cases = [multipath(seed, BANDS[band]) for seed in SEEDS]
    src, smp = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    with mod.Plan(N, 2, 0) as plan:
        got = plan.xcorr_phat_topk_f32(src, smp, 5, SEP, band=BANDS[band])
        for p, (_, _, _, five, gaps, _) in enumerate(cases):
            check_against_model(got, p, five, gaps, PEAK_TOL[band], "multipath " + band)
            assert got[0][p].tolist() == list(phat_topk_model.MULTIPATH_LAGS)
        plan.set_pearson(False)
        direct = plan.xcorr_phat_topk_f32(src, smp, 5, SEP, band=BANDS[band])
        assert all_bits(direct) == all_bits(got)                      # the direct form whatever the plan's setting
        rows = np.stack([direct[0].ravel(), direct[0].ravel()], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(np.repeat(src, 5, axis=0), np.repeat(smp, 5, axis=0), rows)
        assert lag.tolist() == direct[0].ravel().tolist() and ret.tolist() == direct[3].ravel().tolist()
        assert coef.tobytes() == np.ascontiguousarray(direct[1]).tobytes(), (coef, direct[1])


def test_multipath_at_the_longest_length(mod):
    """N = 1 440 000 (600-row columns, two-half rows: other instances of the inverse pass), two pairs, three paths, k = 3"""
    n = 1440000
    lags, gains = phat_topk_model.MULTIPATH_LAGS[:3], phat_topk_model.MULTIPATH_GAINS[:3]
    pairs = [phat_topk_model.multipath_pair(seed, n, lags, gains) for seed in SEEDS[:2]]
    src, smp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with mod.Plan(n, 1, 0) as plan:
        assert plan.layout == "real-column"
        plan.set_pearson(False)
        got = plan.xcorr_phat_topk_f32(src, smp, 3, SEP)
        for p, (s, t) in enumerate(pairs):
            r = phat_band_model.r_phat_band(s, t, 0, n)
            want = phat_topk_model.model(s, t, 0, n, 3, SEP, r=r)
            check_against_model(got, p, want, phat_topk_model.margins(r, n, want, SEP), PEAK_TOL["full"], "longest")
            assert [e[1] for e in want] == list(lags)
        rows = np.stack([got[0].ravel(), got[0].ravel()], axis=1)
        lag, coef, ret = plan.xcorr_windowed_f32(np.repeat(src, 3, axis=0), np.repeat(smp, 3, axis=0), rows)
        assert coef.tobytes() == np.ascontiguousarray(got[1]).tobytes() and ret.tolist() == got[3].ravel().tolist()


def test_zones_and_exhaustion(mod):
    band = BANDS["band"]
    src, smp, r, five, _, _ = multipath(1, band)
    src2, smp2 = np.stack([src, src, src]), np.stack([smp, smp, smp])
    with mod.Plan(N, 2, 0) as plan:
        # min_separation = 0: under a band of N/6 bins the peak is several lags wide, so its neighbours come next in the model
        got = plan.xcorr_phat_topk_f32(src, smp, 3, 0, band=band)
        want = phat_topk_model.model(src, smp, *band, 3, 0, r=r)
        assert sorted(e[1] for e in want) == [1199, 1200, 1201], want
        check_against_model(got, 0, want, phat_topk_model.margins(r, N, want, 0), PEAK_TOL["band"], "neighbours")
        # min_separation >= 2N: one zone takes every lag
        for sep in (2 * N, 2 ** 40):
            got = plan.xcorr_phat_topk_f32(src, smp, 3, sep, band=band)
            assert all_bits([a[:, 0] for a in got]) == all_bits(plan.xcorr_phat_f32(src, smp, band=band))
            for j in (1, 2):
                assert (int(got[0][0][j]), int(got[3][0][j])) == (0, -3) and np.isnan(got[1][0][j]) and np.isnan(got[2][0][j]), got
        # a row of five lags that begins at the strongest path, zones of 129: the peak, the one lag left, then nothing; beside it an
        # invalid row, and a pair with the plan's full row
        rows = np.array([(1200, 1204), (9, 8), (-N, N - 1)], dtype=np.int64)
        got = plan.xcorr_phat_topk_f32(src2, smp2, 4, 3, rows, band)
        want = phat_topk_model.model(src, smp, *band, 4, 3, 1200, 1204, r=r)
        assert [e[0] for e in want] == [0, 0, -3, -3] and [e[1] for e in want[:2]] == [1200, 1204], want
        check_against_model(got, 0, want, phat_topk_model.margins(r, N, want, 3, 1200, 1204), PEAK_TOL["band"], "exhausted")
        for j in range(4):
            assert (int(got[0][1][j]), int(got[3][1][j])) == (0, -2) and np.isnan(got[1][1][j]) and np.isnan(got[2][1][j]), got
        valid = rows.copy()
        valid[1] = (-N, N - 1)
        ref = plan.xcorr_phat_topk_f32(src2, smp2, 4, 3, valid, band)
        assert pair_bits(got, 0) == pair_bits(ref, 0) and pair_bits(got, 2) == pair_bits(ref, 2) == pair_bits(ref, 1)


def signed_seed_cases():
    """-> [(source, sample, (row lo, row hi), min_separation)].  Case 0: the path at lag 5000 has a negative gain and the row begins
    there, so it seeds every pass with a large negative value and loses to any positive one; the strongest path (1200) is outside the
    row.  Case 1: the row begins at the strongest path inside it (5000), and the lag just past its zone (5065) carries the negative
    gain: the seed of passes 2 and 3."""
    a = phat_topk_model.multipath_pair(4, N, (1200, 5000, 31000, 20000, 45000), (1.0, -0.8, 0.65, 0.5, 0.4))
    b = phat_topk_model.multipath_pair(5, N, (1200, 5000, 5065, 31000, 20000), (1.0, 0.9, -0.8, 0.65, 0.5))
    return [a + ((5000, 60000), SEP), b + ((5000, 60000), SEP)]


def test_the_signed_seed(mod):
    cases = signed_seed_cases()
    src, smp = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    rows = np.array([c[2] for c in cases], dtype=np.int64)
    expect = [[31000, 20000, 45000], [5000, 31000, 20000]]
    with mod.Plan(N, 2, 0) as plan:
        got = plan.xcorr_phat_topk_f32(src, smp, 3, SEP, rows)
        for p, (s, t, (lo, hi), sep) in enumerate(cases):
            r = phat_band_model.r_phat_band(s, t, 0, N)
            want = phat_topk_model.model(s, t, 0, N, 3, sep, lo, hi, r=r)
            assert [e[1] for e in want] == expect[p], want
            seed = 5000 if p == 0 else 5065
            assert r[seed] < -0.15 and abs(r[seed]) > want[2][3], (p, r[seed], want)      # the seed would win unsigned
            check_against_model(got, p, want, phat_topk_model.margins(r, N, want, sep, lo, hi), PEAK_TOL["full"], "signed seed")


def test_a_silent_pair(mod):
    """every pass finds an empty maximum: the successive seeds of A_j, peak 0, ret by the NaN coefficient; beside it a pair that is
    not silent keeps its bits"""
    src, smp = stacked(range(2))
    quiet = smp.copy()
    quiet[1] = 0.0
    with mod.Plan(N, 2, 0) as plan:
        base = plan.xcorr_phat_topk_f32(src, smp, 4, 1000)
        got = plan.xcorr_phat_topk_f32(src, quiet, 4, 1000)
        want = phat_topk_model.model(src[1], quiet[1], 0, N, 4, 1000)
        assert [(e[0], e[1], e[3]) for e in want] == [(-1, 0, 0.0), (-1, 1001, 0.0), (-1, 2002, 0.0), (-1, 3003, 0.0)], want
        assert got[0][1].tolist() == [0, 1001, 2002, 3003] and got[2][1].tolist() == [0.0] * 4 and got[3][1].tolist() == [-1] * 4, got
        assert np.isnan(got[1][1]).all()
        assert pair_bits(got, 0) == pair_bits(base, 0)
        rows = np.array([(100, 5000), (-50, 700)], dtype=np.int64)     # the seeds of rows without and with lag 0
        got = plan.xcorr_phat_topk_f32(np.stack([src[1], src[1]]), np.stack([quiet[1], quiet[1]]), 3, 300, rows)
        for p, (lo, hi) in enumerate(rows.tolist()):
            want = phat_topk_model.model(src[1], quiet[1], 0, N, 3, 300, lo, hi)
            assert [(int(got[3][p][j]), int(got[0][p][j])) for j in range(3)] == [(e[0], e[1]) for e in want], (p, got, want)
            assert [float(v) if e[0] != -3 else None for v, e in zip(got[2][p], want)] == [0.0 if e[0] != -3 else None for e in want]
        assert got[0][0].tolist() == [100, 401, 702] and got[0][1].tolist() == [0, 301, 602]


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_position_independence(mod, torch, monkeypatch, lanes):
    """nine pairs over several launch groups, on one and on two lanes; a source stride of 0; strides below the track length: each
    pair's k entries are the bits the call returns for that pair alone"""
    monkeypatch.setenv("ASX_WS_MB", "24")
    monkeypatch.setenv("ASX_LANES", lanes)
    band = BANDS["band"]
    src0, smp0, _, _, _, _ = multipath(1, band)
    smp = np.stack([np.roll(smp0, 37 * p) for p in range(9)])          # the paths of pair p are 37 p frames earlier
    with mod.Plan(N, 9, 0) as plan:
        assert plan.group < 9
        bc = plan.xcorr_phat_topk_f32(src0, smp, 3, SEP, band=band)                     # source stride 0
        full = plan.xcorr_phat_topk_f32(np.stack([src0] * 9), smp, 3, SEP, band=band)
        assert all_bits(bc) == all_bits(full)
        for p in (0, 4, 8):
            alone = plan.xcorr_phat_topk_f32(src0, smp[p], 3, SEP, band=band)
            assert pair_bits(full, p) == pair_bits(alone, 0), p
        hop = 1000                                                                       # windows of one recording
        rec = np.concatenate([src0, src0[:8 * hop]])
        d_rec, d_smp = torch.from_numpy(rec).cuda(), torch.from_numpy(smp[0].copy()).cuda()
        out = outputs(torch, 27)
        torch.cuda.synchronize()
        plan.xcorr_phat_topk_dev(d_rec.data_ptr(), hop, d_smp.data_ptr(), 0, 0, 0, 9, *band, 3, SEP, *(a.data_ptr() for a in out))
        plan.sync()
        wins = np.stack([rec[p * hop:p * hop + 2 * N] for p in range(9)])
        want = plan.xcorr_phat_topk_f32(wins, np.broadcast_to(smp[0], (9, N)), 3, SEP, band=band)
        assert [a.cpu().numpy().tobytes() for a in out] == all_bits(want)
        assert want[0][:, 0].tolist() == [1200 - p * hop for p in range(9)], want[0]


def test_what_the_call_leaves_alone(mod, torch):
    band = BANDS["band"]
    src, smp = stacked(range(5))
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()

    def neighbours(plan):
        out = (torch.zeros(5, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"),
               torch.zeros(5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_strided_dev(d_src.data_ptr(), 2 * N, d_smp.data_ptr(), N, 5, *(a.data_ptr() for a in out))
        plan.sync()
        return ([a.cpu().numpy().tobytes() for a in out], all_bits(plan.xcorr_topk_f32(src, smp, 3, 2000)),
                all_bits(plan.xcorr_phat_f32(src, smp, band=band)))

    def counters(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes)

    rows = np.array([(-9, 9), (3, 2), (-N, N - 1), (0, 0), (-N, -N)], dtype=np.int64)
    with mod.Plan(N, 2, 0) as fresh:
        want = neighbours(fresh)
    with mod.Plan(N, 2, 0) as plan:
        neighbours(plan)                                              # the counters hold something to begin with
        plan.xcorr_phat_f32(src[0], smp, band=band)                   # the broadcast slot's first allocation is any stride-0 call's
        before = counters(plan)
        assert before[2] != (0, 0, 0) and before[3][1] > 0 and before[5] > 0, before
        seen = {}
        for exact in (True, False):
            plan.set_exact(exact)
            seen[exact] = (all_bits(plan.xcorr_phat_topk_f32(src, smp, 4, 1000, band=band)) + all_bits(plan.xcorr_phat_topk_f32(src, smp, 3, 5, rows)) +
                           all_bits(plan.xcorr_phat_topk_f32(src[0], smp, 2, 2 * N)))
        assert seen[True] == seen[False]
        plan.set_exact(True)
        assert counters(plan) == before
        # the records, the running maxima and the bound are shared: each neighbour right behind a PHAT top-k call
        for which in range(3):
            plan.xcorr_phat_topk_f32(src, smp, 4, 1000, rows, band)
            assert neighbours(plan)[which] == want[which], which
        plan.xcorr_phat_topk_f32(src, smp, 4, 1000, rows, band)
        assert neighbours(plan) == want


def test_refusals(mod, torch):
    src, smp = stacked(range(2))
    d_src = torch.from_numpy(np.concatenate([src.ravel(), src[0][:8]])).cuda()
    d_smp = torch.from_numpy(smp).cuda()
    k = 4
    with mod.Plan(N, 2, 0) as plan:
        good = dict(src=d_src.data_ptr(), ss=2 * N, smp=d_smp.data_ptr(), ts=N, lo=100, hi=1000, k=k, sep=10)
        bad = [("k = 0", dict(k=0)), ("k = 9", dict(k=9)), ("negative", dict(sep=-1)), ("not a band", dict(lo=5, hi=4)),
               ("not a band", dict(hi=N + 1)), ("null", dict(src=0)), ("null", dict(smp=0)), ("null", dict(drop=1)),
               ("null", dict(drop=3)), ("aligned", dict(src=d_src.data_ptr() + 4)), ("multiples of 4", dict(ss=6))]
        for text, change in bad:
            a = dict(good)
            a.update(change)
            out = outputs(torch, 2 * k)
            ptrs = [t.data_ptr() for t in out]
            if "drop" in a:
                ptrs[a["drop"]] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_phat_topk_dev(a["src"], a["ss"], a["smp"], a["ts"], 0, 0, 2, a["lo"], a["hi"], a["k"], a["sep"], *ptrs)
            assert untouched(torch, out), (text, change)
        out = outputs(torch, 2 * k)
        plan.xcorr_phat_topk_dev(good["src"], 2 * N, good["smp"], N, 0, 0, 0, 100, 1000, k, 10, *(t.data_ptr() for t in out))  # batch == 0
        assert untouched(torch, out)
        # d_lag and d_peak may be NULL
        out = outputs(torch, 2 * k)
        plan.xcorr_phat_topk_dev(good["src"], 2 * N, good["smp"], N, 0, 0, 2, 100, 1000, k, 10, 0, out[1].data_ptr(), 0, out[3].data_ptr())
        plan.sync()
        want = plan.xcorr_phat_topk_f32(src, smp, k, 10, band=(100, 1000))
        assert out[1].cpu().numpy().tobytes() == want[1].tobytes() and out[3].cpu().numpy().tobytes() == want[3].tobytes()
        assert out[0].cpu().tolist() == [-99] * (2 * k) and out[2].cpu().tolist() == [7.0] * (2 * k)


PACKED_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as graft
mod = graft.load()
n = 144000
with mod.Plan(n, 1, 0) as plan:
    assert plan.layout == "packed", plan.layout
    for lo, hi in ((1, n // 6), (0, n)):
        try:
            plan.xcorr_phat_topk_f32(np.ones(2 * n, dtype=np.float32), np.ones(n, dtype=np.float32), 3, 10, band=(lo, hi))
        except mod.AsxError as e:
            assert "real-column" in str(e), e
            print("refused", lo, hi)
"""


def test_a_production_length_forced_to_a_packed_plan_is_refused(mod):
    """ASX_LAYOUT=packed is read when a plan is made; a fresh process, so that nothing of this one's state is involved"""
    import os
    import subprocess
    import sys
    from util import ROOT
    env = dict(os.environ, ASX_LAYOUT="packed")
    done = subprocess.run([sys.executable, "-c", PACKED_CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split("\n")[:2] == ["refused 1 24000", "refused 0 144000"], (done.stdout, done.stderr)
