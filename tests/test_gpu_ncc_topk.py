"""Top-k normalised cross-correlation on the MI355X (asx_xcorr_ncc_topk_f32_dev, Plan.xcorr_ncc_topk_f32): k = 1 and entry 0 are the
NCC call, every entry is the rule of tests/ncc_topk_model.py applied to the curve the device itself forms (no tolerance), fixture C
against the float64 model, the entries that are not lags (-2, -3, no competing lag), refusals, and the state the call leaves alone."""
import numpy as np
import pytest

import edges
import ncc_model
import ncc_topk_model as tm
import oracle
from util import asx

pytestmark = pytest.mark.gpu

COEF_TOL = 1e-5
CURVE_TOL = 8e-7   # tests/test_gpu_ncc.py: the measured tolerance of the curve against the float64 model
MARGIN = 0.1       # tests/test_ncc_topk.py asserts it on the model of fixture C

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixture_c(n, p):
    return cached(("c", n, p), lambda: tm.fixture_c(n, p))


def parity_pair(n, k):
    """fixtures A and B of tests/ncc_model.py, then generator pairs"""
    if k == 0:
        return cached(("a", n), lambda: ncc_model.fixture_a(n, 0))
    if k == 1:
        return cached(("b", n), lambda: ncc_model.fixture_b(n, 0))
    return cached(("synth", n, k), lambda: oracle.synth_pair(91, k, n, 1))


def model_c(n, p):
    """the float64 model's curve of fixture C, computed once and never written to"""
    def make():
        src, smp, _ = fixture_c(n, p)
        cv = ncc_model.curve(src, smp)
        for a in cv[:2]:
            a.setflags(write=False)
        return cv
    return cached(("curve c", n, p), make)


def same(a, b):
    return [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]


def bits(out, k):
    return [np.asarray(a)[k].tobytes() for a in out]


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


def device_curves(plan, torch, d_src, src_step, d_smp, smp_step, batch, n, min_energy=ncc_model.DEFAULT_ENERGY):
    """asx_xcorr_ncc_debug_c_dev on every pair of device tensors d_src / d_smp (pair i at i * step floats): |c32| [batch, N], NaN
    where the lag does not compete"""
    d_c = torch.full((batch, n), 7.0, dtype=torch.float32, device="cuda")
    out = (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for i in range(batch):
        plan.ncc_debug_c_dev(d_src.data_ptr() + 4 * i * src_step, d_smp.data_ptr() + 4 * i * smp_step, min_energy,
                             d_c.data_ptr() + 4 * i * n, *(a.data_ptr() for a in out))
    plan.sync()
    return np.abs(d_c.cpu().numpy())


def check_exact(what, got, keys, k, sep, rows=None):
    """every entry of every pair is the rule applied to the device's own curve: lag, peak and ret equal, no tolerance"""
    lag, coef, peak, ret = (np.asarray(a).reshape(-1, k) for a in got)
    for i in range(keys.shape[0]):
        row = None if rows is None else (rows[i] if rows.ndim == 2 else rows)
        want = tm.topk_of_keys(keys[i], k, sep, None if row is None else (int(row[0]), int(row[1])))
        for j, (status, wlag, wpeak) in enumerate(want):
            here = (what, i, j, want, lag[i].tolist(), peak[i].tolist(), ret[i].tolist())
            if status == 0:
                assert int(lag[i, j]) == wlag and float(peak[i, j]) == wpeak, here
                assert int(ret[i, j]) == (-1 if np.isnan(coef[i, j]) else 0), here
            else:
                assert (int(lag[i, j]), int(ret[i, j])) == (0, status) and np.isnan(coef[i, j]) and np.isnan(peak[i, j]), here


def small_pairs(n):
    """fixture C (p = 0, 1) and two generator pairs at a small length"""
    ps = [fixture_c(n, 0), fixture_c(n, 1)] + [cached(("small", n, k), lambda k=k: oracle.synth_pair(31, k, n, 1)) for k in (2, 3)]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])


# ---- relation to the NCC call -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5000, 144000])
def test_k_one_and_entry_zero_are_the_ncc_call(mod, n):
    if n == 144000:
        ps = [fixture_c(n, 0), parity_pair(n, 0), parity_pair(n, 1), fixture_c(n, 1), parity_pair(n, 2)]
        src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    else:
        src, smp = small_pairs(n)
    b = src.shape[0]
    rows = np.array([(0, n - 1), (n // 3, n // 2), (5, 5), (7, 3), (0, n // 4)][:b], dtype=np.int64)
    sep = n // 100
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == ("real-column" if n == 144000 else "packed")
        for args in ((src, smp, None), (src, smp, rows), (src[0], smp, None), (src[0], smp, rows[1])):
            want = plan.xcorr_ncc_f32(args[0], args[1], args[2])
            one = plan.xcorr_ncc_topk_f32(args[0], args[1], 1, sep, args[2])
            assert all(a.shape == (b, 1) for a in one)
            assert same([a[:, 0] for a in one], want)
            for k in (3, 8):
                got = plan.xcorr_ncc_topk_f32(args[0], args[1], k, sep, args[2])
                assert same([np.ascontiguousarray(a[:, 0]) for a in got], want), k


# ---- the exact check --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 2049, 5000])
def test_every_entry_is_the_rule_on_the_devices_curve_packed(mod, torch, n):
    src, smp = small_pairs(n)
    b = src.shape[0]
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    rows = np.array([(0, n - 1), (n // 3, n - 1 - n // 4), (0, n // 2), (n // 5, n // 5 + min(n - 1 - n // 5, 40))], dtype=np.int64)
    with mod.Plan(n, 3, 0) as plan:
        assert plan.layout == "packed"
        keys = device_curves(plan, torch, d_src, 2 * n, d_smp, n, b, n)
        for sep in sorted({0, n // 100, n}):
            for k in (2, 8):
                check_exact((n, sep, k), plan.xcorr_ncc_topk_f32(src, smp, k, sep), keys, k, sep)
                check_exact((n, sep, k, "rows"), plan.xcorr_ncc_topk_f32(src, smp, k, sep, rows), keys, k, sep, rows)


def test_every_entry_is_the_rule_on_the_devices_curve_real_column(mod, torch):
    """fixture C, fixtures A and B and a generator pair; max_batch 2: three launch groups"""
    n = 144000
    ps = [fixture_c(n, 0), parity_pair(n, 0), parity_pair(n, 1), parity_pair(n, 2), fixture_c(n, 2)]
    src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()
    rows = np.array([(0, n - 1), (14000, 15000), (100, n - 100), (n // 2, n - 1), (70000, 120000)], dtype=np.int64)
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column" and plan.group <= 2
        keys = device_curves(plan, torch, d_src, 2 * n, d_smp, n, 5, n)
        for sep in (0, n // 100, n):
            check_exact((n, sep), plan.xcorr_ncc_topk_f32(src, smp, 4, sep), keys, 4, sep)
            check_exact((n, sep, "rows"), plan.xcorr_ncc_topk_f32(src, smp, 4, sep, rows), keys, 4, sep, rows)


def test_more_than_one_ncc_group(mod, torch):
    """N = 144 000: an NCC group is 310 pairs; 330 rotations of fixture C's sample against its source, broadcast"""
    n, b, k = 144000, 330, 3
    src, smp, _ = fixture_c(n, 0)
    smps = np.stack([np.roll(smp, 37 * i) for i in range(b)])
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smps).cuda()
    rows = np.array([(0, n - 1) if i % 3 else (i * 100, n - 1 - i * 50) for i in range(b)], dtype=np.int64)
    rows[311] = (9, 8)
    sep = n // 100
    with mod.Plan(n, b, 0) as plan:
        assert plan.group >= b
        before = plan.debug_ncc()
        got = plan.xcorr_ncc_topk_f32(src, smps, k, sep, rows)
        after = plan.debug_ncc()
        assert (after[2] - before[2], after[3] - before[3]) == (1, b)
        keys = device_curves(plan, torch, d_src, 0, d_smp, n, b, n)
    check_exact("groups", got, keys, k, sep, rows)
    assert got[3][311].tolist() == [-2] * k and len({int(v) for v in got[0][:, 0]}) > 100


# ---- fixture C against the float64 model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5000, 144000])
def test_fixture_c_against_the_model(mod, n):
    ps = [fixture_c(n, p) for p in (0, 1, 2)]
    src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    sep = n // 100
    with mod.Plan(n, 2, 0) as plan:
        plan.set_pearson(False)
        lag, coef, peak, ret = plan.xcorr_ncc_topk_f32(src, smp, 3, sep)
        rows = np.stack([lag.reshape(-1), lag.reshape(-1)], axis=1)
        direct = plan.xcorr_windowed_f32(np.repeat(src, 3, axis=0), np.repeat(smp, 3, axis=0), rows)
        if plan.layout == "real-column":  # (the only plans with a spectral form)
            plan.set_pearson(True)        # the coefficient is the direct form's whatever the plan's setting
            assert same(plan.xcorr_ncc_topk_f32(src, smp, 3, sep), (lag, coef, peak, ret))
    worst = 0.0
    for p in (0, 1, 2):
        want = tm.topk(*model_c(n, p), 4, sep)
        assert tuple(e[1] for e in want[:3]) == ps[p][2] and all(a[2] - b[2] >= MARGIN for a, b in zip(want[:3], want[1:]))
        assert tuple(lag[p].tolist()) == ps[p][2] and ret[p].tolist() == [0, 0, 0], (p, lag[p], ret[p])
        for j in range(3):
            worst = max(worst, abs(float(peak[p, j]) - want[j][2]))
            at = int(lag[p, j])
            assert abs(float(coef[p, j]) - oracle.pearson_coefficient(src[p][at:at + n], smp[p])) < COEF_TOL
    print("ncc top-k fixture c N", n, "worst |peak - model|", worst)
    assert worst <= CURVE_TOL
    assert direct[0].tolist() == lag.reshape(-1).tolist() and direct[1].tobytes() == coef.tobytes()


def test_the_point_of_the_call(mod):
    """fixture C at N = 144 000: the raw top 3 over the same lags never hold the 0.3 copy; the normalised top 3 end with it"""
    n = 144000
    ps = [fixture_c(n, p) for p in (0, 1, 2)]
    src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    sep = n // 100
    with mod.Plan(n, 3, 0) as plan:
        raw = plan.xcorr_topk_f32(src, smp, 3, sep, np.array([0, n - 1], dtype=np.int64))
        free = plan.xcorr_topk_f32(src, smp, 3, sep)
        got = plan.xcorr_ncc_topk_f32(src, smp, 3, sep)
    for p in (0, 1, 2):
        quiet = ps[p][2][2]
        print("fixture c", p, "planted", ps[p][2], "raw", raw[0][p].tolist(), "raw, every lag", free[0][p].tolist(), "ncc", got[0][p].tolist())
        assert raw[2][p].tolist() == [0, 0, 0]
        for table in (raw, free):
            assert all(abs(int(v) - quiet) > sep for v in table[0][p])
        assert int(got[0][p][2]) == quiet and tuple(got[0][p].tolist()) == ps[p][2]


# ---- entries that are not lags ----------------------------------------------------------------------------------------------------

def test_special_entries(mod):
    n = 144000
    ps = [parity_pair(n, 1), fixture_c(n, 0), fixture_c(n, 1), parity_pair(n, 2), fixture_c(n, 2)]
    src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    k, sep = 4, 1000
    full = (0, n - 1)
    with mod.Plan(n, 2, 0) as plan:
        alone = [plan.xcorr_ncc_topk_f32(src[i], smp[i], k, sep) for i in range(5)]
        # -3: a row narrower than 2 min_separation + 1 around the loudest copy of pair 1 holds one entry; -2: rows that are not rows
        # of this call; the neighbours are what they are alone
        rows = np.array([full, (72000 - 300, 72000 + 300), (9, 3), full, (-1, 5)], dtype=np.int64)
        got = plan.xcorr_ncc_topk_f32(src, smp, k, sep, rows)
        for i in (0, 3):
            assert bits(got, i) == bits(alone[i], 0), i
        lag, coef, peak, ret = (a[1] for a in got)
        assert int(lag[0]) == 72000 == ps[1][2][0] and int(ret[0]) == 0 and float(peak[0]) == float(alone[1][2][0][0])
        assert lag[1:].tolist() == [0, 0, 0] and ret[1:].tolist() == [-3, -3, -3] and np.isnan(coef[1:]).all() and np.isnan(peak[1:]).all()
        for i in (2, 4):
            assert got[0][i].tolist() == [0] * k and got[3][i].tolist() == [-2] * k
            assert np.isnan(got[1][i]).all() and np.isnan(got[2][i]).all()
        # a constant sample: no lag competes, every entry is the smallest lag of A_j with peak 0
        flat = np.full(n, 0.25, dtype=np.float32)
        got = plan.xcorr_ncc_topk_f32(src[:3], np.stack([smp[0], flat, smp[2]]), k, sep, np.array([full, (17, 3500), full], dtype=np.int64))
        assert got[0][1].tolist() == [17, 1018, 2019, 3020] and got[2][1].tolist() == [0.0] * 4
        assert got[3][1].tolist() == [-1] * 4 and np.isnan(got[1][1]).all()
        for i in (0, 2):
            assert bits(got, i) == bits(alone[i], 0), i
        got = plan.xcorr_ncc_topk_f32(src[0], flat, 3, n // 2)
        assert got[0][0].tolist() == [0, n // 2 + 1, 0] and got[3][0].tolist() == [-1, -1, -3] and np.isnan(got[2][0][2])
    one = oracle.synth_pair(31, 1, 1, 1)
    with mod.Plan(1, 1, 0) as plan:
        got = plan.xcorr_ncc_topk_f32(one[0], one[1], 2, 0)
        assert got[0][0].tolist() == [0, 0] and got[3][0].tolist() == [-1, -3] and float(got[2][0][0]) == 0.0 and np.isnan(got[2][0][1])


# ---- refusals, and what the call leaves alone -------------------------------------------------------------------------------------

def test_refusals(mod, torch):
    n, k = 144000, 3
    src, smp, _ = fixture_c(n, 0)
    d_src = torch.from_numpy(np.concatenate([src, src, src[:8]])).cuda()
    d_smp = torch.from_numpy(np.concatenate([smp, smp])).cuda()
    kinds = ("int64", "float64", "float64", "int32")

    def outputs():
        return [edges.guarded(torch, kind, 2 * k) for kind in kinds]

    def untouched(out):
        torch.cuda.synchronize()
        return all(not edges.check_guards(whole, 2 * k) and view.cpu().tolist() == [edges.PAYLOAD] * (2 * k) for whole, view in out)

    with mod.Plan(n, 2, 0) as plan:
        good = (d_src.data_ptr(), 2 * n, d_smp.data_ptr(), n)
        cases = [("null", good, 1e-3, k, 0, 1), ("null", good, 1e-3, k, 0, 2), ("null", good, 1e-3, k, 0, 3),
                 ("null", (0, 2 * n, d_smp.data_ptr(), n), 1e-3, k, 0, None), ("null", (d_src.data_ptr(), 2 * n, 0, n), 1e-3, k, 0, None),
                 ("aligned", (d_src.data_ptr() + 4, 2 * n, d_smp.data_ptr(), n), 1e-3, k, 0, None),
                 ("multiples of 4", (d_src.data_ptr(), 6, d_smp.data_ptr(), n), 1e-3, k, 0, None),
                 ("min_energy", good, 0.0, k, 0, None), ("min_energy", good, 1e-7, k, 0, None), ("min_energy", good, 1.5, k, 0, None),
                 ("min_energy", good, float("nan"), k, 0, None),
                 ("k = 0", good, 1e-3, 0, 0, None), ("k = 9", good, 1e-3, 9, 0, None), ("negative", good, 1e-3, k, -1, None)]
        for text, (ps, ss, pm, ms), energy, kk, sep, drop in cases:
            out = outputs()
            ptrs = [view.data_ptr() for _, view in out]
            if drop is not None:
                ptrs[drop] = 0
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=text):
                plan.xcorr_ncc_topk_dev(ps, ss, pm, ms, 0, 0, 2, energy, kk, sep, *ptrs)
            assert untouched(out), (text, energy, kk, sep, drop)
        out = outputs()
        ptrs = [view.data_ptr() for _, view in out]
        assert mod.lib().asx_xcorr_ncc_topk_f32_dev(None, *good, None, 0, 2, 1e-3, k, 0, *ptrs, None) == -1
        assert mod.lib().asx_xcorr_ncc_topk_f32_dev(plan._h, *good, None, 0, 0, 1e-3, k, 0, *ptrs, None) == 0  # batch == 0
        assert untouched(out)
        # d_lag may be NULL
        plan.xcorr_ncc_topk_dev(*good, 0, 0, 2, 1e-3, k, n // 100, 0, *ptrs[1:])
        plan.sync()
        assert not any(edges.check_guards(whole, 2 * k) for whole, _ in out)
        assert out[0][1].cpu().tolist() == [edges.PAYLOAD] * (2 * k) and out[3][1].cpu().tolist() == [0] * (2 * k)


def test_what_the_call_leaves_alone(mod, torch):
    n = 144000
    ps = [fixture_c(n, 0), parity_pair(n, 0), parity_pair(n, 1), fixture_c(n, 1), parity_pair(n, 2)]
    src, smp = np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])
    d_src, d_smp = torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda()

    def plain(plan):
        out = (torch.zeros(5, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"),
               torch.zeros(5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), 5, *(a.data_ptr() for a in out))
        plan.sync()
        return [a.cpu().numpy().tobytes() for a in out]

    def state(plan):
        return (plan.peak_overflows(), plan.peak_repairs(), plan.pearson_modes(), plan.prune_stats(), plan.qstore_stats(),
                plan.workspace_bytes)

    with mod.Plan(n, 2, 0) as fresh:
        want_plain = plain(fresh)
    with mod.Plan(n, 2, 0) as plan:
        plain(plan)                                                   # the counters hold something to begin with
        plan.xcorr_broadcast_f32(src[0], smp)                         # (the broadcast slot is the strided call's, and counted)
        before = state(plan)
        assert before[2] != (0, 0, 0) and before[3][1] > 0, before
        made = plan.debug_ncc()
        first = plan.xcorr_ncc_topk_f32(src, smp, 4, 1440)
        assert plan.debug_ncc()[2:] == (made[2] + 5, made[3] + 5)
        assert same(plan.xcorr_ncc_topk_f32(src, smp, 4, 1440), first)  # a second call: the same bits
        for exact, prune, qstore in ((False, True, 1), (True, False, 2), (False, False, 0)):
            plan.set_exact(exact)
            plan.set_prune(prune)
            plan.set_qstore(qstore)
            assert same(plan.xcorr_ncc_topk_f32(src, smp, 4, 1440), first), (exact, prune, qstore)
        plan.set_exact(True)
        plan.set_prune(True)
        plan.set_qstore(1)
        plan.set_lag_window(100, 5000)
        assert same(plan.xcorr_ncc_topk_f32(src, smp, 4, 1440), first) and plan.lag_window == (100, 5000)
        plan.set_lag_window(-n, n - 1)
        plan.xcorr_ncc_topk_f32(src[0], smp, 8, 0, np.array([(0, 9), (3, 2), (0, n - 1), (0, 0), (-n, -n)], dtype=np.int64))
        assert state(plan) == before
        assert plain(plan) == want_plain
