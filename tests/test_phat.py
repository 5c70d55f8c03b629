"""GCC-PHAT without a GPU: the float64 model of tests/phat_model.py on inputs whose answer is known, and the census and budgets
of the PHAT row kernels in the built library (k_rows_rp: a name of its own next to the twelve k_rows_r instances)."""
import re

import numpy as np

import oracle
import phat_model
from test_kernel_resources import demangled, kernels  # noqa: F401  (the fixture)
from util import asx


def test_a_pure_circular_delay_has_peak_one():
    n = 6000
    rng = np.random.default_rng(5)
    src = rng.standard_normal(2 * n)
    for lag in (0, 1, 777, n - 1, -1, -2500, -n):
        full = np.roll(src, -lag)                       # full[j] = src[j + lag], circular
        r = phat_model.r_phat(src, full)                # all 2N samples of the delayed track: nothing is cut off
        ret, got, _, peak = phat_model.model(src, full[:n], r=r)
        assert got == lag and abs(peak - 1.0) < 1e-12, (lag, got, peak)
        rest = np.abs(r)
        rest[lag % (2 * n)] = 0.0
        assert rest.max() < 1e-12


def test_zero_bins_cast_no_vote():
    n = 512
    src = np.zeros(2 * n)
    src[3] = 1.0
    r = phat_model.r_phat(src, np.zeros(n))
    assert not r.any()
    ret, lag, coef, peak = phat_model.model(src, np.zeros(n))
    assert (ret, lag, peak) == (-1, 0, 0.0) and np.isnan(coef)


def test_hum_moves_the_raw_peak_and_not_the_phat_peak():
    for p in range(3):
        src, smp, planted = phat_model.hum_pair(p)
        plain = oracle.cross_correlation(src, smp)[1]
        ret, lag, coef, peak = phat_model.model(src, smp)
        assert plain != planted and lag == planted and ret == 0, (p, planted, plain, lag)
        assert 0.2 < peak < 0.5, (p, peak)


def test_the_model_scales_and_negates_as_the_contract_says():
    n = 6000
    src, smp, planted = oracle.synth_pair(3, 1, n, 1)
    base = phat_model.model(src, smp)
    assert base[1] == planted
    for s in (2.0 ** 40, 2.0 ** -40):
        got = phat_model.model(src.astype(np.float64) * s, smp.astype(np.float64) * s)
        assert got[1] == base[1] and abs(got[3] - base[3]) < 1e-12
    neg = phat_model.model(src, -smp)
    assert neg[1] == base[1] and abs(neg[2] + base[2]) < 1e-12 and abs(neg[3] - base[3]) < 1e-12


def test_phat_row_kernels_census_and_budgets(kernels):  # noqa: F811
    names = {demangled(k): v for k, v in kernels.items()}
    rows = [(n, r) for n, r in names.items() if n.startswith("void k_rows_rp<")]
    assert len(rows) == 12, sorted(n for n, _ in rows)
    forms = set()
    for n, r in rows:
        assert r["vgpr_count"] <= 128 and r["private_segment_fixed_size"] == 0, (n, r)
        m = re.match(r"void k_rows_rp<(Sched<[^>]*>, \d+), (true|false), (\d)>", n)
        two = m.group(2) == "true"
        forms.add((m.group(1), two, int(m.group(3))))
        m2 = int(re.search(r"Sched<(\d+)", n).group(1)) * (2 if two else 1)
        blocks = 4 if two else 8
        if m2 <= 1200 or two:  # k_rows_r's LDS budget (tests/test_kernel_resources.py)
            assert blocks * (m2 * 16 + r["group_segment_fixed_size"]) <= 160 * 1024, (n, r)
        # the plain instance of the same form: the same registers' worth of occupancy and the same static LDS
        plain = names[next(p for p in names if p.startswith(n.replace("k_rows_rp<", "k_rows_r<").split("(")[0] + "("))]
        assert r["group_segment_fixed_size"] == plain["group_segment_fixed_size"], (n, r, plain)
    assert len({f[:2] for f in forms}) == 3 and {f[2] for f in forms} == {0, 1, 2, 3}, forms
    assert len([n for n in names if n.startswith("void k_rows_r<")]) == 12
    tails = [n for n in names if n.startswith("void k_phat_finalize<")]
    assert len(tails) == 2, tails


def test_the_python_surface_names_the_two_calls():
    mod = asx()
    from audiosync_amd import hipxcorr
    assert {"asx_xcorr_phat_f32_dev", "asx_xcorr_phat_debug_r_dev"} <= set(hipxcorr.ABI_SYMBOLS)
    for name in ("xcorr_phat_dev", "phat_debug_r_dev", "xcorr_phat_f32"):
        assert callable(getattr(mod.Plan, name)), name
    assert all(hasattr(mod.lib(), name) for name in ("asx_xcorr_phat_f32_dev", "asx_xcorr_phat_debug_r_dev"))
