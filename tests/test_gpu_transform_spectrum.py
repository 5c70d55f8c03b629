"""The device correlation bin by bin (tests/spectrum_check.py): r from asx_xcorr_debug_r_dev goes back to the frequency domain
in float64 and every bin of X conj(Y) is held against its own float32 error scale -- an error confined to a few bins, which
the time-domain comparisons in test_gpu_parity.py cannot see, fails here with the bin's coordinates in the plan's split.

Then impulse pairs on the decomposition's edges through the production entry points, whose exact answer is known.
Run with `-m gpu -s` on an MI355X to see the measured z of every case (spectrum_check.Z_MAX records the floor)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import spectrum_check as sc
from device_spectrum import run_case
from util import asx

pytestmark = pytest.mark.gpu

PRODUCTION = [144000, 288000, 480000, 720000, 960000, 1440000]
COEF_TOL = 1e-5


@pytest.fixture(scope="module")
def mod():
    m = asx()
    assert m.device_count() >= 1, "no MI355X visible"
    return m


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- per-bin parity: the real-column kernels (csrc/rlayout.hip) at the six production lengths ----------------------------

@pytest.mark.parametrize("kind", ["W", "I", "C", "D"])
@pytest.mark.parametrize("n", PRODUCTION)
def test_real_column_spectrum_bin_by_bin(mod, torch, monkeypatch, n, kind):
    monkeypatch.delenv("ASX_LAYOUT", raising=False)
    run_case(mod, torch, n, kind, want_layout="real-column")


# ---- the packed-sample kernels (csrc/xcorr_kernels.hip), $ASX_LAYOUT=packed read at plan creation -------------------------

@pytest.mark.parametrize("kind", ["W", "I"])
@pytest.mark.parametrize("n", [144000, 288000, 720000, 1440000])
def test_packed_spectrum_bin_by_bin(mod, torch, monkeypatch, n, kind):
    monkeypatch.setenv("ASX_LAYOUT", "packed")
    run_case(mod, torch, n, kind, want_layout="packed")


# ---- smooth lengths outside the tuned table (F == 2N, the planner's own split) ---------------------------------------------

@pytest.mark.parametrize("n", [1000, 4096, 48000, 65536, 96000, 250000])
def test_smooth_lengths_spectrum_bin_by_bin(mod, torch, monkeypatch, n):
    monkeypatch.delenv("ASX_LAYOUT", raising=False)
    d = mod.planmath_describe(n)
    assert d["F"] == 2 * n, "N = %d is smooth by construction, the planner embeds it in F = %d" % (n, d["F"])
    run_case(mod, torch, n, "W")


# ---- forced splits of 144 000 (test_same_answer_for_every_split's list, plus the tuned split forced) -------------------------

SPLITS_144000 = ["144x1000x32", "288x500x16", "360x400x16", "1000x144x8", "96x1500x64", "600x240x8", "1x144000x1",
                 "300x480x16"]


def test_forced_splits_spectrum_bin_by_bin(mod, torch, monkeypatch):
    monkeypatch.delenv("ASX_LAYOUT", raising=False)
    layouts, rejected = {}, []
    for split in SPLITS_144000:
        try:
            with mod.Plan(144000, 1, 0, split=split):
                pass
        except mod.AsxError:
            rejected.append(split)
            continue
        layouts[split] = run_case(mod, torch, 144000, "W", split=split).layout
    print("forced splits of 144000: %s; rejected by the planner: %s" % (layouts, rejected))
    assert set(layouts.values()) == {"real-column", "packed"}, layouts


# ---- the run-time-schedule kernels ($ASX_GENERIC=1, read when a plan is created; here in a child process) ------------------------------

_GENERIC_SPECTRUM = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import torch
assert torch.cuda.is_available()
import numpy as np
import __graft_entry__ as g
import spectrum_check as sc
asx = g.load()
for n in (144000, 480000):
    d = asx.planmath_describe(n)
    for kind in ("W", "I"):
        x, y = sc.inputs(kind, n, a=2 * n - 1, b=d["M2"] - 1)
        d_src = torch.from_numpy(x).cuda(); d_smp = torch.from_numpy(y).cuda()
        d_r = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        d_lag = torch.zeros(1, dtype=torch.int64, device="cuda"); d_coef = torch.zeros(1, dtype=torch.float64, device="cuda")
        d_ret = torch.zeros(1, dtype=torch.int32, device="cuda")
        with asx.Plan(n, 1, 0) as plan:
            layout, spl, F = plan.layout, plan.split, plan.fft_len
            plan.debug_r_dev(d_src.data_ptr(), d_smp.data_ptr(), d_r.data_ptr(), d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
            plan.sync()
        assert F == 2 * n
        r = d_r.cpu().numpy().astype(np.float64) / F
        res = sc.check(sc.Reference(x, y), r, spl[0], spl[1], layout, "generic " + kind)
        print("RESULT " + json.dumps({"n": n, "kind": kind, "layout": layout, "zmax": res.zmax, "summary": res.summary(),
                                      "message": res.message()}), flush=True)
"""


def test_generic_kernels_spectrum_bin_by_bin(mod):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("ASX_LAYOUT", None)
    env["ASX_GENERIC"] = "1"
    p = subprocess.run([sys.executable, "-c", _GENERIC_SPECTRUM % {"root": root, "tests": os.path.join(root, "tests")}],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [json.loads(l[len("RESULT "):]) for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(got) == 4, p.stdout[-2000:]
    for g in got:
        print(g["summary"])
    for g in got:
        assert g["layout"] == "packed", g
        assert g["zmax"] < sc.Z_MAX, g["message"]


# ---- impulse pairs on the decomposition's edges through the production entry points ------------------------------------------

def impulse_batch(d, n):
    """(a, b) pairs: x = e_a, y = e_b, the exact r a single spike at p = (a - b) mod 2N.  a on the edges of tiles, rows, bands
    and the matrix; b on the edges of the sample; every a with two of the b's"""
    M1, M2, T = d["M1"], d["M2"], d["T"]
    F = 2 * n
    band = 40 * M2   # a band edge at every length (test_spectral_form_matches_the_oracle_and_the_direct_form)
    As = [0, T - 1, T, M2 - 1, M2, band - 1, band + 1, (2 * M1 - 1) * M2, F - 1]
    Bs = [0, 1, M2 - 1, n - 1]
    return [(a, Bs[i % 4]) for i, a in enumerate(As)] + [(a, Bs[(i + 2) % 4]) for i, a in enumerate(As)]


@pytest.mark.parametrize("n", PRODUCTION)
def test_impulse_pairs_on_the_edges_match_the_oracle(mod, torch, monkeypatch, n):
    monkeypatch.delenv("ASX_LAYOUT", raising=False)
    d = mod.planmath_describe(n)
    F = 2 * n
    pairs = impulse_batch(d, n)
    B = len(pairs)
    src = np.zeros((B, F), dtype=np.float32)
    smp = np.zeros((B, n), dtype=np.float32)
    for i, (a, b) in enumerate(pairs):
        src[i, a] = 1.0
        smp[i, b] = 1.0
    with mod.Plan(n, B, 0) as plan:
        assert plan.layout == "real-column"
        lag, coef, ret = plan.xcorr_batch_f32(src, smp)
        d_src = torch.from_numpy(src).cuda()
        d_smp = torch.from_numpy(smp).cuda()
        d_lag = torch.zeros(B, dtype=torch.int64, device="cuda")
        d_coef = torch.zeros(B, dtype=torch.float64, device="cuda")
        d_ret = torch.zeros(B, dtype=torch.int32, device="cuda")
        plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), B, d_lag.data_ptr(), d_coef.data_ptr(), d_ret.data_ptr())
        plan.sync()
        modes = plan.pearson_modes()
    print("N=%d impulse batch of %d: pearson_modes (spectral, spectral + wrap, direct) = %s" % (n, B, modes))
    lag_d, coef_d, ret_d = d_lag.cpu().numpy(), d_coef.cpu().numpy(), d_ret.cpu().numpy()
    # the two entry points: bit for bit
    assert np.array_equal(lag, lag_d) and np.array_equal(ret, ret_d)
    assert np.array_equal(coef.view(np.uint64), coef_d.view(np.uint64))
    for i, (a, b) in enumerate(pairs):
        p = (a - b) % F
        o_ret, o_lag, o_coef = oracle.cross_correlation(src[i], smp[i])
        assert o_lag == (p if p < n else p - F), (a, b, o_lag)   # the oracle finds the analytic spike
        where = "N=%d pair %d (a=%d, b=%d, spike at %d)" % (n, i, a, b, p)
        assert int(ret[i]) == o_ret and int(lag[i]) == o_lag, (where, int(ret[i]), int(lag[i]), o_ret, o_lag)
        if o_ret == 0:
            assert abs(float(coef[i]) - o_coef) < COEF_TOL, (where, float(coef[i]), o_coef)
        if np.isnan(coef[i]):
            assert int(ret[i]) == -1 and np.isnan(o_coef), (where, int(ret[i]), o_coef)
