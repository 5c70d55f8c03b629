"""Host planning arithmetic (csrc/plan_math.cpp) against the NumPy model of the device
algorithm (tests/model_fourstep.py): transform length, split, radix schedule, digit-reversal
tables, twiddle tables.  No GPU needed."""
import numpy as np
import pytest

import model_fourstep as model
from util import asx

PRODUCTION = [144000, 288000, 480000, 720000, 960000, 1440000]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 11, 13, 100, 1000, 1001, 4096, 48000, 12345] + PRODUCTION)
def test_length_and_split(n):
    d = asx().planmath_describe(n)
    F, valid = model.embed_params(n, model.next_smooth_even)
    assert d["F"] == F and d["src_valid"] == valid
    M = F // 2
    assert d["M1"] * d["M2"] == M
    assert d["T"] >= 1 and d["T"] & (d["T"] - 1) == 0 and d["T"] <= 64
    # LDS: a column tile; a row block = four rows of the packed-sample kernel, or one row of each spectrum of the
    # real-column kernel (the 2400-point rows of the two longest reference lengths, csrc/rlayout.hip)
    assert d["M1"] * d["T"] * 8 <= 80 * 1024
    assert 4 * d["M2"] * 8 <= 64 * 1024 or (n in (960000, 1440000) and 2 * d["M2"] * 8 <= 64 * 1024)
    assert int(np.prod(d["radix1"], dtype=np.int64)) == d["M1"]
    assert int(np.prod(d["radix2"], dtype=np.int64)) == d["M2"]
    assert set(d["radix1"] + d["radix2"]) <= {2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16}


@pytest.mark.parametrize("n", PRODUCTION)
def test_production_lengths_are_not_embedded_and_use_wide_tiles(n):
    d = asx().planmath_describe(n)
    assert d["F"] == 2 * n          # true circular correlation of length 2N
    assert d["T"] >= 16             # sixteen real columns per tile: 64-byte input pieces, whole lines of the intermediates
    assert d["M1"] % 2 == 0 and d["M2"] % d["T"] == 0 and d["M2"] in (480, 1200, 2400)   # what csrc/rlayout.hip needs


@pytest.mark.parametrize("n", [6, 30, 1000, 48000, 144000])
def test_position_tables_match_model(n):
    mod = asx()
    d = mod.planmath_describe(n)
    pos1 = mod.planmath_table(n, 0)
    inv1 = mod.planmath_table(n, 1)
    pos2 = mod.planmath_table(n, 2)
    assert np.array_equal(pos1, model.position_table(d["M1"], d["radix1"]))
    assert np.array_equal(pos2, model.position_table(d["M2"], d["radix2"]))
    assert np.array_equal(inv1[pos1], np.arange(d["M1"]))
    assert sorted(pos2.tolist()) == list(range(d["M2"]))


def test_split_override_and_rejects():
    mod = asx()
    d = mod.planmath_describe(1000, "25x40x8")
    assert (d["M1"], d["M2"], d["T"]) == (25, 40, 8)
    for bad in ("25x41x8", "25x40x3", "0x1000x8", "nonsense"):
        with pytest.raises(mod.AsxError):
            mod.planmath_describe(1000, bad)


@pytest.mark.parametrize("n", [1000, 144000, 1440000])
def test_twiddle_tables(n):
    mod = asx()
    d = mod.planmath_describe(n)
    F, M1, M2 = d["F"], d["M1"], d["M2"]
    tw1 = mod.planmath_twiddles(n, 0)
    tw2 = mod.planmath_twiddles(n, 1)
    lo = mod.planmath_twiddles(n, 2)
    hi = mod.planmath_twiddles(n, 3)
    assert np.abs(tw1 - model.tw(M1, np.arange(M1))).max() < 1e-7
    assert np.abs(tw2 - model.tw(M2, np.arange(M2))).max() < 1e-7
    # the two-level table reproduces w_F^p for random p < F to float32 accuracy
    rng = np.random.default_rng(0)
    p = rng.integers(0, F, 4096)
    got = lo[p & 2047].astype(np.complex128) * hi[p >> 11].astype(np.complex128)
    assert np.abs(got - model.tw(F, p)).max() < 2.5e-7


def test_inplace_stage_model_round_trip():
    # the in-place DIF / DIT recipe the kernels use (lds_fft.h), checked in float64
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 12, 60, 360):
        rad = model.radix_list(n)
        x = rng.normal(size=n) + 1j * rng.normal(size=n)
        y = model.dif_forward_inplace(x, rad)
        pos = model.position_table(n, rad)
        assert np.abs(y[pos] - np.fft.fft(x)).max() < 1e-10
        assert np.abs(model.dit_inverse_inplace(y, rad) - n * x).max() < 1e-9


def test_unsupported_lengths_are_rejected_with_a_message():
    mod = asx()
    for bad in (0, (1 << 27) + 1):
        with pytest.raises(mod.AsxError):
            mod.planmath_describe(bad)
    # a huge prime sample_len embeds into a smooth length that must still split into LDS-sized factors
    d = mod.planmath_describe(3999971)
    assert d["F"] >= 3 * 3999971 - 1 and d["M1"] * d["M2"] * 2 == d["F"]


@pytest.mark.parametrize("n", [45, 1000, 44100, 96000, 1000000, 1440000])
def test_measured_mode_candidates_are_valid_splits(n):
    mod = asx()
    base = mod.planmath_describe(n)
    cands = mod.planmath_candidates(n, 16)
    assert 1 <= len(cands) <= 16 and len(set(cands)) == len(cands)
    for c in cands:
        d = mod.planmath_describe(n, c)          # every candidate must be accepted as an explicit split
        m1, m2, t = (int(x) for x in c.split("x"))
        assert (d["M1"], d["M2"], d["T"]) == (m1, m2, t)
        assert m1 * m2 * 2 == base["F"] and d["F"] == base["F"]
        assert t >= 2 and (t & (t - 1)) == 0 and m1 * t * 8 <= 80 * 1024 and 4 * m2 * 8 <= 64 * 1024


@pytest.mark.parametrize("m1,m2", [(4, 8), (6, 4), (10, 12), (12, 20), (30, 16)])
def test_real_column_decomposition_matches_the_reference_recipe(m1, m2):
    """csrc/rlayout.hip's algebra (model_fourstep.rlayout_*): r2c columns with the untangling inside the tile, rows
    k1 = 0..M1 independent, c2r columns -- equals rfft * conj(rfft) -> irfft of src/cross_correlation.c:204-239"""
    n = m1 * m2
    rng = np.random.default_rng(m1 * 100 + m2)
    src = rng.standard_normal(2 * n)
    smp = rng.standard_normal(n)
    r = model.rlayout_xcorr(src, smp, m1, m2)
    ref = model.reference_r(src, smp)
    assert np.abs(r - ref).max() < 1e-9 * np.abs(ref).max()


def test_spectral_pearson_algebra_matches_the_reference_reduction():
    """csrc/pearson_spectral.hip's identity, in float64: r[peak] (minus the products that did not wrap around, for a negative
    lag) and band + edge window sums give pearson_coefficient() of the segments src/cross_correlation.c:256-271 selects --
    for lags inside a band, on band borders, with windows that hold no whole band, and with offsets in both tracks."""
    import oracle
    M2, T, rows = 48, 16, 40                  # a [40][48] sample matrix for the sample, [80][48] for the source; bands of 8 rows
    N = rows * M2
    gs = 8 * M2
    rng = np.random.default_rng(17)
    source = rng.normal(size=2 * N) + 0.3
    sample = rng.normal(size=N) - 0.2
    peaks = [0, 1, 5, gs - 1, gs, gs + 1, 3 * gs, N - 1, N - gs, N, N + 1, N + 7, N + gs, 2 * N - gs, 2 * N - gs - 3, 2 * N - 5,
             2 * N - 1, N + N // 2]
    for peak in peaks:
        lag, coef, mode = model.spectral_pearson(source, sample, peak, M2, T)
        if peak >= N:
            want_lag = (peak % N) - N
            a, b = source[: N + want_lag], sample[-want_lag:]
        else:
            want_lag = peak
            a, b = source[peak: peak + N], sample
        assert lag == want_lag
        if len(a) < 2:
            continue
        want = oracle.pearson_coefficient(a.copy(), b.copy())
        assert abs(coef - want) < 1e-10, (peak, mode, coef, want)


# ---- which compiled-in kernels a plan runs (csrc/kernel_table.h, AsxKernelChoice) ----------------
# The environment is read when a plan is built, so each case sets it for itself.

KERNEL_ENV = ("ASX_LAYOUT", "ASX_GENERIC", "ASX_THREADS_COLS", "ASX_THREADS_ROWS", "ASX_STAGE_ORDER")


def kernels(monkeypatch, n, split=None, **env):
    for k in KERNEL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return asx().planmath_kernels(n, split)


def rcol_rows_per_group(m1, nt, t):
    """row pairs one lane group of k_fwd_cols_r loads: the block's nt / (t / 4) groups share the m1 rows"""
    groups = nt // (t // 4)
    return (m1 + groups - 1) // groups


RCOL = {300: (300, 16, 256, (10, 6, 5)), 400: (400, 16, 512, (10, 8, 5)), 600: (600, 16, 512, (10, 10, 6))}
RROW = {480: (64, False, 480, (10, 8, 6)), 1200: (128, False, 1200, (12, 10, 10)), 2400: (128, True, 1200, (12, 10, 10))}
REAL_COLUMN = {144000: (300, 480), 288000: (600, 480), 480000: (400, 1200), 720000: (600, 1200), 960000: (400, 2400),
               1440000: (600, 2400)}
# ASX_LAYOUT=packed: what the parent of the commit that introduced the table matched at run time (its ASX_STATIC_COLS chain and the
# two hand-written row schedules, with asx_pick_threads' block sizes), evaluated by a host program on that commit's sources
PCOL = {300: (300, 16, 256, 10, (10, 6, 5)), 400: (400, 16, 320, 10, (10, 8, 5)), 600: (600, 16, 512, 10, (10, 10, 6)),
        800: (800, 8, 320, 10, (10, 10, 8)), 1200: (1200, 8, 512, 12, (12, 10, 10))}
PROW = {480: (128, 10, 480, (10, 8, 6)), 1200: (256, 12, 1200, (12, 10, 10))}
PACKED = {144000: (300, 480, (256, 128)), 288000: (600, 480, (512, 128)), 480000: (400, 1200, (320, 256)),
          720000: (600, 1200, (512, 256)), 960000: (800, 1200, (320, 256)), 1440000: (1200, 1200, (512, 256))}


@pytest.mark.parametrize("n", PRODUCTION)
def test_production_lengths_run_the_real_column_kernels(monkeypatch, n):
    k = kernels(monkeypatch, n)
    m1, m2 = REAL_COLUMN[n]
    assert k["layout"] == "real-column"
    assert k["cols"] == RCOL[m1] and k["rows"] == RROW[m2]
    assert k["prunable"] is True
    _, t, nt, _ = RCOL[m1]
    assert k["band_rows"] == 2 * rcol_rows_per_group(m1, nt, t)


@pytest.mark.parametrize("n", PRODUCTION)
def test_packed_layout_runs_the_compiled_in_packed_schedules(monkeypatch, n):
    k = kernels(monkeypatch, n, ASX_LAYOUT="packed")
    m1, m2, threads = PACKED[n]
    assert k == {"layout": "packed", "cols": PCOL[m1], "rows": PROW[m2], "threads": threads, "band_rows": 0, "prunable": False}
    assert k["cols"][2] == threads[0] and k["rows"][0] == threads[1]     # a compiled-in block size is the plan's block size


@pytest.mark.parametrize("n", PRODUCTION)
def test_generic_runs_no_compiled_in_schedule(monkeypatch, n):
    k = kernels(monkeypatch, n, ASX_GENERIC="1")
    assert (k["layout"], k["cols"], k["rows"], k["prunable"]) == ("packed", None, None, False)
    assert k["threads"] == PACKED[n][2]


def test_a_length_outside_the_table_runs_the_run_time_schedules(monkeypatch):
    k = kernels(monkeypatch, 1000, "25x40x8")
    assert (k["layout"], k["cols"], k["rows"], k["band_rows"], k["prunable"]) == ("packed", None, None, 0, False)


def test_a_split_without_a_column_pair_is_refused_as_before(monkeypatch):
    with pytest.raises(asx().AsxError, match="bad ASX_SPLIT override"):
        kernels(monkeypatch, 144000, "1x144000x1")
    # one the planner accepts but no table holds: the packed kernels on run-time schedules
    k = kernels(monkeypatch, 144000, "150x960x16")
    assert (k["layout"], k["cols"], k["rows"]) == ("packed", None, None)


def test_a_block_size_override_leaves_the_compiled_in_packed_schedule(monkeypatch):
    """the packed instances are compiled for one block size: another one runs the run-time-schedule kernel of that pass alone"""
    k = kernels(monkeypatch, 144000, ASX_LAYOUT="packed", ASX_THREADS_COLS="512")
    assert k["cols"] is None and k["rows"] == PROW[480] and k["threads"] == (512, 128)
    k = kernels(monkeypatch, 144000, ASX_LAYOUT="packed", ASX_THREADS_ROWS="256")
    assert k["cols"] == PCOL[300] and k["rows"] is None and k["threads"] == (256, 256)


def test_every_entry_of_the_kernel_table_is_reached(monkeypatch):
    """an entry no plan resolves to is a set of kernels built for nothing: the lengths and environments above reach all of them.
    The lists are read from the library (csrc/kernel_table.h), so an entry added there is held to this too."""
    table = asx().planmath_kernel_table()
    assert table == {"real-column cols": [RCOL[600], RCOL[400], RCOL[300]], "real-column rows": [RROW[1200], RROW[2400], RROW[480]],
                     "packed cols": [PCOL[1200], PCOL[800], PCOL[600], PCOL[400], PCOL[300]], "packed rows": [PROW[1200], PROW[480]]}
    seen = {"real-column": (set(), set()), "packed": (set(), set())}
    for env in ({}, {"ASX_LAYOUT": "packed"}, {"ASX_GENERIC": "1"}):
        for n in PRODUCTION:
            k = kernels(monkeypatch, n, **env)
            seen[k["layout"]][0].add(k["cols"])
            seen[k["layout"]][1].add(k["rows"])
    for layout in seen:
        for which, reached in zip(("cols", "rows"), seen[layout]):
            unreached = set(table["%s %s" % (layout, which)]) - reached
            assert not unreached, "no plan runs %s %s %s" % (layout, which, sorted(unreached))
    assert seen["real-column"] == (set(RCOL.values()), set(RROW.values()))
    assert seen["packed"] == (set(PCOL.values()) | {None}, set(PROW.values()) | {None})
