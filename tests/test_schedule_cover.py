"""The committed lists of tests/schedule_cover.py against the planner itself (host-only): CASES reaches every feature the run-time
transform schedules can show, EMBEDDED_CASES and LONG are what the GPU tests take them for.  A change to the planner, to
asx_make_stages or to pick_threads that moves a feature fails here until `python tests/schedule_cover.py` has made a new list --
as test_plan_math.py fails on a kernel-table entry that no plan reaches."""
import pytest

import schedule_cover as sv
from util import asx


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in sv.PLAN_ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def mod():
    return asx()


@pytest.fixture(scope="module")
def whole(mod):
    import os
    saved = {k: os.environ.pop(k) for k in sv.PLAN_ENV if k in os.environ}
    try:
        return sv.universe(mod)
    finally:
        os.environ.update(saved)


def spell(fs):
    return sorted(fs, key=repr)


def test_the_universe_holds_every_radix_instance_block_and_tile(whole):
    """every radix of lds_fft.h in every MAXR instance that can hold it, both families; the stage counts, blocks and tiles"""
    for fam in ("cols", "rows"):
        radices = {f[2] for f in whole if f[0] == fam and isinstance(f[1], int)}
        assert radices == {16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2}, (fam, radices)
        assert {f[1] for f in whole if f[0] == fam and isinstance(f[1], int)} == {10, 12, 16}
        assert {f[2] for f in whole if f[:2] == (fam, "block")} <= set(range(64, 513, 64))
        assert 512 in {f[2] for f in whole if f[:2] == (fam, "block")}
    assert {f[2] for f in whole if f[:2] == ("cols", "T")} == set(sv.TILES)
    assert max(f[2] for f in whole if f[:2] == ("cols", "stages")) >= 5
    assert {f[2] for f in whole if f[:2] == ("rows", "M2")} == {"even", "odd"}
    assert {f[2] for f in whole if f[:2] == ("rows", "steps")} == set(range(1, sv.ROW_STEPS + 1))


def test_cases_reach_every_feature_and_nothing_else(mod, whole):
    got = set()
    for c in sv.CASES:
        got |= sv.case_features(mod, c)
    missing, unknown = whole - got, got - whole
    assert not missing, "no entry of CASES runs %s: regenerate the list (python tests/schedule_cover.py)" % spell(missing)
    assert not unknown, "CASES run %s, which the universe does not hold" % spell(unknown)


def test_every_case_is_a_packed_plan_on_run_time_kernels(mod):
    assert len(set(c[:3] for c in sv.CASES)) == len(sv.CASES)
    for m1, m2, t, seed in sv.CASES:
        n = m1 * m2
        d, k = sv.plan_of(mod, n, sv.split_string(m1, m2, t))      # AsxError: the planner refuses the split
        assert (d["F"], d["M1"], d["M2"], d["T"]) == (2 * n, m1, m2, t), (m1, m2, t, d)
        assert (k["layout"], k["cols"], k["rows"]) == ("packed", None, None), (m1, m2, t, k)
        assert sv.N_MIN <= n <= sv.N_MAX and m2 >= t, (m1, m2, t)
        assert sv.column_features(d, k) and sv.row_features(d, k)


def test_the_batch_pairs_of_every_case_have_a_clear_peak():
    """the GPU test skips no pair as a near-tie: the oracle's margin of all three pairs of every case's seed, here on the CPU"""
    for c in sv.CASES:
        m = sv.margins(c[0] * c[1], c[3])
        assert min(m) >= sv.MARGIN_MIN, (c, m)
    for c in sv.EMBEDDED_CASES:
        m = sv.margins(c[0], c[4])
        assert min(m) >= sv.MARGIN_MIN, (c, m)


def test_embedded_cases_are_embedded_and_varied(mod):
    assert len(sv.EMBEDDED_CASES) >= 6
    plans = []
    for n, m1, m2, t, seed in sv.EMBEDDED_CASES:
        assert not mod.planmath_describe(n)["F"] == 2 * n
        d, k = sv.plan_of(mod, n, sv.split_string(m1, m2, t))
        F = d["F"]
        assert F >= 3 * n - 1 and F % 2 == 0 and 2 * m1 * m2 == F and d["src_valid"] == 3 * n - 1, (n, d)
        assert all(F2 % 2 or not _smooth(F2) for F2 in range(3 * n - 1, F)), (n, F)     # the NEXT smooth even length
        assert (d["M1"], d["M2"], d["T"]) == (m1, m2, t)
        assert (k["layout"], k["cols"], k["rows"]) == ("packed", None, None), (n, k)
        plans.append((n, d))
    assert {n & 1 for n, d in plans} == {0, 1}
    assert {2, 64} <= {d["T"] for n, d in plans}
    assert any(len(d["radix1"]) >= 3 for n, d in plans)
    assert any(d["M2"] & 1 for n, d in plans)


def _smooth(v):
    for p in (2, 3, 5):
        while v % p == 0:
            v //= p
    return v == 1


@pytest.mark.parametrize("n", sorted(sv.LONG))
def test_the_longest_lengths_plan_as_recorded_inside_the_universe(mod, whole, n):
    F, split, threads = sv.LONG[n]
    d, k = sv.plan_of(mod, n)
    assert (d["F"], (d["M1"], d["M2"], d["T"]), tuple(k["threads"])) == (F, split, threads)
    assert (k["layout"], k["cols"], k["rows"]) == ("packed", None, None)
    f = sv.column_features(d, k) | sv.row_features(d, k)
    assert f and not f - whole, "N = %d runs %s, which no configuration of the universe shows" % (n, spell(f - whole))


def test_the_long_list_holds_the_four_lengths():
    assert sorted(sv.LONG) == [1953125, 2097152, 3999971, 4000000]
    assert sv.LONG[1953125][0] == 2 * 1953125 and sv.LONG[1953125][1][1] & 1         # odd N, odd M2, not embedded
    assert sv.LONG[3999971][0] == 12000000                                            # a prime: embedded in 3N - 1 -> 12 000 000
