"""The form of a launch group (csrc/plan_math.cpp: asx_group_form) tabled without a device: the ask of every caller of run_group
gives what that caller launches, each scope rule turns off with any one of its conditions and takes nothing else with it, and over
the ask's whole value space the form is the rules as DESIGN.md ("The form of a launch group") states them -- written out here a
second time, so that an edit of the C++ that changes a rule has to change this file too."""
import itertools

import pytest

from util import asx


@pytest.fixture(scope="module")
def form():
    return asx().planmath_group_form


# What a plan contributes to the ask (asx_plan_create_ex: a real-column plan has band sums and both switches on; a packed plan has
# neither; both have the overflow list).
REAL = dict(rlayout=True, plan_prune=True, plan_spectral=True, band_sums=True, over_list=True)
PACKED = dict(rlayout=False, plan_prune=False, plan_spectral=False, band_sums=False, over_list=True)
# GroupOpts' defaults with a float32 group's Pairs: what run_batch's group asks in the exact mode
CALL = dict(f32_inputs=True, f32_abi=True, listed=True, r_out=False, own_lists=False, k=1, search="all", weight="none", pool=False,
            bc=0, qstore=True)


def ask(plan=REAL, **changes):
    a = dict(plan, **CALL)
    assert set(changes) <= set(a), changes
    a.update(changes)
    return a


# The second look (second_look): lists of its own without the overflow list and the band sums, the direct form, not listed
SECOND_LOOK = dict(listed=False, f32_abi=False, own_lists=True, over_list=False, band_sums=False)

# caller -> (what it changes in the exact-mode ask, the form on a real-column plan, the form on a packed plan or None: the entry
# point refuses a packed plan or the group cannot arise there).  A form is (fwd, rows, weight, bc, pruned, tail, appends, qstore,
# takeback).
PACKED_EXACT = ("packed", "packed", "none", 0, False, "direct", True, False, False)
PACKED_QUIET = ("packed", "packed", "none", 0, False, "direct", False, False, False)
CALLERS = {
    "run_batch, exact mode": ({}, ("real-column", "energy", "none", 0, True, "spectral", True, True, True), PACKED_EXACT),
    "run_batch, asynchronous mode": (dict(listed=False),
                                     ("real-column", "energy", "none", 0, True, "spectral", False, False, False), PACKED_QUIET),
    "run_batch under a lag window": (dict(search="window"),
                                     ("real-column", "plain", "none", 0, False, "spectral", True, False, False), PACKED_EXACT),
    "strided, no shared track": ({}, ("real-column", "energy", "none", 0, True, "spectral", True, True, True), PACKED_EXACT),
    "strided, bc 1": (dict(bc=1), ("real-column", "plain", "none", 1, False, "spectral", True, False, False), None),
    "strided, bc 2": (dict(bc=2), ("real-column", "plain", "none", 2, False, "spectral", True, False, False), None),
    "strided, bc 3": (dict(bc=3), ("real-column", "plain", "none", 3, False, "spectral", True, False, False), None),
    "windowed": (dict(search="rows"), ("real-column", "plain", "none", 0, False, "spectral", True, False, False), PACKED_EXACT),
    "top-k": (dict(k=3), ("real-column", "plain", "none", 0, False, "spectral", True, False, False), PACKED_EXACT),
    "top-k, windowed, bc 1": (dict(k=8, search="rows", bc=1),
                              ("real-column", "plain", "none", 1, False, "spectral", True, False, False), None),
    "pool": (dict(pool=True), ("pool", "listed", "none", 0, False, "spectral", True, False, False), None),
    "pool top-k": (dict(pool=True, k=4), ("pool", "listed", "none", 0, False, "spectral", True, False, False), None),
    # (run_batch: a PHAT batch is asynchronous whatever the plan's mode)
    "PHAT": (dict(weight="phat", listed=False), ("real-column", "plain", "phat", 0, False, "phat", False, False, False), None),
    "PHAT, bc 2, windowed": (dict(weight="phat", listed=False, bc=2, search="rows"),
                             ("real-column", "plain", "phat", 2, False, "phat", False, False, False), None),
    "banded PHAT": (dict(weight="phat-band", listed=False),
                    ("real-column", "plain", "phat-band", 0, False, "phat", False, False, False), None),
    "pool PHAT": (dict(weight="phat", listed=False, pool=True), ("pool", "listed", "phat", 0, False, "phat", False, False, False), None),
    "pool PHAT, banded": (dict(weight="phat-band", listed=False, pool=True),
                          ("pool", "listed", "phat-band", 0, False, "phat", False, False, False), None),
    "host-pointer float32 (asx_xcorr_batch_f32)": ({}, ("real-column", "energy", "none", 0, True, "spectral", True, True, True),
                                                   PACKED_EXACT),
    "double ABI, narrowed": (dict(f32_abi=False), ("real-column", "plain", "none", 0, False, "direct", True, False, False), PACKED_EXACT),
    "double ABI, not narrowed": (dict(f32_abi=False, f32_inputs=False),
                                 ("real-column", "plain", "none", 0, False, "direct", True, False, False), PACKED_EXACT),
    "stream prefix (asx_stream_xcorr)": (dict(f32_inputs=False),
                                         ("real-column", "plain", "none", 0, False, "direct", True, False, False), PACKED_EXACT),
    "second look": (SECOND_LOOK, ("real-column", "plain", "none", 0, False, "direct", False, False, False), PACKED_QUIET),
    "second look of a double pair": (dict(SECOND_LOOK, f32_inputs=False),
                                     ("real-column", "plain", "none", 0, False, "direct", False, False, False), PACKED_QUIET),
    "second look of a top-k pair": (dict(SECOND_LOOK, k=3, search="rows"),
                                    ("real-column", "plain", "none", 0, False, "direct", False, False, False), PACKED_QUIET),
    "partial-store redo": (dict(qstore=False), ("real-column", "energy", "none", 0, True, "spectral", True, False, False), None),
    "asx_xcorr_debug_r_dev, exact mode": (dict(f32_abi=False, r_out=True),
                                          ("real-column", "plain", "none", 0, False, "direct", True, False, False), PACKED_EXACT),
    "asx_xcorr_debug_r_dev, asynchronous mode": (dict(f32_abi=False, r_out=True, listed=False),
                                                 ("real-column", "plain", "none", 0, False, "direct", False, False, False),
                                                 PACKED_QUIET),
    "asx_xcorr_phat_debug_r_dev": (dict(f32_abi=False, r_out=True, listed=False, weight="phat"),
                                   ("real-column", "plain", "phat", 0, False, "phat", False, False, False), None),
    "asx_xcorr_phat_band_debug_r_dev": (dict(f32_abi=False, r_out=True, listed=False, weight="phat-band"),
                                        ("real-column", "plain", "phat-band", 0, False, "phat", False, False, False), None),
}


def as_tuple(f, GROUP_FORM):
    return tuple(f[n] for n in GROUP_FORM)


@pytest.mark.parametrize("caller", sorted(CALLERS))
def test_every_caller_of_run_group_gets_the_form_it_launches(form, caller):
    names = asx().hipxcorr.GROUP_FORM
    changes, real, packed = CALLERS[caller]
    assert as_tuple(form(**ask(REAL, **changes)), names) == real
    if packed is not None:
        # (a packed plan has no broadcast slot: strided_batch gives its groups bc = 0)
        assert as_tuple(form(**ask(PACKED, **dict(changes, band_sums=False))), names) == packed


def test_the_binding_states_the_ask_and_the_form_in_the_order_of_the_header(form):
    import os
    import re
    from util import graft
    h = asx().hipxcorr
    text = open(os.path.join(graft.PKG_DIR, "csrc", "plan_math.h")).read()
    fields = lambda struct: [n for line in re.search(r"struct %s \{(.*?)\n\};" % struct, text, re.S).group(1).split("\n")
                             for n in re.findall(r"^\s+(?:bool|int|Asx\w+) (\w+)(?: = [^;]+)?;", line)]
    assert tuple(fields("AsxGroupAsk")) == h.GROUP_ASK
    assert tuple(fields("AsxGroupForm")) == ("fwd", "rows", "weight", "bc", "pruned", "tail", "appends", "qstore", "takeback") == h.GROUP_FORM
    with pytest.raises(ValueError):
        form(**dict(ask(), extra=1))
    a = ask()
    del a["k"]
    with pytest.raises(ValueError):
        form(**a)


# one flip of each condition of a rule, from the in-scope ask (run_batch's exact-mode group on a real-column plan)
PRUNE_FLIPS = [dict(plan_prune=False), dict(weight="phat"), dict(weight="phat-band"), dict(f32_inputs=False), dict(f32_abi=False),
               dict(pool=True), dict(bc=1), dict(bc=2), dict(bc=3), dict(r_out=True), dict(own_lists=True), dict(k=2),
               dict(search="window"), dict(search="rows"), dict(search="topk")]
SPECTRAL_FLIPS = [dict(f32_inputs=False), dict(plan_spectral=False), dict(f32_abi=False), dict(band_sums=False), dict(weight="phat"),
                  dict(weight="phat-band")]
QSTORE_FLIPS = PRUNE_FLIPS + [dict(listed=False), dict(qstore=False), dict(over_list=False)]


def expected_after(flip, base):
    """the in-scope form with what `flip` itself states or takes along by the OTHER rules; the rule under test is set by the caller"""
    e = dict(base)
    phat = flip.get("weight", "none") != "none"
    e["weight"], e["bc"] = flip.get("weight", "none"), flip.get("bc", 0)
    e["fwd"] = "pool" if flip.get("pool") else "real-column"
    if phat:
        e["tail"], e["appends"] = "phat", False
    return e


def test_in_scope_for_everything(form):
    assert form(**ask()) == dict(fwd="real-column", rows="energy", weight="none", bc=0, pruned=True, tail="spectral", appends=True,
                                 qstore=True, takeback=True)


@pytest.mark.parametrize("flip", PRUNE_FLIPS, ids=str)
def test_one_condition_less_turns_pruning_off_and_nothing_else(form, flip):
    base = form(**ask())
    got = form(**ask(**flip))
    assert not got["pruned"]
    # what follows from pruning by the rules: the row flavour, partial storing and its take-back
    e = expected_after(flip, base)
    e.update(pruned=False, rows="listed" if flip.get("pool") else "plain", qstore=False, takeback=False)
    # the two conditions pruning shares with the spectral tail take that along by ITS rule
    if "f32_inputs" in flip or "f32_abi" in flip:
        e["tail"] = "direct"
    assert got == e


@pytest.mark.parametrize("flip", SPECTRAL_FLIPS, ids=str)
def test_one_condition_less_turns_the_spectral_tail_off_and_nothing_else(form, flip):
    base = form(**ask())
    got = form(**ask(**flip))
    assert got["tail"] != "spectral"
    e = expected_after(flip, base)
    e.update(tail="phat" if "weight" in flip else "direct", takeback=False)
    # the conditions the tail shares with pruning take that along by ITS rule
    if "f32_inputs" in flip or "f32_abi" in flip or "weight" in flip:
        e.update(pruned=False, rows="plain", qstore=False)
    assert got == e


@pytest.mark.parametrize("flip", QSTORE_FLIPS, ids=str)
def test_one_condition_less_turns_partial_storing_off_and_nothing_else(form, flip):
    base = form(**ask())
    got = form(**ask(**flip))
    assert not got["qstore"] and not got["takeback"]
    if flip in PRUNE_FLIPS:
        return  # (stated in full by the pruning test)
    e = dict(base, qstore=False, takeback=False)
    if "listed" in flip:
        e["appends"] = False
    assert got == e


@pytest.fixture(scope="module")
def whole_space(form):
    """[(ask, form)] over every value of every field of the ask: 2^12 x k in {1, 2} x 4 searches x 3 weights x 4 bc, asked once"""
    h = asx().hipxcorr
    values = {n: (False, True) for n in h.GROUP_ASK}
    values.update(k=(1, 2), search=h.GROUP_ENUMS["search"], weight=h.GROUP_ENUMS["weight"], bc=(0, 1, 2, 3))
    asks = [dict(zip(h.GROUP_ASK, v)) for v in itertools.product(*(values[n] for n in h.GROUP_ASK))]
    assert len(asks) == 2 ** 12 * 2 * 4 * 3 * 4
    return [(a, form(**a)) for a in asks]


def test_a_weighted_ask_never_lists_is_never_spectral_and_never_pruned(whole_space):
    n = 0
    for a, f in whole_space:
        if a["weight"] != "none":
            assert not f["appends"] and f["tail"] == "phat" and not f["pruned"] and not f["qstore"] and not f["takeback"], a
            assert f["rows"] != "energy" and f["weight"] == a["weight"], a
            n += 1
    assert n == 2 * len(whole_space) // 3


def rules(a):
    """DESIGN.md, "The form of a launch group", a second time"""
    phat = a["weight"] != "none"
    appends = a["listed"] and not phat
    spectral = a["f32_inputs"] and a["plan_spectral"] and a["f32_abi"] and a["band_sums"] and not phat
    pruned = (a["plan_prune"] and not phat and a["f32_inputs"] and a["f32_abi"] and not a["pool"] and a["bc"] == 0 and not a["r_out"]
              and not a["own_lists"] and a["k"] == 1 and a["search"] == "all")
    qstore = pruned and a["listed"] and a["qstore"] and a["over_list"]
    if not a["rlayout"]:
        rows = "packed"
    elif pruned:
        rows = "energy"
    elif a["pool"]:
        rows = "listed"
    else:
        rows = "plain"
    return dict(fwd="pool" if a["pool"] else "real-column" if a["rlayout"] else "packed", rows=rows, weight=a["weight"], bc=a["bc"],
                pruned=pruned, tail="phat" if phat else "spectral" if spectral else "direct", appends=appends, qstore=qstore,
                takeback=qstore and spectral)


def test_over_the_whole_space_the_form_is_the_rules(whole_space):
    for a, f in whole_space:
        assert f == rules(a), a
