"""The checker's own test (tests/edges.py), on numpy stand-ins: a helper that cannot see a planted write proves nothing on the GPU."""
import numpy as np
import pytest

import edges


def tracks(count, length, seed=0):
    return np.random.default_rng(seed).standard_normal((count, length)).astype(np.float32)


@pytest.mark.parametrize("poison", edges.POISONS)
@pytest.mark.parametrize("count, length, front, stride", [(3, 10, 5, 13), (3, 12, 64, 48), (1, 7, 0, 7), (3, 1, 5, 2), (2, 6, 5, 6)])
def test_embed_then_gather_returns_the_tracks(poison, count, length, front, stride):
    t = tracks(count, length)
    buf, offset, st = edges.embed(t, front, stride, poison)
    assert (offset, st) == (front, stride) and buf.dtype == np.float32
    assert edges.gather(buf, offset, st, count, length).tobytes() == t.tobytes()
    for slack in (0, 16):
        dense = edges.materialise(t, slack=slack)
        assert dense.tobytes() == t.tobytes() and dense.ctypes.data % 16 == 0 and dense.shape == (count * length,)
    # every other element is poison: in front, in the gaps, and at least `front` (and at least 4) behind
    mask = np.ones(buf.size, dtype=bool)
    for i in range(count):
        mask[offset + i * stride:offset + i * stride + length] = False
    assert buf.size - (offset + (count - 1) * stride + length) >= max(front, 4)
    rest = buf[mask]
    if poison == "nan":
        assert np.isnan(rest).all()
    else:
        assert (np.abs(rest) == np.float32(1e30)).all() and np.isfinite(rest).all()
        assert (rest > 0).any() and (rest < 0).any()


def test_a_stride_of_zero_is_one_track_between_poison():
    t = tracks(3, 9)
    buf, offset, st = edges.embed(t, 5, 0, "nan")
    assert st == 0 and buf.size == 5 + 9 + 5
    assert edges.gather(buf, offset, 0, 3, 9).tobytes() == np.stack([t[0]] * 3).tobytes()
    assert np.isnan(buf[:5]).all() and np.isnan(buf[14:]).all()
    with pytest.raises(AssertionError):
        edges.embed(t, 5, 8, "nan")                            # overlapping tracks leave no room for poison


def test_embed_rows_puts_the_filler_everywhere_else():
    rows = np.array([[-3, 4], [0, 0], [5, 9]], dtype=np.int64)
    buf, offset = edges.embed_rows(rows, 2, [100, 100], front=2)
    got = buf.reshape(-1, 2)
    assert offset == 4 and got.shape == (2 + 5 + 2, 2)
    assert got[2::2][:3].tolist() == rows.tolist()
    assert got[[0, 1, 3, 5, 7, 8]].tolist() == [[100, 100]] * 6
    lines, offset = edges.embed_rows(np.array([[0.5, 1.0, np.nan]] * 2), 1, [np.nan] * 3, front=1)
    assert offset == 3 and lines.size == 12 and np.isnan(lines[:3]).all() and np.isnan(lines[9:]).all() and lines[3] == 0.5
    one, offset = edges.embed_rows(rows, 0, [7, 7], front=1)
    assert one.tolist() == [7, 7, -3, 4, 7, 7] and offset == 2


@pytest.mark.parametrize("dtype", list(edges.SENTINEL))
def test_check_guards_sees_one_element_on_either_side_and_nothing_else(dtype):
    count = 5
    whole, view = edges.guarded(None, dtype, count)
    assert whole.size == count + 2 * edges.GUARD and view.size == count and (view == 7).all()
    assert view.ctypes.data % 16 == 0 and np.shares_memory(view, whole)
    assert edges.check_guards(whole, count) == []
    view[:] = np.arange(count)                                 # the call's own writes: any values, NaN included
    if dtype.startswith("float"):
        view[0] = np.nan
    assert edges.check_guards(whole, count) == []
    for at, side in ((edges.GUARD + count, "back"), (edges.GUARD - 1, "front"), (0, "front"), (whole.size - 1, "back")):
        w, _ = edges.guarded(None, dtype, count)
        w[at] = 0
        found = edges.check_guards(w, count)
        assert len(found) == 1 and found[0].startswith(side), (at, found)
    # a write of the payload's own 7, of a NaN and of the other type's pattern are all seen: the comparison is by bytes
    for value in ([7, np.nan] if dtype.startswith("float") else [7, -1]):
        w, _ = edges.guarded(None, dtype, count)
        w[edges.GUARD + count] = value
        assert len(edges.check_guards(w, count)) == 1, value


def test_a_guard_of_another_width():
    whole, view = edges.guarded(None, "int32", 3, guard=4)
    assert whole.size == 11 and edges.check_guards(whole, 3, guard=4) == []
    whole[7] = 1
    assert len(edges.check_guards(whole, 3, guard=4)) == 1


@pytest.mark.parametrize("poison", edges.POISONS)
def test_unchanged_sees_a_write_into_a_gap(poison):
    t = tracks(3, 10)
    buf, offset, stride = edges.embed(t, 5, 13, poison)
    before = edges.snapshot(buf)
    assert edges.unchanged(buf, before)                        # NaN poison compares equal to itself: bytes, not values
    for at in (offset + 10, offset + 12, 0, buf.size - 1, offset):
        b = buf.copy()
        b[at] = np.float32(0.0) if at != offset else np.float32(b[at] + 1.0)
        assert not edges.unchanged(b, before), at
    b = buf.copy()
    b[offset + 11] = -b[offset + 11]                            # the sign bit of a poison value alone
    assert not edges.unchanged(b, before)
