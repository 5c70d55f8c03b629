"""Helpers for the tests of where a track or a buffer begins and ends (tests/test_gpu_track_edges.py; their own test on numpy
stand-ins: tests/test_edges.py).

An entry point reads pair i at base + i * stride and writes exactly the documented number of output elements.  These helpers put
the tracks into one buffer with poison everywhere else, put sentinel bit patterns around every output, and compare bytes afterwards:

    embed        tracks at offset + i * stride of one buffer, poison in front, in the gaps and behind
    materialise  the same tracks dense, as every other test builds them
    embed_rows   index and row arrays (windows, pool pairs, centres, lines) with rows in between that would change the answer
    guarded      an output with `guard` sentinel elements on each side of the `count` the call may write
    check_guards the sentinels are still there
    snapshot / unchanged   an input buffer holds the bytes it held before the call, poison included

Every function takes `torch=None`: with the torch module the buffers live on the current device, without it they are numpy arrays
(the stand-ins the CPU test plants its writes into).  Plain module: no fixtures, nothing happens on import."""
import numpy as np

GUARD = 64
# poisons: a quiet NaN, and 1e30 with alternating sign -- finite, so that a path that short-cuts on a NaN input still sees it, and
# large enough that one stray product changes every sum it enters
POISONS = ("nan", "big")
# sentinels no call produces: signalling-NaN payloads for the floating types, 0x5a5a... for the integers
SENTINEL = {"float64": (np.uint64, 0x7FF4DEAD7FF4DEAD), "float32": (np.uint32, 0x7FA4DEAD),
            "int64": (np.uint64, 0x5A5A5A5A5A5A5A5A), "int32": (np.uint32, 0x5A5A5A5A)}
PAYLOAD = 7          # what the existing tests fill their outputs with


def poison_values(count, poison, dtype=np.float32):
    """`count` poison values: "nan", or "big" = +1e30, -1e30, +1e30, ..."""
    if poison == "nan":
        return np.full(count, np.nan, dtype=dtype)
    assert poison == "big", poison
    v = np.full(count, 1e30, dtype=dtype)
    v[1::2] = -1e30
    return v


def _device(host, torch):
    return host if torch is None else torch.from_numpy(host).cuda()


def _host(buffer):
    return buffer.cpu().numpy() if hasattr(buffer, "cpu") else np.asarray(buffer)


def embed(tracks, front, stride, poison, torch=None, back=None):
    """float32 tracks [count, length] -> (buffer, offset, stride): track i sits at buffer[offset + i * stride ..+ length], every other
    element holds the poison -- the `front` elements ahead of track 0, the gaps, and `back` elements behind the last track (at least
    max(front, 4), the default; more where a wrong kernel would read further, such as the zero half behind a sample).
    stride = 0: one track (tracks[0]; the call broadcasts it) with poison on both sides."""
    tracks = np.asarray(tracks, dtype=np.float32)
    assert tracks.ndim == 2 and front >= 0
    count, length = tracks.shape
    if stride == 0:
        count = 1
    assert stride == 0 or stride >= length, "tracks must not overlap: the poison sits in the gaps"
    back = max(front, 4) if back is None else back
    assert back >= max(front, 4), (back, front)
    total = front + (count - 1) * stride + length + back
    host = poison_values(total, poison)
    for i in range(count):
        host[front + i * stride:front + i * stride + length] = tracks[i]
    return _device(host, torch), front, stride


def gather(buffer, offset, stride, count, length):
    """what a call that honours (offset, stride) reads: [count, length]"""
    host = _host(buffer)
    return np.stack([host[offset + i * stride:offset + i * stride + length] for i in range(count)])


def materialise(tracks, torch=None, slack=0):
    """the same tracks dense and (as a fresh allocation) 16-byte aligned: [count * length] row after row, as the other tests build
    them.  slack: that many zeros behind the last track, outside the returned view, so that a wrong kernel's read past the end
    stays inside memory the test owns"""
    dense = np.ascontiguousarray(tracks, dtype=np.float32).reshape(-1)
    whole = _device(np.concatenate([dense, np.zeros(slack, dtype=np.float32)]), torch)
    return whole[:dense.size]


def embed_rows(rows, row_stride, filler, front=2, torch=None):
    """rows [count, width] of an index or row array -> (buffer, offset): row i sits at buffer[offset + i * row_stride * width ..+
    width]; the `front` rows ahead of row 0, the row_stride - 1 rows between two read rows and the `front` rows behind the last one
    hold `filler` (one row of `width` values that would change the answer if it were read).  row_stride = 0: one row."""
    rows = np.asarray(rows)
    assert rows.ndim == 2
    count, width = rows.shape
    if row_stride == 0:
        count = 1
    slots = front + (count - 1) * row_stride + 1 + front
    host = np.empty((slots, width), dtype=rows.dtype)
    host[:] = np.asarray(filler, dtype=rows.dtype)
    for i in range(count):
        host[front + i * row_stride] = rows[i]
    return _device(host.reshape(-1), torch), front * width


def guarded(torch, dtype, count, guard=GUARD):
    """-> (whole, view): `whole` has guard + count + guard elements of `dtype` ("float64", "float32", "int64", "int32"), the guards
    filled with the type's sentinel bit pattern and the payload with 7s; `view` = whole[guard : guard + count] is what the call gets
    (view.data_ptr() on the device).  guard * itemsize is a multiple of 16 for every guard that is a multiple of 4."""
    bits, pattern = SENTINEL[dtype]
    host = np.empty(count + 2 * guard, dtype=dtype)
    host.view(bits)[:] = pattern
    host[guard:guard + count] = PAYLOAD
    whole = _device(host, torch)
    return whole, whole[guard:guard + count]


def check_guards(whole, count, guard=GUARD):
    """-> the problems found, as strings: empty when both guards of guarded()'s `whole` hold their sentinel bytes"""
    host = _host(whole)
    bits, pattern = SENTINEL[str(host.dtype)]
    assert host.size == count + 2 * guard, (host.size, count, guard)
    raw = host.view(bits)
    found = []
    for name, lo, hi in (("front", 0, guard), ("back", guard + count, count + 2 * guard)):
        for at in np.flatnonzero(raw[lo:hi] != bits(pattern)).tolist():
            found.append("%s guard: element %d (%+d from the payload) holds 0x%x" %
                         (name, lo + at, lo + at - guard if name == "front" else lo + at - guard - count + 1, int(raw[lo + at])))
    return found


def snapshot(buffer):
    """the bytes of an input buffer, taken before the call"""
    return _host(buffer).tobytes()


def unchanged(buffer, before):
    """the buffer holds the bytes of its snapshot, poison included"""
    return _host(buffer).tobytes() == before
