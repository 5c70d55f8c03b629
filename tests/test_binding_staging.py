"""The host-array methods of Plan over a recording stand-in for the loaded library: what goes up before the _dev call, the strides,
counts and null pointers that call gets, sync before the copies back, the shapes and dtypes that come back, and every device
pointer freed exactly once -- also when the call or an allocation fails.  No device: the plan is built without a handle."""
import ctypes

import numpy as np
import pytest

from util import asx

N, B, HANDLE = 16, 3, 0x1000
I64, F64, I32 = np.int64, np.float64, np.int32
RESULTS, PHAT_RESULTS = (I64, F64, I32), (I64, F64, F64, I32)


class FakeLib:
    """asx_device_malloc hands out distinct integers; the copies, the sync and the asx_xcorr_*_dev calls record themselves.  A
    copy back fills the host array with the number of the allocation it reads (1, 2, ... in the order of the allocations)."""

    def __init__(self, dev_rc=0, fail_alloc=None):
        self.log, self.ptrs, self.uploaded, self.dev_rc, self.fail_alloc = [], [], {}, dev_rc, fail_alloc

    def asx_last_error(self):
        return b"fake failure"

    def asx_device_malloc(self, nbytes, device):
        if self.fail_alloc is not None and len(self.ptrs) + 1 == self.fail_alloc:
            self.log.append(("malloc", nbytes, device, 0))
            return 0
        self.ptrs.append(0x10000 + 0x1000 * len(self.ptrs))
        self.log.append(("malloc", nbytes, device, self.ptrs[-1]))
        return self.ptrs[-1]

    def asx_device_free(self, ptr):
        self.log.append(("free", ptr))
        return 0

    def asx_memcpy_h2d(self, dst, src, nbytes):
        self.uploaded[dst] = ctypes.string_at(src, nbytes)
        self.log.append(("h2d", dst, nbytes))
        return 0

    def asx_memcpy_d2h(self, dst, src, nbytes):
        ctypes.memset(dst, self.ptrs.index(src) + 1, nbytes)
        self.log.append(("d2h", src, nbytes))
        return 0

    def asx_stream_sync(self, handle, stream):
        self.log.append(("sync", handle, stream))
        return 0

    def __getattr__(self, name):
        if not (name.startswith("asx_xcorr_") and name.endswith("_dev")):
            raise AttributeError(name)

        def call(*args):
            self.log.append(("dev", name, args))
            return self.dev_rc
        return call

    def kinds(self):
        return [e[0] for e in self.log]


@pytest.fixture
def hipxcorr():
    asx()
    from audiosync_amd import hipxcorr
    return hipxcorr


def plan_of(hipxcorr):
    plan = object.__new__(hipxcorr.Plan)
    plan._h, plan.sample_len, plan.device, plan._destroy = HANDLE, N, 0, lambda h: None
    return plan


def data():
    rng = np.random.default_rng(7)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    return dict(src1=f(2 * N), smp1=f(N), srcB=f(B, 2 * N), smpB=f(B, N), src2=f(2, 2 * N), rec=f(2 * N + 8),
                win1=np.array([-3, 5], dtype=I64), winB=np.array([[-1, 1], [0, 7], [-16, 15]], dtype=I64),
                win6=np.arange(12, dtype=I64).reshape(6, 2) - 6, pairs=np.array([[0, 1], [1, 2], [1, 0]], dtype=np.int32))


D = data()
IN, OUT = "in", "out"     # ("in", i): the device copy of the case's i-th input; ("out", j): the buffer of its j-th result

# (name, the call, the host arrays that go up, the _dev function, its arguments as the parent commit's code passes them, the
# results' shape and dtypes).  The strides are floats (rows for the windows), 0 for a shared 1-D operand; a window, pair list or
# stream that is left out is a null pointer (None).
CASES = [
    ("broadcast shared source", lambda p: p.xcorr_broadcast_f32(D["src1"], D["smpB"]), [D["src1"], D["smpB"]],
     "asx_xcorr_strided_f32_dev", (HANDLE, (IN, 0), 0, (IN, 1), N, B, (OUT, 0), (OUT, 1), (OUT, 2), None), (B,), RESULTS),
    ("broadcast one pair", lambda p: p.xcorr_broadcast_f32(D["src1"], D["smp1"]), [D["src1"], D["smp1"]],
     "asx_xcorr_strided_f32_dev", (HANDLE, (IN, 0), 0, (IN, 1), 0, 1, (OUT, 0), (OUT, 1), (OUT, 2), None), (1,), RESULTS),
    ("windowed rows", lambda p: p.xcorr_windowed_f32(D["srcB"], D["smp1"], D["winB"]), [D["srcB"], D["smp1"], D["winB"]],
     "asx_xcorr_windowed_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), 0, (IN, 2), 1, B, (OUT, 0), (OUT, 1), (OUT, 2), None), (B,), RESULTS),
    ("windowed one window", lambda p: p.xcorr_windowed_f32(D["srcB"], D["smpB"], [-3, 5]), [D["srcB"], D["smpB"], D["win1"]],
     "asx_xcorr_windowed_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), N, (IN, 2), 0, B, (OUT, 0), (OUT, 1), (OUT, 2), None), (B,), RESULTS),
    ("windows", lambda p: p.xcorr_windows_f32(D["rec"], D["smp1"], 4), [D["rec"], D["smp1"]],
     "asx_xcorr_strided_f32_dev", (HANDLE, (IN, 0), 4, (IN, 1), 0, 3, (OUT, 0), (OUT, 1), (OUT, 2), None), (3,), RESULTS),
    ("topk plan window", lambda p: p.xcorr_topk_f32(D["srcB"], D["smpB"], 2, 3), [D["srcB"], D["smpB"]],
     "asx_xcorr_topk_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), N, None, 0, B, 2, 3, (OUT, 0), (OUT, 1), (OUT, 2), None), (B, 2), RESULTS),
    ("topk rows", lambda p: p.xcorr_topk_f32(D["src1"], D["smpB"], np.int64(8), 0, D["winB"]), [D["src1"], D["smpB"], D["winB"]],
     "asx_xcorr_topk_f32_dev", (HANDLE, (IN, 0), 0, (IN, 1), N, (IN, 2), 1, B, 8, 0, (OUT, 0), (OUT, 1), (OUT, 2), None), (B, 8), RESULTS),
    ("phat", lambda p: p.xcorr_phat_f32(D["srcB"], D["smp1"]), [D["srcB"], D["smp1"]],
     "asx_xcorr_phat_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), 0, None, 0, B, (OUT, 0), (OUT, 1), (OUT, 2), (OUT, 3), None), (B,),
     PHAT_RESULTS),
    ("phat one window", lambda p: p.xcorr_phat_f32(D["srcB"], D["smpB"], (-3, 5)), [D["srcB"], D["smpB"], D["win1"]],
     "asx_xcorr_phat_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), N, (IN, 2), 0, B, (OUT, 0), (OUT, 1), (OUT, 2), (OUT, 3), None), (B,),
     PHAT_RESULTS),
    ("phat band", lambda p: p.xcorr_phat_band_f32(D["srcB"], D["smpB"], 2, 9), [D["srcB"], D["smpB"]],
     "asx_xcorr_phat_band_f32_dev", (HANDLE, (IN, 0), 2 * N, (IN, 1), N, None, 0, B, 2, 9, (OUT, 0), (OUT, 1), (OUT, 2), (OUT, 3), None),
     (B,), PHAT_RESULTS),
    ("phat band rows", lambda p: p.xcorr_phat_band_f32(D["src1"], D["smpB"], 0, N, D["winB"]), [D["src1"], D["smpB"], D["winB"]],
     "asx_xcorr_phat_band_f32_dev", (HANDLE, (IN, 0), 0, (IN, 1), N, (IN, 2), 1, B, 0, N, (OUT, 0), (OUT, 1), (OUT, 2), (OUT, 3), None),
     (B,), PHAT_RESULTS),
    ("pool every combination", lambda p: p.xcorr_pool_f32(D["src2"], D["smpB"]), [D["src2"], D["smpB"]],
     "asx_xcorr_pool_f32_dev", (HANDLE, (IN, 0), 2 * N, 2, (IN, 1), N, B, None, None, 0, 2 * B, (OUT, 0), (OUT, 1), (OUT, 2), None),
     (2, B), RESULTS),
    ("pool every combination, rows", lambda p: p.xcorr_pool_f32(D["src2"], D["smpB"], windows=D["win6"]), [D["src2"], D["smpB"], D["win6"]],
     "asx_xcorr_pool_f32_dev", (HANDLE, (IN, 0), 2 * N, 2, (IN, 1), N, B, None, (IN, 2), 1, 2 * B, (OUT, 0), (OUT, 1), (OUT, 2), None),
     (2, B), RESULTS),
    ("pool listed", lambda p: p.xcorr_pool_f32(D["src2"], D["smpB"], D["pairs"].tolist(), D["winB"]),
     [D["src2"], D["smpB"], D["pairs"], D["winB"]],
     "asx_xcorr_pool_f32_dev", (HANDLE, (IN, 0), 2 * N, 2, (IN, 1), N, B, (IN, 2), (IN, 3), 1, 3, (OUT, 0), (OUT, 1), (OUT, 2), None),
     (3,), RESULTS),
    ("pool topk every combination", lambda p: p.xcorr_pool_topk_f32(D["src2"], D["smpB"], 2, 1), [D["src2"], D["smpB"]],
     "asx_xcorr_pool_topk_f32_dev",
     (HANDLE, (IN, 0), 2 * N, 2, (IN, 1), N, B, None, None, 0, 2 * B, 2, 1, (OUT, 0), (OUT, 1), (OUT, 2), None), (2, B, 2), RESULTS),
    ("pool topk listed", lambda p: p.xcorr_pool_topk_f32(D["src2"], D["smpB"], 3, 0, D["pairs"], (-3, 5)),
     [D["src2"], D["smpB"], D["pairs"], D["win1"]], "asx_xcorr_pool_topk_f32_dev",
     (HANDLE, (IN, 0), 2 * N, 2, (IN, 1), N, B, (IN, 2), (IN, 3), 0, 3, 3, 0, (OUT, 0), (OUT, 1), (OUT, 2), None), (3, 3), RESULTS),
]


def check_protocol(fake, inputs, fn, args):
    """-> the device pointers of the results.  Allocations at least 16 bytes on device 0; every input up before the one _dev call,
    which gets `args`; then one sync on the plan's own stream, then the copies back; every pointer freed exactly once, last."""
    kinds = fake.kinds()
    assert kinds.count("dev") == 1 and kinds.count("sync") == 1
    at_dev, at_sync = kinds.index("dev"), kinds.index("sync")
    assert all(e[1] >= 16 and e[2] == 0 for e in fake.log if e[0] == "malloc")
    ups = [i for i, k in enumerate(kinds) if k == "h2d"]
    assert len(ups) == len(inputs) and all(i < at_dev for i in ups)
    where = {}
    for i, a in enumerate(inputs):
        hits = [p for p, blob in fake.uploaded.items() if blob == a.tobytes()]
        assert len(hits) == 1, (i, hits)
        where[(IN, i)] = hits[0]
        assert [e[1] for e in fake.log if e[0] == "malloc" and e[3] == hits[0]] == [max(a.nbytes, 16)]
    _, name, got = fake.log[at_dev]
    assert name == fn and len(got) == len(args), (name, got)
    outs = {}
    for g, want in zip(got, args):
        if isinstance(want, tuple) and want[0] == OUT:
            assert g in fake.ptrs and g not in where.values() and g not in outs.values(), got
            outs[want[1]] = g
        elif isinstance(want, tuple):
            assert g == where[want], (got, args)
        else:
            assert g == want and type(g) is type(want), (got, args)
    assert fake.log[at_sync][1:] == (HANDLE, None) and at_dev < at_sync
    downs = [i for i, k in enumerate(kinds) if k == "d2h"]
    assert len(downs) == len(outs) and all(i > at_sync for i in downs)
    frees = [e[1] for e in fake.log if e[0] == "free"]
    assert sorted(frees) == sorted(fake.ptrs) and len(fake.ptrs) == len(inputs) + len(outs)
    assert kinds[-len(frees):] == ["free"] * len(frees)
    return [outs[j] for j in range(len(outs))]


def filled_from(fake, array, ptr):
    """the array holds what the stand-in's copy back of `ptr` wrote"""
    return bool((np.frombuffer(array.tobytes(), dtype=np.uint8) == fake.ptrs.index(ptr) + 1).all()) and array.size > 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_method_stages_what_the_dev_call_needs(hipxcorr, monkeypatch, case):
    _, call, inputs, fn, args, shape, dtypes = case
    fake = FakeLib()
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    got = call(plan_of(hipxcorr))
    d_out = check_protocol(fake, inputs, fn, args)
    assert isinstance(got, tuple) and len(got) == len(dtypes)
    for array, dtype, ptr in zip(got, dtypes, d_out):
        assert array.shape == shape and array.dtype == dtype
        assert filled_from(fake, array, ptr)
        assert [e[2] for e in fake.log if e[0] == "d2h" and e[1] == ptr] == [array.nbytes]
        assert [e[1] for e in fake.log if e[0] == "malloc" and e[3] == ptr] == [max(array.nbytes, 16)]


def test_windows_with_positions_stage_only_the_windows_that_can_hold_the_start(hipxcorr, monkeypatch):
    """recording of 2N + 8 frames, hop 4: three windows; a start at frame 20 can lie only in window 2 (lag 12), so frames 8 ..
    8 + 2N go up with the one row (12, 12), and windows 0 and 1 come back (0, NaN, -2) without having been correlated"""
    fake = FakeLib()
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    lag, coef, ret = plan_of(hipxcorr).xcorr_windows_f32(D["rec"], D["smp1"], 4, positions=(20, 20))
    inputs = [np.ascontiguousarray(D["rec"][8:8 + 2 * N]), D["smp1"], np.array([[12, 12]], dtype=I64)]
    d_out = check_protocol(fake, inputs, "asx_xcorr_windowed_f32_dev",
                           (HANDLE, (IN, 0), 4, (IN, 1), 0, (IN, 2), 1, 1, (OUT, 0), (OUT, 1), (OUT, 2), None))
    assert (lag.shape, coef.shape, ret.shape) == ((3,),) * 3 and (lag.dtype, coef.dtype, ret.dtype) == RESULTS
    assert lag[:2].tolist() == [0, 0] and np.isnan(coef[:2]).all() and ret[:2].tolist() == [-2, -2]
    for array, ptr in zip((lag, coef, ret), d_out):
        assert filled_from(fake, array[2:], ptr)
    # no window can hold the start: nothing is staged at all
    fake = FakeLib()
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    lag, coef, ret = plan_of(hipxcorr).xcorr_windows_f32(D["rec"], D["smp1"], 4, positions=(100, 120))
    assert fake.log == [] and ret.tolist() == [-2] * 3 and lag.tolist() == [0] * 3 and np.isnan(coef).all()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_failing_dev_call_raises_and_frees_everything(hipxcorr, monkeypatch, case):
    _, call, inputs, fn, args, shape, dtypes = case
    fake = FakeLib(dev_rc=-1)
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    with pytest.raises(hipxcorr.AsxError, match="fake failure"):
        call(plan_of(hipxcorr))
    kinds = fake.kinds()
    assert kinds.count("dev") == 1 and "d2h" not in kinds and "sync" not in kinds
    assert len(fake.ptrs) == len(inputs) + len(dtypes)
    assert sorted(e[1] for e in fake.log if e[0] == "free") == sorted(fake.ptrs)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_failing_third_allocation_raises_and_frees_the_first_two(hipxcorr, monkeypatch, case):
    call = case[1]
    fake = FakeLib(fail_alloc=3)
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    with pytest.raises(hipxcorr.AsxError, match="fake failure"):
        call(plan_of(hipxcorr))
    kinds = fake.kinds()
    assert kinds.count("malloc") == 3 and len(fake.ptrs) == 2 and "dev" not in kinds and "d2h" not in kinds
    assert sorted(e[1] for e in fake.log if e[0] == "free") == sorted(fake.ptrs)


BAD = [
    lambda p: p.xcorr_broadcast_f32(D["src1"][:-1], D["smpB"]),
    lambda p: p.xcorr_broadcast_f32(D["srcB"], D["smpB"][:2]),
    lambda p: p.xcorr_windowed_f32(D["srcB"], D["smpB"], [[0, 1]] * 2),
    lambda p: p.xcorr_windowed_f32(D["srcB"], D["smpB"], (0.5, 1.0)),
    lambda p: p.xcorr_windowed_f32(D["srcB"], D["smpB"], None),
    lambda p: p.xcorr_windowed_f32(D["srcB"][:0], D["smpB"][:0], (0, 1)),
    lambda p: p.xcorr_windows_f32(D["rec"][:2 * N - 1], D["smp1"], 4),
    lambda p: p.xcorr_windows_f32(D["rec"], D["smp1"], 0),
    lambda p: p.xcorr_windows_f32(D["rec"], D["smp1"], 4, positions=(5, 4)),
    lambda p: p.xcorr_topk_f32(D["srcB"], D["smpB"], 0, 0),
    lambda p: p.xcorr_topk_f32(D["srcB"], D["smpB"], True, 0),
    lambda p: p.xcorr_topk_f32(D["srcB"], D["smpB"], 2, -1),
    lambda p: p.xcorr_topk_f32(D["srcB"], D["smpB"], 2, 0, (0, 1, 2)),
    lambda p: p.xcorr_phat_f32(D["srcB"], D["smp1"][:-1]),
    lambda p: p.xcorr_phat_f32(D["srcB"], D["smpB"], [[0, 1]] * 2),
    lambda p: p.xcorr_phat_band_f32(D["srcB"], D["smpB"], 2, 9, (1.5, 2)),
    lambda p: p.xcorr_pool_f32(D["src1"], D["smpB"]),
    lambda p: p.xcorr_pool_f32(D["src2"], D["smpB"], [[0, 1, 2]]),
    lambda p: p.xcorr_pool_f32(D["src2"], D["smpB"], D["pairs"], D["win6"]),
    lambda p: p.xcorr_pool_topk_f32(D["src2"], D["smpB"], 9, 0),
    lambda p: p.xcorr_pool_topk_f32(D["src2"], D["smpB"], 2, 1.0),
    lambda p: p.xcorr_pool_topk_f32(D["src2"], D["smpB"], 2, 0, [[2 ** 31, 0]]),
]


@pytest.mark.parametrize("call", BAD, ids=range(len(BAD)))
def test_a_value_error_touches_nothing(hipxcorr, monkeypatch, call):
    fake = FakeLib()
    monkeypatch.setattr(hipxcorr, "_lib", fake)
    with pytest.raises(ValueError):
        call(plan_of(hipxcorr))
    assert fake.log == []
