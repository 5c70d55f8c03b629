"""Strided batches: one track correlated against many (asx_xcorr_strided_f32_dev, include/audiosync/xcorr_hip.h).

Every pair must come back BIT FOR BIT as asx_xcorr_batch_f32_dev returns it on the materialised contiguous pairs, on the same
plan, and must agree with the float64 oracle (lag and ret exactly, coefficient within 1e-5).  Covered: a broadcast source at the
six production lengths in both Pearson forms, a broadcast sample, overlapping windows of one long recording, several launch
groups (one and two stream lanes, the packed decomposition), a length outside the tuned table, overflowing pairs (second look,
asynchronous mode), both strides 0, a contiguous call behind a broadcast one, and the layout rule of the real-column plans."""
import numpy as np
import pytest

import oracle
from util import asx

COEF_TOL = 1e-5
PRODUCTION = [144000, 288000, 480000, 720000, 960000, 1440000]

gpu = pytest.mark.gpu


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


def planted_samples(src, n, rng, offsets, signs, noise):
    """samples cut from the (circular) source at `offsets`, times `signs`, plus Gaussian noise of the given relative levels"""
    sd = float(np.std(src)) or 1.0
    out = []
    for off, sg, nz in zip(offsets, signs, noise):
        idx = (off + np.arange(n)) % (2 * n)
        out.append((sg * src[idx] + nz * sd * rng.standard_normal(n)).astype(np.float32))
    return np.stack(out)


def outputs(torch, batch):
    return (torch.full((batch,), -99, dtype=torch.int64, device="cuda"), torch.full((batch,), 7.0, dtype=torch.float64, device="cuda"),
            torch.full((batch,), 7, dtype=torch.int32, device="cuda"))


def strided(plan, torch, d_src, ss, d_smp, ms, batch):
    lag, coef, ret = outputs(torch, batch)
    torch.cuda.synchronize()
    plan.xcorr_strided_dev(d_src.data_ptr(), ss, d_smp.data_ptr(), ms, batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr())
    plan.sync()
    return lag.cpu().numpy(), coef.cpu().numpy(), ret.cpu().numpy()


def contiguous(plan, torch, src2, smp2):
    batch = smp2.shape[0]
    d_src = torch.from_numpy(np.ascontiguousarray(src2)).cuda()
    d_smp = torch.from_numpy(np.ascontiguousarray(smp2)).cuda()
    lag, coef, ret = outputs(torch, batch)
    torch.cuda.synchronize()
    plan.xcorr_batch_dev(d_src.data_ptr(), d_smp.data_ptr(), batch, lag.data_ptr(), coef.data_ptr(), ret.data_ptr())
    plan.sync()
    return lag.cpu().numpy(), coef.cpu().numpy(), ret.cpu().numpy()


def same_bits(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (x, y)


def check_oracle(src2, smp2, res):
    lag, coef, ret = res
    for i in range(smp2.shape[0]):
        o_ret, o_lag, o_coef = oracle.cross_correlation(src2[i], smp2[i])
        assert (int(ret[i]), int(lag[i])) == (o_ret, o_lag), (i, ret[i], lag[i], o_ret, o_lag)
        assert abs(float(coef[i]) - o_coef) < COEF_TOL, (i, coef[i], o_coef)


def compare(plan, torch, src2, smp2, ss, ms, d_src, d_smp):
    """strided call vs contiguous call on the materialised pairs (bits, counters) and vs the oracle"""
    batch = smp2.shape[0]
    m0, r0, v0 = plan.pearson_modes(), plan.peak_repairs(), plan.peak_overflows()
    got = strided(plan, torch, d_src, ss, d_smp, ms, batch)
    m1, r1, v1 = plan.pearson_modes(), plan.peak_repairs(), plan.peak_overflows()
    ref = contiguous(plan, torch, src2, smp2)
    m2, r2, v2 = plan.pearson_modes(), plan.peak_repairs(), plan.peak_overflows()
    same_bits(got, ref)
    assert [b - a for a, b in zip(m0, m1)] == [b - a for a, b in zip(m1, m2)], (m0, m1, m2)
    assert (r1 - r0, v1 - v0) == (r2 - r1, v2 - v1)
    check_oracle(src2, smp2, got)
    return got, [b - a for a, b in zip(m0, m1)]


@gpu
@pytest.mark.parametrize("n", PRODUCTION)
def test_broadcast_source_at_production_lengths(mod, torch, n):
    rng = np.random.default_rng(n)
    src, _, _ = oracle.synth_pair(77, 1, n, 1)
    offsets = [0, 1234, n // 2, n - 3, n + 5, 3 * n // 2, 2 * n - 7, 2 * n - n // 3]
    signs = [1, -1, 1, -1, 1, 1, -1, 1]
    noise = [0.0, 0.3, 1.0, 0.1, 3.0, 30.0, 0.5, 60.0]   # the noisiest pairs have coefficients of a few hundredths
    smp2 = planted_samples(src, n, rng, offsets, signs, noise)
    b = smp2.shape[0]
    src2 = np.broadcast_to(src, (b, 2 * n))
    d_src = torch.from_numpy(src).cuda()
    d_smp = torch.from_numpy(smp2).cuda()
    with mod.Plan(n, b, 0) as plan:
        assert plan.layout == "real-column"
        modes = []
        for spectral in (True, False):
            plan.set_pearson(spectral)
            _, m = compare(plan, torch, src2, smp2, 0, n, d_src, d_smp)
            modes.append(m)
        assert sum(modes[0]) == b


@gpu
@pytest.mark.parametrize("n", [144000, 1440000])
def test_broadcast_sample(mod, torch, n):
    rng = np.random.default_rng(n + 1)
    srcs = np.stack([oracle.synth_pair(91, k, n, 1)[0] for k in range(5)])
    smp = srcs[2][n // 3:n // 3 + n].copy()   # the sample was cut from candidate 2
    smp2 = np.broadcast_to(smp, (5, n))
    d_src = torch.from_numpy(srcs).cuda()
    d_smp = torch.from_numpy(smp).cuda()
    with mod.Plan(n, 5, 0) as plan:
        got, _ = compare(plan, torch, srcs, smp2, 2 * n, 0, d_src, d_smp)
    assert int(np.argmax(np.abs(got[1]))) == 2 and abs(got[1][2] - 1.0) < 1e-6


@gpu
def test_windows_with_hop_n(mod, torch):
    n = 480000
    rng = np.random.default_rng(5)
    rec = (rng.standard_normal(6 * n)).astype(np.float32)
    at = 3 * n + 12345                       # inside windows 2 ([2N, 4N)) and 3 ([3N, 5N))
    clip = (rec[at:at + n] + 0.2 * rng.standard_normal(n)).astype(np.float32)
    nwin = (6 * n - 2 * n) // n + 1
    wins = np.stack([rec[k * n:k * n + 2 * n] for k in range(nwin)])
    clips = np.broadcast_to(clip, (nwin, n))
    d_rec = torch.from_numpy(rec).cuda()
    d_clip = torch.from_numpy(clip).cuda()
    with mod.Plan(n, nwin, 0) as plan:
        got, _ = compare(plan, torch, wins, clips, n, 0, d_rec, d_clip)
        host = plan.xcorr_windows_f32(rec, clip, n)
    same_bits(got, host)
    best = int(np.argmax(np.abs(got[1])))
    assert best in (2, 3) and got[1][best] > 0.9, got


@gpu
@pytest.mark.parametrize("env", [{}, {"ASX_LANES": "2"}, {"ASX_LAYOUT": "packed"}], ids=["one-lane", "two-lanes", "packed"])
def test_several_launch_groups(mod, torch, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = 144000
    rng = np.random.default_rng(11)
    src, _, _ = oracle.synth_pair(12, 0, n, 1)
    b = 9
    smp2 = planted_samples(src, n, rng, [(k * 37717) % (2 * n) for k in range(b)], [1, -1] * 5, [0.2 * k for k in range(b)])
    d_src = torch.from_numpy(src).cuda()
    d_smp = torch.from_numpy(smp2).cuda()
    with mod.Plan(n, 3, 0) as plan:
        assert plan.group == 3
        assert plan.layout == ("packed" if env.get("ASX_LAYOUT") else "real-column")
        compare(plan, torch, np.broadcast_to(src, (b, 2 * n)), smp2, 0, n, d_src, d_smp)
        # and a broadcast sample over several groups
        srcs = np.stack([np.roll(src, 1000 * k) for k in range(b)])
        compare(plan, torch, srcs, np.broadcast_to(smp2[0], (b, n)), 2 * n, 0, torch.from_numpy(srcs).cuda(), d_smp[0])


@gpu
def test_length_outside_the_tuned_table(mod, torch):
    n = 100003
    rng = np.random.default_rng(3)
    src, _, _ = oracle.synth_pair(4, 0, n, 1)
    smp2 = planted_samples(src, n, rng, [17, n + 3, 2 * n - 9], [1, -1, 1], [0.1, 0.5, 2.0])
    with mod.Plan(n, 3, 0) as plan:
        assert plan.layout == "packed"
        compare(plan, torch, np.broadcast_to(src, (3, 2 * n)), smp2, 0, n, torch.from_numpy(src).cuda(), torch.from_numpy(smp2).cuda())
        srcs = np.stack([np.roll(src, 7 * k) for k in range(3)])
        compare(plan, torch, srcs, np.broadcast_to(smp2[1], (3, n)), 2 * n, 0, torch.from_numpy(srcs).cuda(),
                torch.from_numpy(smp2[1].copy()).cuda())


@gpu
def test_overflowing_pairs_with_a_broadcast_source(mod, torch):
    n = 48000
    base = np.array([3, -1, 2, 0, -2, 1, -3, 0], dtype=np.float32)
    per = np.tile(base, 2 * n // 8)            # 2N/8 exactly tied peaks: every pair against it overflows
    rng = np.random.default_rng(8)
    smp2 = np.stack([per[:n], per[8:n + 8], per[3:n + 3], (rng.standard_normal(n)).astype(np.float32)])
    b = smp2.shape[0]
    src2 = np.broadcast_to(per, (b, 2 * n))
    d_src = torch.from_numpy(per).cuda()
    d_smp = torch.from_numpy(smp2).cuda()
    with mod.Plan(n, b, 0) as plan:
        assert plan.peak_capacity < 2 * n
        o0, r0 = plan.peak_overflows(), plan.peak_repairs()
        got = strided(plan, torch, d_src, 0, d_smp, n, b)
        over = plan.peak_overflows() - o0
        assert over >= 3 and plan.peak_repairs() - r0 == over
        # pair 0 is the existing suite's case: every 8th lag ties exactly, the smallest wins, as in the reference's scan
        o_ret, o_lag, o_coef = oracle.cross_correlation(per, per[:n])
        assert (int(got[2][0]), int(got[0][0]), float(got[1][0])) == (o_ret, o_lag, 1.0)
        for i in range(1, b):
            o_ret, o_lag, o_coef, _, margin = oracle.cross_correlation(src2[i], smp2[i], want_results=True)
            assert int(got[2][i]) == o_ret and abs(float(got[1][i]) - o_coef) < COEF_TOL, (i, got, o_coef)
            if margin > 1.0 + 1e-12:
                assert int(got[0][i]) == o_lag
            else:   # exact ties: the oracle's own float64 rounding picks among them
                assert (int(got[0][i]) - o_lag) % 8 == 0
        same_bits(got, contiguous(plan, torch, src2, smp2))
        # asynchronous mode: no second look, the overflowed pairs come back marked
        plan.set_exact(False)
        o1, r1 = plan.peak_overflows(), plan.peak_repairs()
        lag, coef, ret = strided(plan, torch, d_src, 0, d_smp, n, b)
        assert plan.peak_overflows() - o1 == over and plan.peak_repairs() == r1
        assert int((ret == 1).sum()) == over and ret[0] == 1
        same_bits((lag, coef, ret), contiguous(plan, torch, src2, smp2))
        plan.set_exact(True)


@gpu
@pytest.mark.parametrize("n", [144000, 100003])
def test_both_strides_zero(mod, torch, n):
    src, smp, _ = oracle.synth_pair(21, 0, n, 1)
    with mod.Plan(n, 2, 0) as plan:
        compare(plan, torch, np.broadcast_to(src, (4, 2 * n)), np.broadcast_to(smp, (4, n)), 0, 0,
                torch.from_numpy(src).cuda(), torch.from_numpy(smp).cuda())
        lag, coef, ret = plan.xcorr_broadcast_f32(src, smp)
        assert lag.shape == (1,)


@gpu
def test_contiguous_call_after_a_broadcast_call(mod, torch):
    n = 288000
    rng = np.random.default_rng(2)
    src, _, _ = oracle.synth_pair(31, 0, n, 1)
    smp2 = planted_samples(src, n, rng, [5, n + 11, 2 * n - 100], [1, -1, 1], [0.1, 1.0, 0.3])
    other = np.stack([oracle.synth_pair(32, k, n, 1)[0] for k in range(3)])
    other_smp = np.stack([oracle.synth_pair(32, k, n, 1)[1] for k in range(3)])
    with mod.Plan(n, 3, 0) as fresh:
        want = contiguous(fresh, torch, other, other_smp)
    with mod.Plan(n, 3, 0) as plan:
        strided(plan, torch, torch.from_numpy(src).cuda(), 0, torch.from_numpy(smp2).cuda(), n, 3)
        same_bits(contiguous(plan, torch, other, other_smp), want)
        # the host helpers: 1-D / 2-D arguments
        same_bits(plan.xcorr_broadcast_f32(src, smp2), contiguous(plan, torch, np.broadcast_to(src, (3, 2 * n)), smp2))


@gpu
def test_layout_rule_of_real_column_plans(mod, torch):
    n = 144000
    src, smp, _ = oracle.synth_pair(1, 0, n, 1)
    d_src = torch.from_numpy(np.concatenate([src, src])).cuda()
    d_smp = torch.from_numpy(np.concatenate([smp, smp])).cuda()
    with mod.Plan(n, 2, 0) as plan:
        assert plan.layout == "real-column"
        cases = [(d_src.data_ptr() + 4, 0, d_smp.data_ptr(), n, "aligned"),
                 (d_src.data_ptr(), 0, d_smp.data_ptr() + 8, 0, "aligned"),
                 (d_src.data_ptr(), 6, d_smp.data_ptr(), 0, "multiples of 4"),
                 (d_src.data_ptr(), 0, d_smp.data_ptr(), n + 2, "multiples of 4")]
        for ps, ss, pm, ms, msg in cases:
            lag, coef, ret = outputs(torch, 2)
            torch.cuda.synchronize()
            with pytest.raises(mod.AsxError, match=msg):
                plan.xcorr_strided_dev(ps, ss, pm, ms, 2, lag.data_ptr(), coef.data_ptr(), ret.data_ptr())
            torch.cuda.synchronize()
            assert (lag == -99).all() and (coef == 7.0).all() and (ret == 7).all()
        # a stride that is a multiple of 4 but shorter than a track is fine (overlapping pairs)
        strided(plan, torch, d_src, 4, d_smp, 0, 2)
    with mod.Plan(100003, 1, 0) as packed:   # packed plans take any float alignment and stride
        s2, m2, _ = oracle.synth_pair(2, 0, 100003, 1)
        buf = np.concatenate([np.zeros(1, np.float32), s2])
        d_buf = torch.from_numpy(buf).cuda()
        d_m = torch.from_numpy(m2).cuda()
        got = strided(packed, torch, d_buf[1:], 3, d_m, 0, 1)
        same_bits(got, contiguous(packed, torch, s2[None], m2[None]))
