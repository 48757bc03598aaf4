"""Pair failure statuses, non-default stream configurations and caller-capacity paths on the
GPU against the oracle.

One 320x240 batch (tests/geom_cases.py mixed_batch) holds, in order, a normal pair, a pair
with 1..4 matches (ransac_finish_kernel's m < 5 exit: DVO_EFEWPTS, zero E, R, t), one with
exactly 5 (its m == 5 exit: status OK, 3k rows of E, n_models = k > 1, and records_kernel
zeroes R and t), one with >= 6 matches and a model, and one against a blank frame
(DVO_ENOFEAT).  Every record field is compared with oracle.pair_pose; the pose tail must skip
exactly the pairs whose status is not OK or whose n_models is not 1."""
import ctypes

import numpy as np
import pytest

import geom_cases as G
from conftest import synth_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    frames, K = G.mixed_batch()
    return frames, K, G.mixed_reference(oracle_mod)


def _check_records(recs, refs):
    from droplet_visual_odometry_amd import _native
    for p, (r, ref) in enumerate(zip(recs, refs)):
        G.assert_record_equals(r, ref, _native)


def test_mixed_status_batch(gpu_ctx, mixed):
    import torch
    from droplet_visual_odometry_amd import _native
    from droplet_visual_odometry_amd.stream import FrameStream
    frames, K, refs = mixed
    fs = FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=len(frames), ctx=gpu_ctx)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, len(refs))
    assert list(recs["status"]) == [_native.DVO_OK, _native.DVO_EFEWPTS, _native.DVO_OK, _native.DVO_OK,
                                    _native.DVO_ENOFEAT]
    assert recs["n_models"][2] > 1 and list(recs["n_models"][[0, 1, 3, 4]]) == [1, 0, 1, 0]
    _check_records(recs, refs)
    for p, ref in enumerate(refs):
        mg = fs.matches(p)  # distance-sorted (v3:221), as pair_pose's
        np.testing.assert_array_equal(mg["queryIdx"], ref["q"])
        np.testing.assert_array_equal(mg["trainIdx"], ref["t"])
    fs.close()


def test_mixed_status_batch_submit_and_pose_tail(gpu_ctx, oracle_mod, mixed):
    """The same batch pipelined (submit + drain) gives identical records, and the device pose
    tail equals oracle.pose_tail chained on the host over the successful pairs only; a failed
    pair gets the identity T_rel and leaves T_abs and P_prev where they were.  The m == 5 pair
    is status OK with n_models != 1: unsuccessful.  Tolerance as tests/test_gpu_pose_tail.py
    (float64 libm calls on both sides, each <= 1 ulp off): 1e-9 relative."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    from droplet_visual_odometry_amd.synth import MARKER_LEN, marker_corners
    frames, K, refs = mixed
    n = len(refs)
    dev = torch.from_numpy(frames).cuda()
    corners = np.stack([marker_corners(i, K) for i in range(n + 1)])
    dc = torch.from_numpy(corners).cuda()
    fs = FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=len(frames), ctx=gpu_ctx)
    fs.reset_pose()
    rec = fs.process(dev)
    T_rel, T_abs = fs.pose_tail(dc[:-1], dc[1:], MARKER_LEN)
    fs.sync()
    want = FrameStream.records_numpy(rec, n)
    T_rel, T_abs = T_rel.cpu().numpy(), T_abs.cpu().numpy()
    P, T = K @ np.hstack((np.eye(3), np.zeros((3, 1)))), np.eye(4)
    ok = [G.pair_successful(r) for r in refs]
    assert ok == [True, False, False, True, False]
    for p in range(n):
        if ok[p]:
            P, Tr, T = oracle_mod.pose_tail(K, refs[p]["R"], refs[p]["t_unit"], corners[p], corners[p + 1], MARKER_LEN,
                                            P, T)
            np.testing.assert_allclose(T_rel[p], Tr, rtol=1e-9, atol=1e-12)
        else:
            np.testing.assert_array_equal(T_rel[p], np.eye(4))
            np.testing.assert_array_equal(T_abs[p], T_abs[p - 1])
        np.testing.assert_allclose(T_abs[p], T, rtol=1e-9, atol=1e-12)
    r2 = fs.new_records(n)
    torch.cuda.synchronize()
    assert fs.submit(dev, r2, wait_torch=False) == []
    retired = fs.drain()
    fs.sync()
    assert [(t.data_ptr(), k) for t, k in retired] == [(r2.data_ptr(), n)]
    assert FrameStream.records_numpy(r2, n).tobytes() == want.tobytes()
    fs.close()


def _skew_K(K):
    K = K.copy()
    K[1, 1] = K[0, 0] * 1.04
    K[0, 2] += 3.5
    K[1, 2] -= 2.25
    return K


# name -> (config, first frame of the 320x240 synthetic stream, expected statuses of its three pairs).
# At threshold 1e-25 the squared threshold is 0 in float: only points whose Sampson error is exactly
# 0 are inliers.  Frames 8..11 have no model with five of them (every pair DVO_ENOMODEL); frames
# 0..3 have such models in two pairs (the f64 test with fast_ok false finds inliers).
CONFIGS = {
    "loose_prob": (dict(threshold=0.5, prob=0.9), 0, (0, 0, 0)),
    "wide": (dict(threshold=3.0, prob=0.999999, dist_thresh=6.0), 0, (0, 0, 0)),
    "t_zero": (dict(threshold=G.T_ZERO_THRESHOLD), 8, (-6, -6, -6)),
    "t_zero_exact_inliers": (dict(threshold=G.T_ZERO_THRESHOLD), 0, (-6, 0, 0)),
    "no_cross_check": (dict(cross_check=0), 0, (0, 0, 0)),
    "fx_ne_fy": (dict(), 0, (0, 0, 0)),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_stream_configs(gpu_ctx, oracle_mod, name):
    """Three pairs of the 320x240 synthetic stream under a non-default dvo_stream_config, through
    process() (the batched rounds) and through stream.pair() (the fused per-call path, one
    round): every record equals the oracle's pair_pose with the same arguments."""
    import torch
    from droplet_visual_odometry_amd import _native, ops
    from droplet_visual_odometry_amd.stream import FrameStream
    kw, first, statuses = CONFIGS[name]
    assert _native.DVO_ENOMODEL == -6
    frames, K = synth_frames(G.W, G.H, range(first, first + 4))
    if name == "fx_ne_fy":
        K = _skew_K(K)
        assert K[0, 0] != K[1, 1]
    refs, kp = [], None
    for p in range(3):
        ref = G.pair_reference(oracle_mod, frames[p], frames[p + 1], K, kp_prev=kp, **kw)
        kp = (ref["kp_cur"], ref["desc_cur"])
        refs.append(ref)
    fs = FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=4, ctx=gpu_ctx, **kw)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, 3)
    fs.close()
    _check_records(recs, refs)
    assert tuple(recs["status"]) == statuses
    if name.startswith("t_zero"):
        assert list(recs["ransac_iters"]) == [1000] * 3
    ps = ops.PairStream(G.W, G.H, K, nfeatures=G.NF, ctx=gpu_ctx, **kw)
    for p in range(3):
        r = ps.pair(frames[p], frames[p + 1], reuse_prev=False)
        G.assert_record_equals(r, refs[p], _native)
        for f in recs.dtype.names:
            if f != "n_hypotheses":  # the schedules differ in how far the rounds overshoot
                np.testing.assert_array_equal(r[f], recs[p][f], err_msg=f"pair {p} {f}")
    ps.close()


GUARD = 0xA5


def test_caller_capacity(gpu_ctx, oracle_mod):
    """Capacity one below the needed size: DVO_ECAP, the needed count in the out-parameter
    (dvo_stream_get_pyramid has none), the guard-filled output untouched; the exact capacity
    succeeds with the normal result."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import (DMATCH_DTYPE, DVO_ECAP, DVO_OK, KEYPOINT_DTYPE, orb_params, ptr)
    from droplet_visual_odometry_amd.plan import level_sizes
    from droplet_visual_odometry_amd.stream import FrameStream
    lib, h = gpu_ctx.lib, gpu_ctx.h
    frames, K = synth_frames(G.W, G.H, range(2))
    img = np.ascontiguousarray(frames[0])
    kw, dw = ops.detect_and_compute(img, G.NF, ctx=gpu_ctx)
    n = len(kw)
    assert n > 10
    prm = orb_params(nfeatures=G.NF)

    def detect(cap):
        kps = np.full(n, GUARD, np.uint8).repeat(KEYPOINT_DTYPE.itemsize).view(KEYPOINT_DTYPE)
        desc = np.full((n, 32), GUARD, np.uint8)
        cnt = ctypes.c_int(-1)
        rc = lib.dvo_orb_detect_and_compute(h, ctypes.byref(prm), ptr(img), G.W, G.H, G.W, ptr(kps), ptr(desc), cap,
                                            ctypes.byref(cnt))
        return rc, cnt.value, kps, desc

    rc, cnt, kps, desc = detect(n - 1)
    assert (rc, cnt) == (DVO_ECAP, n)
    assert np.all(kps.view(np.uint8) == GUARD) and np.all(desc == GUARD)
    rc, cnt, kps, desc = detect(n)
    assert (rc, cnt) == (DVO_OK, n)
    np.testing.assert_array_equal(kps.view(np.uint8), kw.view(np.uint8))
    np.testing.assert_array_equal(desc, dw)

    _, d1 = ops.detect_and_compute(np.ascontiguousarray(frames[1]), G.NF, ctx=gpu_ctx)
    mw = ops.bf_match(dw, d1, 1, ctx=gpu_ctx)
    m = len(mw)
    assert 10 < m < len(dw)

    def match(cap):
        out = np.full(m * DMATCH_DTYPE.itemsize, GUARD, np.uint8).view(DMATCH_DTYPE)
        cnt = ctypes.c_int(-1)
        rc = lib.dvo_bf_match_hamming(h, ptr(dw), len(dw), ptr(d1), len(d1), 1, ptr(out), cap, ctypes.byref(cnt))
        return rc, cnt.value, out

    rc, cnt, out = match(m - 1)
    assert (rc, cnt) == (DVO_ECAP, m) and np.all(out.view(np.uint8) == GUARD)
    rc, cnt, out = match(m)
    assert (rc, cnt) == (DVO_OK, m)
    np.testing.assert_array_equal(out, mw)

    fs = FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=2, ctx=gpu_ctx)
    fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    kf, df = fs.features(1)
    nf = len(kf)

    def features(cap):
        kps = np.full(nf * KEYPOINT_DTYPE.itemsize, GUARD, np.uint8).view(KEYPOINT_DTYPE)
        desc = np.full((nf, 32), GUARD, np.uint8)
        cnt = ctypes.c_int(-1)
        rc = lib.dvo_stream_get_features(fs.h, 1, ptr(kps), ptr(desc), cap, ctypes.byref(cnt))
        return rc, cnt.value, kps, desc

    rc, cnt, kps, desc = features(nf - 1)
    assert (rc, cnt) == (DVO_ECAP, nf)
    assert np.all(kps.view(np.uint8) == GUARD) and np.all(desc == GUARD)
    rc, cnt, kps, desc = features(nf)
    assert (rc, cnt) == (DVO_OK, nf)
    np.testing.assert_array_equal(kps.view(np.uint8), kf.view(np.uint8))
    np.testing.assert_array_equal(desc, df)

    ms = fs.matches(0)
    nm = len(ms)
    assert nm > 10

    def matches(cap):
        out = np.full(nm * DMATCH_DTYPE.itemsize, GUARD, np.uint8).view(DMATCH_DTYPE)
        cnt = ctypes.c_int(-1)
        rc = lib.dvo_stream_get_matches(fs.h, 0, ptr(out), cap, ctypes.byref(cnt))
        return rc, cnt.value, out

    rc, cnt, out = matches(nm - 1)
    assert (rc, cnt) == (DVO_ECAP, nm) and np.all(out.view(np.uint8) == GUARD)
    rc, cnt, out = matches(nm)
    assert (rc, cnt) == (DVO_OK, nm)
    np.testing.assert_array_equal(out, ms)

    lw, lh = level_sizes(G.W, G.H)[2]
    want = fs.pyramid(1, 2)
    np.testing.assert_array_equal(want, oracle_mod.pyramid(frames[1])[2])
    buf = np.full(lw * lh, GUARD, np.uint8)
    assert lib.dvo_stream_get_pyramid(fs.h, 1, 2, 0, ptr(buf), lw * lh - 1) == DVO_ECAP
    assert np.all(buf == GUARD)
    assert lib.dvo_stream_get_pyramid(fs.h, 1, 2, 0, ptr(buf), lw * lh) == DVO_OK
    np.testing.assert_array_equal(buf.reshape(lh, lw), want)
    fs.close()
