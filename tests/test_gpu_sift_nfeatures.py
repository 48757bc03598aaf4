"""SIFT_create(nfeatures = N).detectAndCompute on the GPU (dvo_sift_detect_and_compute_n, the retain
stage of sift.hip, and ops.SiftBatch's group form): OpenCV 4.x's retainBest between
removeDuplicatedSorted and the descriptors.  Every expected value is the oracle's default detection
permuted by oracle.retain_best (sift_nfeatures_cases.expected), compared byte for byte: the kept
keypoints, ties at the boundary included, in libstdc++'s nth_element + partition order, and their
descriptors.  test_sift_nfeatures_host.py checks on the CPU that these inputs cut, tie and permute."""
import ctypes

import numpy as np
import pytest

import sift_nfeatures_cases as sc

pytestmark = pytest.mark.gpu


def _cuts(name):
    return [(n, kept) for nm, n, kept in sc.CUTS if nm == name]


@pytest.mark.parametrize("name", list(sc.FULL))
def test_single_frame_equals_oracle_composition(gpu_ctx, oracle_mod, name):
    """The listed N of the image, then n - 1, n, n + 1 around the list's length n, and 0: from n
    upward (and at 0) nothing is cut and the result is the default call's."""
    from droplet_visual_odometry_amd import ops
    img, full = sc.image(name), sc.FULL[name]
    default = ops.sift_detect_and_compute(img, ctx=gpu_ctx)
    sc.same_features(default, sc.full(oracle_mod, name))
    assert len(default[0]) == full
    for n, kept in _cuts(name):
        got = ops.sift_detect_and_compute(img, ctx=gpu_ctx, nfeatures=n)
        assert len(got[0]) == kept, (n, len(got[0]))
        sc.same_features(got, sc.expected(oracle_mod, name, n))
    sc.same_features(ops.sift_detect_and_compute(img, ctx=gpu_ctx, nfeatures=full - 1),
                     sc.expected(oracle_mod, name, full - 1))
    for n in (full, full + 1, 0):
        sc.same_features(ops.sift_detect_and_compute(img, ctx=gpu_ctx, nfeatures=n), default)


def test_caller_capacity_is_compared_with_the_kept_count(gpu_ctx, oracle_mod):
    """noise at N = 64 keeps 65: cap 64 is DVO_ECAP with *n_out = 65, cap 65 (below the full count
    107) succeeds, and nothing is written past the kept features."""
    from droplet_visual_odometry_amd._native import DVO_ECAP, DVO_EINVAL, DVO_OK, KEYPOINT_DTYPE, ptr
    img = sc.image("noise")
    h, w = img.shape
    lib = gpu_ctx.lib

    def call(nfeatures, cap):
        kps = np.full(80 * KEYPOINT_DTYPE.itemsize, 0xAB, np.uint8)
        desc = np.full((80, 128), -7.0, np.float32)
        n = ctypes.c_int(-1)
        rc = lib.dvo_sift_detect_and_compute_n(gpu_ctx.h, ptr(img), w, h, w, nfeatures, ptr(kps), ptr(desc), cap,
                                               ctypes.byref(n))
        return rc, n.value, kps, desc

    rc, n, kps, desc = call(64, 64)
    assert (rc, n) == (DVO_ECAP, 65)
    assert (kps == 0xAB).all() and (desc == -7.0).all()
    rc, n, kps, desc = call(64, 65)
    assert (rc, n) == (DVO_OK, 65)
    want = sc.expected(oracle_mod, "noise", 64)
    sc.same_features((kps[:65 * KEYPOINT_DTYPE.itemsize].view(KEYPOINT_DTYPE), desc[:65]), want)
    assert (kps[65 * KEYPOINT_DTYPE.itemsize:] == 0xAB).all() and (desc[65:] == -7.0).all()
    rc, n, _, _ = call(-1, 80)
    assert (rc, n) == (DVO_EINVAL, 0)


@pytest.mark.parametrize("name,n", [("noise", 64), ("tiled", 16)])
def test_cv_sift_create_nfeatures(gpu_ctx, oracle_mod, name, n):
    from droplet_visual_odometry_amd import cv
    for make in (cv.SIFT_create, cv.xfeatures2d.SIFT_create):
        kps, desc = make(nfeatures=n).detectAndCompute(sc.image(name), None)
        sc.same_features((kps.array, desc), sc.expected(oracle_mod, name, n))
    kps, desc = cv.SIFT_create().detectAndCompute(sc.image(name), None)
    sc.same_features((kps.array, desc), sc.full(oracle_mod, name))


def _group_frames():
    return np.stack([sc.image(name) for name in sc.GROUP_FRAMES])


@pytest.mark.parametrize("group", [1, 2, 5])
def test_group_equals_single_frame(gpu_ctx, oracle_mod, group):
    """feat_cap 40 is below the full counts 469, 107 and 42 and above every kept count: a group
    detector that cut the list at feat_cap before retain would keep other keypoints."""
    from droplet_visual_odometry_amd import ops
    frames = _group_frames()
    sb = ops.SiftBatch(176, 160, group, ctx=gpu_ctx, nfeatures=sc.GROUP_N)
    for _ in range(2):  # and again on the same handle
        got = sb.detect(frames, feat_cap=40)
        assert tuple(len(k) for k, _ in got) == sc.GROUP_KEPT
        for name, g in zip(sc.GROUP_FRAMES, got):
            sc.same_features(g, sc.expected(oracle_mod, name, sc.GROUP_N))
            sc.same_features(g, ops.sift_detect_and_compute(sc.image(name), ctx=gpu_ctx, nfeatures=sc.GROUP_N))
    sb.close()


def test_group_kept_count_above_feat_cap(gpu_ctx, oracle_mod):
    """feat_cap 16: the frame that keeps 16 is complete; the others report their kept count, hold
    their first 16 kept features, and write nothing past their slot."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ECAP, KEYPOINT_DTYPE, DVOError
    frames, cap, nf = _group_frames(), 16, len(sc.GROUP_FRAMES)
    kps = torch.full((nf + 1, cap, KEYPOINT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    desc = torch.full((nf + 1, cap, 128), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((nf + 1, 2), -3, dtype=torch.int32, device="cuda")
    sb = ops.SiftBatch(176, 160, 2, ctx=gpu_ctx, nfeatures=sc.GROUP_N)
    sb.detect_device(frames, cap, out=(kps, desc, cnt))
    torch.cuda.synchronize()
    kps, desc, cnt = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    np.testing.assert_array_equal(cnt[:nf, 0], sc.GROUP_KEPT)
    assert not cnt[:nf, 1].any()
    for f, name in enumerate(sc.GROUP_FRAMES):
        kw, dw = sc.expected(oracle_mod, name, sc.GROUP_N)
        np.testing.assert_array_equal(kps[f].reshape(-1), kw[:cap].view(np.uint8))
        np.testing.assert_array_equal(desc[f].view(np.uint32), dw[:cap].view(np.uint32))
    assert (kps[nf] == 0xAB).all() and (desc[nf] == -7.0).all() and (cnt[nf] == -3).all()  # behind the last slot
    with pytest.raises(DVOError) as e:
        sb.detect(frames, feat_cap=cap)
    assert e.value.code == DVO_ECAP
    sb.close()


def test_group_default_and_setter(gpu_ctx, oracle_mod):
    """nfeatures = 0 is today's result; set_nfeatures between calls takes effect, both ways."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    frames = _group_frames()
    sb = ops.SiftBatch(176, 160, 3, ctx=gpu_ctx)

    def check(n):
        for name, g in zip(sc.GROUP_FRAMES, sb.detect(frames)):
            sc.same_features(g, sc.expected(oracle_mod, name, n))

    check(0)
    sb.set_nfeatures(sc.GROUP_N)
    check(sc.GROUP_N)
    sb.set_nfeatures(2)
    check(2)
    sb.set_nfeatures(0)
    check(0)
    with pytest.raises(DVOError) as e:
        sb.set_nfeatures(-1)
    assert e.value.code == DVO_EINVAL
    check(0)
    sb.close()


def test_surf_handles_refuse_the_setter(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    K = np.array([[300.0, 0, 88], [0, 300.0, 80], [0, 0, 1]])
    made = []
    for make in (lambda: ops.SurfBatch(176, 160, 2, ctx=gpu_ctx),
                 lambda: KnnFrameStream(176, 160, K, 2, detector="surf", feat_cap=64, ctx=gpu_ctx),
                 lambda: ops.KnnPairStream(176, 160, K, detector="surf", ctx=gpu_ctx)):
        h = make()
        made.append(h)
        with pytest.raises(DVOError) as e:
            h.set_nfeatures(16)
        assert e.value.code == DVO_EINVAL and "SURF" in str(e.value)
    with pytest.raises(DVOError) as e:
        KnnFrameStream(176, 160, K, 2, detector="surf", feat_cap=64, ctx=gpu_ctx, nfeatures=16)
    assert e.value.code == DVO_EINVAL
    for h in made:
        h.close()
