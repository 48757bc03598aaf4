"""The geometry half of the C ABI away from the reference's default arguments, on the
GPU against the oracle, bit for bit: findEssentialMat over (threshold, prob, maxIters,
m, camera), recoverPose's count, R, t AND output mask over every pick, tie, distance
threshold and input mask, triangulatePoints, the cv2 keyword forms, and the argument
checks.  tests/geom_cases.py builds the cases; tests/test_geometry_cases.py asserts on
the CPU that they reach the regimes named here.

Kernel branches reached (csrc/geometry.hip): ransac_score_kernel's t and fast_ok
(`test_find_essential_grid`, fast_ok false in its 1e-25 cases), ransac_replay_kernel's
niters updates with prob != 0.999 and the one-round schedule's stops at the [0,32) [32,64)
boundaries (`test_find_essential_sizes_and_round_edges`), ransac_finish_kernel's mask and
ENOMODEL exits, pose_count_kernel's mirror shortcut, its own-triangulation branch (zero
components of t) and both mask_in ands, all four picks of pose_pick_kernel and its tie
order (`test_recover_pose_*`), triangulate_kernel (`test_triangulate_points`)."""
import numpy as np
import pytest

import geom_cases as G

pytestmark = pytest.mark.gpu

GRID = [pytest.param(cam, th, pr, th != G.T_ZERO_THRESHOLD, id=f"{cam}-{th:g}-{pr:g}") for cam, th, pr in G.param_grid()]


@pytest.mark.parametrize("cam,threshold,prob,has_model", GRID)
def test_find_essential_grid(gpu_ctx, oracle_mod, cam, threshold, prob, has_model):
    """has_model False: t = (float)(threshold / f)^2 is 0, the division-free Sampson test is off
    (fast_ok false) and no hypothesis has an inlier: E empty, DVO_ENOMODEL."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ENOMODEL, DVOError
    K = G.CAMERAS[cam]
    p1, p2 = G.correspondences(400, K)
    Eo, mo, _ = oracle_mod.find_essential(p1, p2, K, prob, threshold, 1000)
    assert (Eo is not None) == has_model
    if not has_model:
        with pytest.raises(DVOError) as e:
            ops.find_essential_mat(p1, p2, K, prob, threshold, 1000, ctx=gpu_ctx)
        assert e.value.code == DVO_ENOMODEL
    else:
        E, mask = ops.find_essential_mat(p1, p2, K, prob, threshold, 1000, ctx=gpu_ctx)
        np.testing.assert_array_equal(E, Eo)
        np.testing.assert_array_equal(mask.ravel(), mo)


@pytest.mark.parametrize("m", G.M_SIZES)
def test_find_essential_sizes_and_round_edges(gpu_ctx, oracle_mod, m):
    """m across the score chunk and the 16-hypothesis block; maxIters at the round boundaries."""
    from droplet_visual_odometry_amd import ops
    p1, p2 = G.correspondences(m, G.K_SKEW)
    for mi in G.MAX_ITERS:
        Eo, mo, _ = oracle_mod.find_essential(p1, p2, G.K_SKEW, 0.999, 1.0, mi)
        E, mask = ops.find_essential_mat(p1, p2, G.K_SKEW, 0.999, 1.0, mi, ctx=gpu_ctx)
        np.testing.assert_array_equal(E, Eo, err_msg=f"maxIters {mi}")
        np.testing.assert_array_equal(mask.ravel(), mo, err_msg=f"maxIters {mi}")


@pytest.mark.parametrize("m", [0, 1, 4])
def test_find_essential_few_points_status(gpu_ctx, oracle_mod, m):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EFEWPTS, DVOError
    p1, p2 = G.correspondences(8, G.K_SKEW)
    assert oracle_mod.find_essential(p1[:m], p2[:m], G.K_SKEW)[0] is None
    with pytest.raises(DVOError) as e:
        ops.find_essential_mat(p1[:m], p2[:m], G.K_SKEW, ctx=gpu_ctx)
    assert e.value.code == DVO_EFEWPTS


def _pose_equal(got, want, msg):
    assert got[0] == want[0], msg
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[2], want[2], err_msg=msg)
    np.testing.assert_array_equal(got[3].ravel(), want[3].ravel(), err_msg=msg)


@pytest.mark.parametrize("scene", list(G.POSE_SCENES))
def test_recover_pose_scenes(gpu_ctx, oracle_mod, scene):
    """good, R, t and the output mask for every pick, the equal-maximum ties, the all-zero tie
    (small distanceThresh) and the zero-component t, each with every input mask.

    The mask with an input mask is cv::recoverPose's bitwise_and(mask, mask1, mask1): the
    caller's byte values survive (a 0/1 RANSAC mask gives 0/1, not 0/255), and the count is
    countNonZero.  The oracle used to write 255; it was the oracle that contradicted OpenCV."""
    from droplet_visual_odometry_amd import ops
    E, parts, _ = G.POSE_SCENES[scene]
    K = G.K_SKEW
    p1, p2 = G.pose_scene(oracle_mod, E, parts)
    masks = G.pose_masks(len(p1), G.ransac_mask(oracle_mod, p1, p2, K))
    for d in G.DIST_THRESHOLDS:
        for name, mk in masks.items():
            want = oracle_mod.recover_pose(E, p1, p2, K, d, mk)
            got = ops.recover_pose(E, p1, p2, K, d, mk, ctx=gpu_ctx)
            _pose_equal(got, want, f"{scene} distanceThresh {d} mask {name}")


@pytest.mark.parametrize("m", G.POSE_M)
def test_recover_pose_sizes(gpu_ctx, oracle_mod, m):
    """m around pose_count_kernel's block of 256 threads (two per point)."""
    from droplet_visual_odometry_amd import ops
    K = G.K_HD
    n0 = m // 2
    p1, p2 = G.pose_scene(oracle_mod, G.POSE_E, [(3, m - n0)] + ([(0, n0)] if n0 else []), K=K, seed=m)
    mk = G.pose_masks(m, np.ones(m, np.uint8))["bytes"]
    for mask in (None, mk):
        want = oracle_mod.recover_pose(G.POSE_E, p1, p2, K, 50.0, mask)
        got = ops.recover_pose(G.POSE_E, p1, p2, K, 50.0, mask, ctx=gpu_ctx)
        _pose_equal(got, want, f"m {m} mask {mask is not None}")
    assert want[3].shape == (m,)


@pytest.mark.parametrize("kind", G.TRI_KINDS)
def test_triangulate_points(gpu_ctx, oracle_mod, kind):
    from droplet_visual_odometry_amd import ops
    for k in G.TRI_K:
        P1, P2, x1, x2 = G.triangulation_case(kind, k)
        want = oracle_mod.triangulate(P1, P2, x1, x2)
        got = ops.triangulate_points(P1, P2, x1, x2, ctx=gpu_ctx)
        np.testing.assert_array_equal(got, want, err_msg=f"k {k}")


def test_cv_keyword_forms(gpu_ctx, oracle_mod):
    from droplet_visual_odometry_amd import cv, ops
    K = G.K_SKEW
    p1, p2 = G.correspondences(400, K)
    E, mask = cv.findEssentialMat(points1=p1, points2=p2, cameraMatrix=K, method=cv.RANSAC, prob=0.9, threshold=3.0,
                                  maxIters=500)
    Eo, mo = ops.find_essential_mat(p1, p2, K, 0.9, 3.0, 500, ctx=gpu_ctx)
    np.testing.assert_array_equal(E, Eo)
    np.testing.assert_array_equal(mask, mo)
    np.testing.assert_array_equal(E, oracle_mod.find_essential(p1, p2, K, 0.9, 3.0, 500)[0])
    got = cv.recoverPose(E=E, points1=p1, points2=p2, cameraMatrix=K, distanceThresh=6.0, mask=mask)
    _pose_equal(got, ops.recover_pose(E, p1, p2, K, 6.0, mask, ctx=gpu_ctx), "cv.recoverPose")
    _pose_equal(got, oracle_mod.recover_pose(E, p1, p2, K, 6.0, mask), "cv.recoverPose vs oracle")
    assert 0 < got[0] < len(p1)
    # both empty-E statuses: DVO_ENOMODEL (t = 0) and DVO_EFEWPTS
    assert cv.findEssentialMat(p1, p2, cameraMatrix=K, threshold=G.T_ZERO_THRESHOLD) == (None, None)
    assert cv.findEssentialMat(p1[:4], p2[:4], cameraMatrix=K) == (None, None)


def test_geometry_arguments_are_rejected(gpu_ctx):
    """threshold non-finite or <= 0, maxIters < 1, prob outside (0, 1) or non-finite and a
    non-finite distanceThresh are DVO_EINVAL before anything is allocated or launched."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    from droplet_visual_odometry_amd.stream import FrameStream
    K = G.K_SKEW
    p1, p2 = G.correspondences(64, K)
    nan, inf = float("nan"), float("inf")
    bad = [dict(threshold=v) for v in (0.0, -1.0, nan, inf, -inf)] + [dict(max_iters=v) for v in (0, -5)] \
        + [dict(prob=v) for v in (0.0, 1.0, -0.5, nan, inf)]
    for kw in bad:
        with pytest.raises(DVOError) as e:
            ops.find_essential_mat(p1, p2, K, ctx=gpu_ctx, **kw)
        assert e.value.code == DVO_EINVAL, kw
        with pytest.raises(DVOError) as e:
            FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=2, ctx=gpu_ctx, **kw)
        assert e.value.code == DVO_EINVAL, kw
    E = G.POSE_E
    for d in (nan, inf, -inf):
        with pytest.raises(DVOError) as e:
            ops.recover_pose(E, p1, p2, K, d, ctx=gpu_ctx)
        assert e.value.code == DVO_EINVAL, d
        with pytest.raises(DVOError) as e:
            FrameStream(G.W, G.H, K, nfeatures=G.NF, max_frames=2, ctx=gpu_ctx, dist_thresh=d)
        assert e.value.code == DVO_EINVAL, d
