"""ratio_gather_kernel (ratio.hip, through dvo_test_ratio_gather): the k-NN modes'
ratio test `m.distance < 0.75 * n.distance`, ordered compaction and keypoint gather
(visual_odometry_v3.py:223-238, KeyPoint_convert v3:355, :358) on the device.

The expected values are Python's rule on the float32 distances DMatch.distance holds:
the product and the compare are double.  The order of the kept matches (ascending
queryIdx) is part of the result: RANSAC's subsets index into the point list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]


def _keypoints(n, seed):
    from droplet_visual_odometry_amd._native import KEYPOINT_DTYPE
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, 640, n).astype(np.float32)
    k["y"] = rng.uniform(0, 480, n).astype(np.float32)
    k["size"] = 3.0
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.uniform(0, 1, n).astype(np.float32)
    k["octave"] = rng.integers(0, 1 << 20, n)
    k["class_id"] = -1
    return k


def _expect(idx, d, kq, kt, ratio=0.75):
    """Python's loop (v3:223-238) on the float32 values DMatch.distance holds."""
    from droplet_visual_odometry_amd._native import DMATCH_DTYPE
    keep = [q for q in range(len(idx)) if float(d[q, 0]) < ratio * float(d[q, 1])]
    pts = np.zeros((len(keep), 4), np.float32)
    m = np.zeros(len(keep), DMATCH_DTYPE)
    if keep:
        t = idx[keep, 0]
        pts[:, 0], pts[:, 1] = kq["x"][keep], kq["y"][keep]
        pts[:, 2], pts[:, 3] = kt["x"][t], kt["y"][t]
        m["queryIdx"], m["trainIdx"], m["distance"] = keep, t, d[keep, 0]
    return keep, pts, m


def _run(gpu_ctx, idx, d, kq, kt, squared=False, ratio=0.75):
    from droplet_visual_odometry_amd import ops
    return ops.test_ratio_gather(idx, d, kq, kt, ratio=ratio, squared=squared, ctx=gpu_ctx)


def _check(gpu_ctx, idx, d_in, d_py, kq, kt, squared=False):
    pts, m, miss = _run(gpu_ctx, idx, d_in, kq, kt, squared)
    keep, epts, em = _expect(idx, d_py, kq, kt)
    assert len(m) == len(keep)
    np.testing.assert_array_equal(pts.view(np.uint32), epts.view(np.uint32))
    np.testing.assert_array_equal(m.view(np.uint8), em.view(np.uint8))
    assert not miss
    return keep


@pytest.mark.parametrize("nq", SIZES)
@pytest.mark.parametrize("case", ["half", "all", "none"])
def test_ratio_gather_random(gpu_ctx, nq, case):
    rng = np.random.default_rng(nq * 7 + len(case))
    nt = max(nq // 2, 3)
    kq, kt = _keypoints(nq + 5, 1), _keypoints(nt, 2)  # more query keypoints than queries is legal
    idx = rng.integers(0, nt, (nq, 2)).astype(np.int32)
    d1 = rng.uniform(10, 500, nq).astype(np.float32)
    scale = {"half": rng.uniform(0.5, 1.0, nq), "all": rng.uniform(0.1, 0.7, nq), "none": rng.uniform(0.8, 1.0, nq)}[case]
    d = np.stack([(d1 * scale).astype(np.float32), d1], 1)
    keep = _check(gpu_ctx, idx, d, d, kq, kt)
    if case == "all":
        assert len(keep) == nq
    elif case == "none":
        assert len(keep) == 0
    elif nq >= 63:
        assert 0 < len(keep) < nq


def test_ratio_gather_rounding_edge(gpu_ctx):
    """d0 = float32(0.75f * d1): Python keeps exactly the queries whose float32 product
    rounded down (about a third); a float32 compare d0 < 0.75f * d1 would keep none."""
    rng = np.random.default_rng(5)
    nq = 4097
    kq, kt = _keypoints(nq, 3), _keypoints(100, 4)
    idx = rng.integers(0, 100, (nq, 2)).astype(np.int32)
    d1 = rng.uniform(0.5, 4.0, nq).astype(np.float32)
    d0 = (np.float32(0.75) * d1).astype(np.float32)
    d = np.stack([d0, d1], 1)
    keep = _check(gpu_ctx, idx, d, d, kq, kt)
    assert 0.2 * nq < len(keep) < 0.45 * nq
    assert not np.any(d0 < np.float32(0.75) * d1)  # what the float32 compare would keep
    # the compare is strict: d0 == 0.75 d1 exactly is rejected
    d = np.tile(np.array([[3.0, 4.0], [6.0, 8.0], [2.9999998, 4.0]], np.float32), (50, 1))
    idx = np.zeros((150, 2), np.int32)
    keep = _check(gpu_ctx, idx, d, d, kq, kt)
    assert keep == list(range(2, 150, 3))


@pytest.mark.parametrize("nq", [65, 1025])
def test_ratio_gather_squared(gpu_ctx, nq):
    """FLANN reports squared L2; DMatch.distance is its float32 square root."""
    rng = np.random.default_rng(nq)
    kq, kt = _keypoints(nq, 5), _keypoints(50, 6)
    idx = rng.integers(0, 50, (nq, 2)).astype(np.int32)
    s1 = rng.integers(1000, 200000, nq).astype(np.float32)
    s0 = np.floor(s1 * rng.uniform(0.3, 0.9, nq)).astype(np.float32)  # ratio of the roots around 0.55 .. 0.95
    sq = np.stack([s0, s1], 1)
    keep = _check(gpu_ctx, idx, sq, np.sqrt(sq), kq, kt, squared=True)
    assert 0 < len(keep) < nq


def test_ratio_gather_missing_second(gpu_ctx):
    rng = np.random.default_rng(9)
    nq = 1500
    kq, kt = _keypoints(nq, 7), _keypoints(40, 8)
    idx = rng.integers(0, 40, (nq, 2)).astype(np.int32)
    d = np.stack([np.full(nq, 1.0, np.float32), np.full(nq, 2.0, np.float32)], 1)
    assert not _run(gpu_ctx, idx, d, kq, kt)[2]
    idx[1234, 1] = -1
    pts, m, miss = _run(gpu_ctx, idx, d, kq, kt)
    assert miss
    # the queries that do have two neighbours are still gathered in order
    np.testing.assert_array_equal(m["queryIdx"], [q for q in range(nq) if q != 1234])


def test_ratio_gather_bad_arguments(gpu_ctx):
    from droplet_visual_odometry_amd._native import DVOError
    kq, kt = _keypoints(4, 1), _keypoints(4, 2)
    idx, d = np.zeros((4, 2), np.int32), np.ones((4, 2), np.float32)
    for bad in (0.0, float("nan")):
        with pytest.raises(DVOError):
            _run(gpu_ctx, idx, d, kq, kt, ratio=bad)
    with pytest.raises(DVOError):
        _run(gpu_ctx, idx, d, kq[:3], kt)  # fewer query keypoints than queries
