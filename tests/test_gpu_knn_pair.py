"""The k-NN modes' one-call pair path (D8, dvo_knn_pair_run / ops.KnnPairStream):
visual_odometry_calculations in modes knn_sift, surf and flann runs detect ->
knnMatch(k=2) -> ratio test -> findEssentialMat -> recoverPose in one library call
and then the same host tail as the operator-by-operator path
(visual_odometry_v3.py:384-408).  The two paths must agree bit for bit (4x4s, E,
P_prev, and in flann mode cv's theRNG state after every pair), the record must equal
the oracle chain's, and a failing pair must raise where the operator path raises."""
import os
import sys

import numpy as np
import pytest

from conftest import synth_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"knn_sift": ("sift", "bf"), "flann": ("sift", "flann"), "surf": ("surf", "bf")}


def _v3():
    sys.path.insert(0, os.path.join(ROOT, "droplet_visual_odometry_amd", "dropin"))
    try:
        import visual_odometry_v3 as v3
    finally:
        sys.path.pop(0)
    return v3


def _make(v3, K, tmp_path, mode, slow):
    from droplet_visual_odometry_amd.synth import MARKER_LEN
    d = ", ".join(repr(float(v)) for v in K.ravel())
    y = tmp_path / ("slow.yaml" if slow else "fused.yaml")
    y.write_text(f"camera_matrix:\n  rows: 3\n  cols: 3\n  data: [{d}]\n"
                 "distortion_coefficients:\n  rows: 1\n  cols: 5\n  data: [0.0, 0.0, 0.0, 0.0, 0.0]\n")

    class OperatorByOperator(v3.VisualOdometry):  # an overridden per-pair method disables the fused path
        def compute_current_image_elements(self, input_image):
            return super().compute_current_image_elements(input_image)

    cls = OperatorByOperator if slow else v3.VisualOdometry
    return cls(mode=mode, calibration_file_path=str(y), controlled=True, real_marker_length=MARKER_LEN)


@pytest.mark.parametrize("mode", list(MODES))
def test_fused_equals_operator_path(gpu_ctx, tmp_path, mode):
    from droplet_visual_odometry_amd import cv
    from droplet_visual_odometry_amd.synth import marker_corners
    v3 = _v3()
    frames, K = synth_frames(640, 480, range(6))
    corners = [marker_corners(i, K) for i in range(6)]
    # consecutive pairs (device features reused), a jump (both frames detected), a repeat
    seq = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 5), (0, 5)]
    runs = {}
    for slow in (False, True):  # one pass each, from the same theRNG state
        cv.setRNGSeed(0)
        vo = _make(v3, K, tmp_path, mode, slow)
        hits, inner = [], vo._fused_pair
        vo._fused_pair = lambda p, c: hits.append(inner(p, c)) or hits[-1]
        T, out = vo.robot_curr_position, []
        for a, b in seq:
            try:
                T, rel = vo.visual_odometry_calculations(frames[a], frames[b], T, corners[a], corners[b])
            except cv.error:  # a pair the reference raises on must raise on both paths (rel None in both)
                rel = None
            out.append((rel, T, np.array(vo.essential_matrix), vo.previous_projection_matrix.copy(), cv._the_rng()))
        assert sum(rel is not None for rel, *_ in out) >= 5  # at most the repeated frame's pair may fail
        # the fused pass takes its results from the one-call path, the other pass never does
        assert sum(h is not None for h in hits) == (0 if slow else sum(rel is not None for rel, *_ in out))
        runs[slow] = (vo, out)
    (fused, of), (slow, os_) = runs[False], runs[True]
    assert fused._pair_engine is not None and slow._pair_engine is None
    assert len(of) == len(os_) == len(seq)
    for (rf, Tf, Ef, Pf, sf), (rs, Ts, Es, Ps, ss) in zip(of, os_):
        np.testing.assert_array_equal(rf, rs)
        np.testing.assert_array_equal(Tf, Ts)
        np.testing.assert_array_equal(Ef, Es)
        np.testing.assert_array_equal(Pf, Ps)
        assert sf == ss
    if mode == "flann":
        assert of[-1][4] != of[0][4] != 0xFFFFFFFF  # the state moves with every forest
    assert len(fused.projection_matrix_list) == len(slow.projection_matrix_list) >= 5
    for x, y in zip(fused.projection_matrix_list, slow.projection_matrix_list):
        np.testing.assert_array_equal(x, y)


_ORACLE_FEATURES = {}


def _oracle_features(oracle_mod, detector, i):
    """The oracle's detection of synthetic frame i, computed once."""
    key = (detector, i)
    if key not in _ORACLE_FEATURES:
        frames, _ = synth_frames(640, 480, [i])
        fn = oracle_mod.sift_detect_and_compute if detector == "sift" else oracle_mod.surf_detect_and_compute
        _ORACLE_FEATURES[key] = fn(frames[0])
    return _ORACLE_FEATURES[key]


@pytest.mark.parametrize("mode", list(MODES))
def test_knn_pair_stream_equals_oracle_chain(gpu_ctx, oracle_mod, mode):
    from droplet_visual_odometry_amd import ops
    detector, matcher = MODES[mode]
    frames, K = synth_frames(640, 480, range(3))
    ks = ops.KnnPairStream(640, 480, K, detector=detector, matcher=matcher, ctx=gpu_ctx)
    state = st_o = oracle_mod.THE_RNG_SEED
    for i in range(2):
        rec, state = ks.pair(None if i else frames[0], frames[i + 1], reuse_prev=i > 0, rng_state=state)
        k1, d1 = _oracle_features(oracle_mod, detector, i)
        k2, d2 = _oracle_features(oracle_mod, detector, i + 1)
        if matcher == "flann":
            idx, dist, st_o = oracle_mod.flann_knn(d1, d2, 2, trees=5, checks=50, rng_state=st_o)
            dist = np.sqrt(dist.astype(np.float32))
        else:
            idx, dist = oracle_mod.bf_knn_float(d1, d2, 2, 0)
        keep = [q for q in range(len(d1)) if float(dist[q, 0]) < 0.75 * float(dist[q, 1])]
        p1 = np.stack([k1["x"][keep], k1["y"][keep]], 1).astype(np.float64)
        p2 = np.stack([k2["x"][idx[keep, 0]], k2["y"][idx[keep, 0]]], 1).astype(np.float64)
        E, _, _ = oracle_mod.find_essential(p1, p2, K)
        assert rec["status"] == 0 and rec["n_models"] == 1
        np.testing.assert_array_equal(rec["E"].reshape(3, 3), E)
        assert (rec["n_kp_prev"], rec["n_kp_cur"], rec["n_matches"]) == (len(k1), len(k2), len(keep))
        assert state == st_o
        m = ks.matches()
        np.testing.assert_array_equal(m["queryIdx"], keep)
        np.testing.assert_array_equal(m["trainIdx"], idx[keep, 0])
        np.testing.assert_array_equal(m["imgIdx"], 0)
        np.testing.assert_array_equal(m["distance"].view(np.uint32), dist[keep, 0].astype(np.float32).view(np.uint32))
        det = ops.sift_detect_and_compute if detector == "sift" else ops.surf_detect_and_compute
        for which in (0, 1):
            kg, dg = det(frames[i + which], ctx=gpu_ctx)
            kf, df = ks.features(which)
            np.testing.assert_array_equal(kf.view(np.uint8), kg.view(np.uint8))
            np.testing.assert_array_equal(df.view(np.uint32), dg.view(np.uint32))
    ks.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_fused_failing_pair_raises_like_operator_path(gpu_ctx, tmp_path, mode):
    from droplet_visual_odometry_amd import cv
    from droplet_visual_odometry_amd.synth import marker_corners
    v3 = _v3()
    frames, K = synth_frames(640, 480, range(3))
    blank = np.zeros_like(frames[0])
    c = [marker_corners(i, K) for i in range(3)]
    for slow in (False, True):
        cv.setRNGSeed(0)
        vo = _make(v3, K, tmp_path, mode, slow)
        T, _ = vo.visual_odometry_calculations(frames[0], frames[1], vo.robot_curr_position, c[0], c[1])
        with pytest.raises(cv.error):
            vo.visual_odometry_calculations(frames[1], blank, T, c[1], c[2])
        # and the path recovers: the next good pair (the previous frame's features re-detected)
        T2, _ = vo.visual_odometry_calculations(frames[1], frames[2], T, c[1], c[2])
        st = cv._the_rng()
        if slow:
            np.testing.assert_array_equal(T2, T2_fused)
            assert st == st_fused
        else:
            assert vo._pair_engine is not None
            T2_fused, st_fused = T2, st


def test_knn_pair_stream_refuses_reuse_after_a_failing_pair(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT, DVOError
    frames, K = synth_frames(640, 480, range(3))
    ks = ops.KnnPairStream(640, 480, K, ctx=gpu_ctx)
    with pytest.raises(DVOError):  # nothing to reuse yet
        ks.pair(None, frames[0], reuse_prev=True)
    rec, _ = ks.pair(frames[0], frames[1])
    assert rec["status"] == 0
    rec, _ = ks.pair(None, np.zeros_like(frames[0]), reuse_prev=True)
    assert rec["status"] == DVO_ENOFEAT and rec["n_kp_prev"] > 0 and rec["n_kp_cur"] == 0
    assert len(ks.matches()) == 0
    with pytest.raises(DVOError) as e:  # the failing pair invalidated the cache
        ks.pair(None, frames[2], reuse_prev=True)
    assert e.value.code == -1
    rec, _ = ks.pair(frames[1], frames[2])  # both frames given: works again
    assert rec["status"] == 0
    ks.close()


def test_knn_pair_small_odd_size(gpu_ctx):
    """97 x 61 (the textured generator of test_sift_small_and_odd_sizes): whatever the
    status, and when the pair gets through E equals the per-call operators' on the same images."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EFEWPTS, DVO_ENOFEAT
    w, h = 97, 61
    rng = np.random.default_rng(w * 31 + h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img = np.clip(img.astype(np.int32) // 2 + np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 128, 0, 255)
    a = np.ascontiguousarray(img.astype(np.uint8))
    b = np.ascontiguousarray(np.roll(a, (1, 2), axis=(0, 1)))
    K = np.array([[100.0, 0, 48.0], [0, 100.0, 30.0], [0, 0, 1]])
    ks = ops.KnnPairStream(w, h, K, ctx=gpu_ctx)
    rec, _ = ks.pair(a, b)
    assert rec["status"] in (0, DVO_EFEWPTS, DVO_ENOFEAT)
    k1, d1 = ops.sift_detect_and_compute(a, ctx=gpu_ctx)
    k2, d2 = ops.sift_detect_and_compute(b, ctx=gpu_ctx)
    assert (rec["n_kp_prev"], rec["n_kp_cur"]) == (len(k1), len(k2))
    if rec["status"] == 0:
        idx, dist = ops.bf_knn_float(d1, d2, 2, ops.NORM_L1, ctx=gpu_ctx)
        keep = [q for q in range(len(d1)) if float(dist[q, 0]) < 0.75 * float(dist[q, 1])]
        assert rec["n_matches"] == len(keep)
        p1 = np.stack([k1["x"][keep], k1["y"][keep]], 1).astype(np.float64)
        p2 = np.stack([k2["x"][idx[keep, 0]], k2["y"][idx[keep, 0]]], 1).astype(np.float64)
        E, _ = ops.find_essential_mat(p1, p2, K, ctx=gpu_ctx)
        assert rec["n_models"] == len(E) // 3
        np.testing.assert_array_equal(rec["E"].reshape(3, 3), E[:3])
    ks.close()


@pytest.mark.parametrize("kw", [dict(ratio=0.0), dict(ratio=float("nan")), dict(detector=7), dict(width=4096),
                                dict(max_iters=0)])
def test_knn_pair_bad_config(gpu_ctx, kw):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    args = dict(width=640, height=480, K=np.eye(3), ctx=gpu_ctx)
    args.update(kw)
    with pytest.raises(DVOError) as e:
        ops.KnnPairStream(**args)
    assert e.value.code == DVO_EINVAL
