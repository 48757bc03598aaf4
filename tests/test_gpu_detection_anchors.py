"""The detection anchors of test_detection_anchors.py (sift_reference.DetectionModel, surf_reference.FastHessian,
orb_reference's resize, blur and definition-FAST) applied to what the device returns, with no oracle in the
loop: which keypoints exist is held to the models directly.

SIFT and SURF: the per-call entry points (ops.sift_detect_and_compute, ops.surf_detect_and_compute) on four
cases of detector_cases.py -- edge_blobs (the edge test), noise_96 (contrast and interpolation rejections),
anchor (octaves -1 to 1), surf_blobs_40 (SURF's layers larger than the image) -- and on
test_detection_anchors.wide_blobs (SIFT octaves 2 and 3, SURF octave 2), and one ops.SiftBatch and one
ops.SurfBatch call over the 96 x 96 stack, which runs the group kernels with their grid-stride loops.
ORB: one FrameStream.process of two frames and ops.detect_and_compute, in both OpenCV semantics, on 190 x 131
noise and 333 x 211 5-pixel blocks (seven levels; both sizes cross the strip and band seams of the FAST kernel,
test_gpu_fast_classify.py).  The stream's levels (fs.pyramid) are held to the resize anchor and the blur anchor,
definition-FAST runs on them, and both entry points' keypoints are held to its positions.

The model work is CPU numpy; bounds and what was measured: the reference modules and test_detection_anchors.py."""
import numpy as np
import pytest

import detector_cases as dc
import orb_reference as orb_ref
import sift_reference as sift_ref
import surf_reference as surf_ref
from test_detection_anchors import NF, SEMANTICS, UNDECIDED_CAP, case, surf_thresholds
from test_gpu_fast_classify import edge_image, noise_image

pytestmark = pytest.mark.gpu

PER_CALL = ("edge_blobs", "noise_96", "anchor", "surf_blobs_40", "wide_blobs")


def _check_sift(c, kps, label):
    r = sift_ref.check_detection(c.img, kps, label)
    assert not r["bad"], (label, r["missing"][:6], r["unexplained"][:6])
    assert r["present"] >= 1
    return r


def _check_surf(c, kps, threshold, label):
    r = surf_ref.check_detection(c.img, kps, threshold, label)
    assert not r["bad"], (label, r["missing"][:6], r["unexplained"][:6])
    assert r["worst_pos"] <= 1.0 and r["worst_resp"] <= 1.0
    if (c.w, c.h) == (40, 30):
        assert r["layers_skipped"] == 14 and (len(kps) > 0) == (c.name == "surf_blobs_40")
    return r


def test_sift_detect_and_compute_keypoint_set(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    cells = undecided = 0
    octaves = set()
    for name in PER_CALL:
        c = case(name)
        kps, _ = ops.sift_detect_and_compute(c.img, ctx=gpu_ctx)
        r = _check_sift(c, kps, f"device sift_detect_and_compute {name}")
        cells += r["cells"]
        undecided += r["undecided_returned"]
        octaves |= {cell[0] for cell in sift_ref.keypoint_cells(kps)}
    assert octaves >= {-1, 0, 1, 2, 3}
    assert undecided <= UNDECIDED_CAP * cells, (undecided, cells)


def test_surf_detect_and_compute_keypoint_set(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    total = undecided = 0
    octaves = set()
    for name in PER_CALL:
        c = case(name)
        for t in surf_thresholds(c):
            kps, _ = ops.surf_detect_and_compute(c.img, t, ctx=gpu_ctx)
            r = _check_surf(c, kps, t, f"device surf_detect_and_compute {name}")
            total += len(kps)
            undecided += r["by_undecided"]
            octaves |= set(int(o) for o in kps["octave"])
    assert octaves >= {0, 1, 2}
    assert undecided <= UNDECIDED_CAP * total, (undecided, total)


def test_sift_batch_keypoint_set(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    cases = dc.by_size(96, 96)
    sb = ops.SiftBatch(96, 96, 3, ctx=gpu_ctx)
    try:
        got = sb.detect(np.stack([c.img for c in cases]))
    finally:
        sb.close()
    assert len(got) == len(cases)
    cells = undecided = 0
    for c, (kps, _) in zip(cases, got):
        r = _check_sift(c, kps, f"device SiftBatch {c.name}")
        cells += r["cells"]
        undecided += r["undecided_returned"]
    assert undecided <= UNDECIDED_CAP * cells, (undecided, cells)


def test_surf_batch_keypoint_set(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    cases = dc.by_size(96, 96)
    sb = ops.SurfBatch(96, 96, 3, ctx=gpu_ctx)
    try:
        got = sb.detect(np.stack([c.img for c in cases]), 400.0)
    finally:
        sb.close()
    assert len(got) == len(cases)
    total = undecided = 0
    for c, (kps, _) in zip(cases, got):
        assert len(kps) >= 1, c.name
        r = _check_surf(c, kps, 400.0, f"device SurfBatch {c.name}")
        total += len(kps)
        undecided += r["by_undecided"]
    assert undecided <= UNDECIDED_CAP * total, (undecided, total)


ORB_IMAGES = {(190, 131): lambda: np.stack([noise_image(190, 131, 128, 7), noise_image(190, 131, 128, 8)]),
              (333, 211): lambda: np.stack([edge_image(333, 211, 5, 5), edge_image(333, 211, 5, 6)])}


@pytest.mark.parametrize("opencv", SEMANTICS)
@pytest.mark.parametrize("w,h", sorted(ORB_IMAGES))
def test_orb_levels_and_keypoints(gpu_ctx, w, h, opencv):
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd.plan import features_per_level
    from droplet_visual_odometry_amd.stream import FrameStream
    frames = ORB_IMAGES[(w, h)]()
    quota = np.array(features_per_level(NF))
    K = np.array([[w, 0, w / 2], [0, w, h / 2], [0, 0, 1.0]])
    fs = FrameStream(w, h, K, nfeatures=NF, max_frames=2, ctx=gpu_ctx, opencv=opencv)
    try:
        dev = torch.from_numpy(frames).cuda()
        fs.process(dev)
        fs.sync()
        # level 0 is the input frame itself; the blurred levels are computed from the frames, which `dev` keeps alive
        levels = [[frames[f]] + [fs.pyramid(f, l) for l in range(1, 8)] for f in range(2)]
        blurred = [[fs.pyramid(f, l, blurred=True) for l in range(8)] for f in range(2)]
        feats = [fs.features(f)[0] for f in range(2)]
    finally:
        fs.close()
    reached = set()
    for f in range(2):
        label = f"device FrameStream {w}x{h} frame {f}"
        assert [L.shape for L in levels[f]] == [orb_ref.level_shape(w, h, l) for l in range(8)]
        assert orb_ref.check_pyramid(levels[f], opencv, label) <= 0.5 + orb_ref.RESIZE_TERM[opencv]
        assert orb_ref.check_blur(levels[f], blurred[f], label) <= orb_ref.BLUR_BOUND
        want = orb_ref.orb_positions(levels[f])
        n = np.array([len(p) for p in want])
        print(f"{label} ({opencv}): definition-FAST per level {n.tolist()} (quota {quota.tolist()})")
        assert (n < quota).all(), (label, n, quota)
        assert orb_ref.keypoint_positions(feats[f]) == want, label
        reached |= set(np.flatnonzero(n).tolist())
    if (w, h) == (333, 211):
        assert reached >= set(range(7))
    kps, _ = ops.detect_and_compute(frames[0], NF, opencv=opencv, ctx=gpu_ctx)
    assert orb_ref.keypoint_positions(kps) == orb_ref.orb_positions(levels[0]), f"device detect_and_compute {w}x{h}"
