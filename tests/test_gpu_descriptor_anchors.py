"""The float64 anchors of sift_reference.py and surf_reference.py (orientation, descriptor entries, SIFT's
refinement) applied to what the device returns, with no oracle in the loop: the per-call entry points
(ops.sift_detect_and_compute, ops.surf_detect_and_compute) on four cases of detector_cases.py and one
ops.SiftBatch and one ops.SurfBatch detect call over the 96 x 96 stack.  The inputs are detector_cases.py's
seeded numpy images.  Where a frame has more than 64 keypoints, 64 at a fixed stride over the list are
checked, so that every octave stays represented.  Tolerances and what was measured:
sift_reference.check_features, surf_reference.check_features, test_descriptor_anchors.py."""
import numpy as np
import pytest

import detector_cases as dc
import sift_reference as sift_ref
import surf_reference as surf_ref
from test_descriptor_anchors import NO_UNDECIDED, SMOOTH, split_ok

pytestmark = pytest.mark.gpu

PER_CALL = ("ramp_blob_37", "noise_96", "edge_blobs", "anchor")
MAX_KEYPOINTS = 64


def _case(name):
    return next(c for c in dc.cases() if c.name == name)


def _check_sift(name, img, kps, desc, label):
    got = sift_ref.check_features(img, kps, desc, label, max_keypoints=MAX_KEYPOINTS, split_ok=split_ok(name))
    assert len(got["by_split"]) <= (3 if name == "anchor" else 0)  # only the named keypoints of anchor
    assert got["checked"] >= min(_case(name).min_sift, MAX_KEYPOINTS)
    if name in NO_UNDECIDED:
        assert got["undecided"] == 0
    return got


@pytest.mark.parametrize("name", PER_CALL)
def test_sift_detect_and_compute_against_float64(gpu_ctx, name):
    from droplet_visual_odometry_amd import ops
    img = _case(name).img
    kps, desc = ops.sift_detect_and_compute(img, ctx=gpu_ctx)
    got = _check_sift(name, img, kps, desc, f"device sift_detect_and_compute {name}")
    if name == "edge_blobs":
        assert got["saturated"] > 0


@pytest.mark.parametrize("name", PER_CALL)
def test_surf_detect_and_compute_against_float64(gpu_ctx, name):
    from droplet_visual_odometry_amd import ops
    c = _case(name)
    kps, desc = ops.surf_detect_and_compute(c.img, 400.0, ctx=gpu_ctx)
    if c.min_surf == 0:  # edge_blobs: 40 x 30 has no SURF keypoint at 400
        assert len(kps) == 0 and desc.shape == (0, 64)
        return
    got = surf_ref.check_features(c.img, kps, desc, f"device surf_detect_and_compute {name}", smooth=name in SMOOTH,
                                  max_keypoints=MAX_KEYPOINTS)
    assert got["other_window"] <= (1 if name == "anchor" else 0)


def test_sift_batch_against_float64(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    cases = dc.by_size(96, 96)
    sb = ops.SiftBatch(96, 96, 3, ctx=gpu_ctx)
    try:
        got = sb.detect(np.stack([c.img for c in cases]))
    finally:
        sb.close()
    assert len(got) == len(cases)
    octaves = set()
    for c, (kps, desc) in zip(cases, got):
        octaves |= _check_sift(c.name, c.img, kps, desc, f"device SiftBatch {c.name}")["octaves"]
    assert octaves >= {-1, 0, 1}


def test_surf_batch_against_float64(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    cases = dc.by_size(96, 96)
    sb = ops.SurfBatch(96, 96, 3, ctx=gpu_ctx)
    try:
        got = sb.detect(np.stack([c.img for c in cases]), 400.0)
    finally:
        sb.close()
    assert len(got) == len(cases)
    for c, (kps, desc) in zip(cases, got):
        assert len(kps) >= 1, c.name
        res = surf_ref.check_features(c.img, kps, desc, f"device SurfBatch {c.name}", smooth=c.name in SMOOTH,
                                      max_keypoints=MAX_KEYPOINTS)
        assert res["other_window"] == 0
