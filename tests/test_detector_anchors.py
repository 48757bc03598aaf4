"""First-principles anchors of the SIFT and SURF oracles (oracle/sift.cpp, oracle/surf.cpp).  Both are
restatements of OpenCV written beside the kernels they judge, and OpenCV itself is absent: a mistake the
two share (a factor of 2 in size, a swapped axis, a flipped angle, a "corrected" upscale offset) passes
every bit-for-bit comparison.  These tests pin the oracle to what the algorithms must give on Gaussian
blobs of known centre, width, sign and background slope; the GPU inherits them through
test_gpu_detector_regimes.py, which compares it with the oracle on the same images (detector_cases.py).
The tolerances are the algorithms' own grids, none is fitted to the results.  CPU only.

These are the blob-level facts.  The orientation peaks, the 128 and 64 descriptor entries and SIFT's refined
position, layer, size and response as functions of the pixels are pinned by test_descriptor_anchors.py
(float64 models: sift_reference.py, surf_reference.py), on the device by test_gpu_descriptor_anchors.py.
Which keypoints exist (SIFT's extremum search with its contrast and edge tests, SURF's Hessian response,
maxima and interpolation) is pinned by test_detection_anchors.py, on the device by
test_gpu_detection_anchors.py.  Not pinned anywhere: parity with an OpenCV binary.

Measured on the committed oracle (printed by the tests):
  SIFT position error (after the +0.25 px offset) <= 0.05 px, size ratio 1.001 .. 1.024;
  SURF position error <= 0.12 px; orientation error <= 4.3 deg (SIFT), <= 9.1 deg (SURF, at theta 270)."""
import numpy as np
import pytest

import detector_cases as dc


def _nearest(k, cx, cy):
    d = np.hypot(k["x"] - cx, k["y"] - cy)
    i = int(np.argmin(d))
    return k[i], float(d[i])


@pytest.fixture(scope="module")
def anchor(oracle_mod):
    img = dc.anchor()
    return oracle_mod.sift_detect_and_compute(img)[0], oracle_mod.surf_detect_and_compute(img, 400.0)[0]


def test_sift_blob_position_size_response(anchor):
    """A blob of std s at (cx, cy): the keypoint nearest to it lies at (cx + 0.25, cy + 0.25) -- the quarter
    pixel of OpenCV's 2x upscale without enable_precise_upscale -- to within 0.125 px per axis (half the
    distance to the convention without the offset), its size is 2 sqrt((s^2 - 0.25) / 2^(1/3)) -- the DoG
    extremum of a Gaussian blob, SIFT's assumed 0.5 px camera blur taken off -- to within a factor 2^(1/6)
    (half a scale layer), and its response is positive."""
    ks, _ = anchor
    for cx, cy, s, _ in dc.ANCHOR_BLOBS:
        k, _ = _nearest(ks, cx + 0.25, cy + 0.25)
        want = 2.0 * np.sqrt((s * s - 0.25) / 2.0 ** (1.0 / 3.0))
        ex, ey, ratio = float(k["x"]) - (cx + 0.25), float(k["y"]) - (cy + 0.25), float(k["size"]) / want
        print(f"SIFT blob std {s}: dx {ex:+.4f} dy {ey:+.4f} size {float(k['size']):.4f} / {want:.4f} = {ratio:.4f}")
        assert abs(ex) <= 0.125 and abs(ey) <= 0.125
        assert 2.0 ** (-1.0 / 6.0) <= ratio <= 2.0 ** (1.0 / 6.0)
        assert k["response"] > 0


def test_surf_blob_position_sign_size_order(anchor):
    """SURF_create(400): the blobs of std 3, 5 and 8 are found within half a sampling step (0.5 * 2^octave
    px) of their centres, class_id (the sign of the Laplacian) is -1 on the bright blobs and +1 on the dark
    one, the sizes increase strictly with the std, and the blob of std 2 is not detected."""
    _, ku = anchor
    sizes = []
    for cx, cy, s, amp in dc.ANCHOR_BLOBS[:3]:
        k, dist = _nearest(ku, cx, cy)
        ex, ey = float(k["x"]) - cx, float(k["y"]) - cy
        print(f"SURF blob std {s}: dx {ex:+.4f} dy {ey:+.4f} octave {int(k['octave'])} size {float(k['size'])} "
              f"class_id {int(k['class_id'])}")
        half_step = 0.5 * 2 ** int(k["octave"])
        assert abs(ex) <= half_step and abs(ey) <= half_step
        assert k["class_id"] == (-1 if amp > 0 else 1)
        sizes.append(float(k["size"]))
    assert sizes[0] < sizes[1] < sizes[2]
    cx, cy, s, _ = dc.ANCHOR_BLOBS[3]
    _, dist = _nearest(ku, cx, cy)
    assert dist > 4 * s  # nothing at the std-2 blob: the nearest keypoint is another blob's


@pytest.mark.parametrize("theta", dc.RAMP_ANGLES)
def test_orientation_follows_the_ramp(oracle_mod, theta):
    """A blob on a ramp whose intensity increases along image angle theta (x right, y down): each detector
    returns exactly one keypoint, at the blob, and its angle is theta to within 10 degrees (one bin of
    SIFT's 36-bin histogram, two of SURF's 5-degree search increments)."""
    img = dc.ramp_blob(theta)
    cx, cy = dc.RAMP_BLOB[:2]
    for name, k in (("SIFT", oracle_mod.sift_detect_and_compute(img)[0]),
                    ("SURF", oracle_mod.surf_detect_and_compute(img, 400.0)[0])):
        assert len(k) == 1, name
        assert np.hypot(float(k["x"][0]) - cx, float(k["y"][0]) - cy) <= 1.0, name
        err = (float(k["angle"][0]) - theta + 180.0) % 360.0 - 180.0
        print(f"{name} theta {theta}: angle {float(k['angle'][0]):.3f} error {err:+.3f}")
        assert abs(err) <= 10.0, name
