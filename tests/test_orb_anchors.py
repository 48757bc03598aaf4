"""Anchors of the ORB oracle (oracle/orb.cpp) to float64 statements of the Harris response, the intensity-
centroid angle and the steered rBRIEF descriptor (orb_reference.py).  test_oracle_kats.py pins the pyramid
sizes, the blur constants, FAST, retainBest and the umax table, but nothing about `response`, `angle` or the
256 descriptor bits: a swapped Sobel term, atan2(m10, m01), a rotation of the wrong sign, a reversed bit
order or t0 > t1 would be the same in the oracle and on the device, and between frames, and pass every
bit-for-bit comparison.  test_gpu_orb_anchors.py applies the same checks to the device.  CPU only.

The tolerances (orb_reference.check_features states each): 0.3 degrees is OpenCV's documented fastAtan2
accuracy; the response bound is a counted float32 rounding bound (n = 18); descriptor bits are exact outside
a 1e-4 neighbourhood of rounding ties, whose share is capped at 0.5 %.

Measured on the committed oracle (printed by the tests): angle error 0.0094 degrees, response error
3.3 * 2^-24 of the terms, 43 of 69632 (320 x 240) and 59 of 53760 (161 x 97) bits excluded, no other bit
differs, and none of the excluded ones either."""
from conftest import synth_frames
import orb_reference as orbref


def _check(oracle_mod, img, nfeatures, label):
    kps, desc = oracle_mod.detect_and_compute(img, nfeatures)
    return orbref.check_features(kps, desc, oracle_mod.pyramid(img), oracle_mod.pyramid(img, blurred=True),
                                 oracle_mod.level_scales(), label)


def test_synthetic_frame_reaches_every_level(oracle_mod):
    """synth_frames(320, 240, [0]) at nfeatures 300: keypoints on all eight pyramid levels."""
    frames, _ = synth_frames(320, 240, [0])
    octaves = _check(oracle_mod, frames[0], 300, "oracle 320x240")
    assert octaves == set(range(8))


def test_small_odd_image(oracle_mod):
    """The 161 x 97 image (odd width and height, level widths that are no multiple of anything)."""
    _check(oracle_mod, orbref.small_image(), 500, "oracle 161x97")
