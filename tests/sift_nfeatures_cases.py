"""The inputs of the SIFT nfeatures tests (test_sift_nfeatures_host.py, test_gpu_sift_nfeatures.py,
test_gpu_knn_nfeatures.py) and their expected values: SIFT_create(nfeatures = N).detectAndCompute is
the oracle's default detection with OpenCV 4.x's retainBest applied to the keypoint list,

    k, d = oracle.sift_detect_and_compute(img);  p = oracle.retain_best(k["response"], N);  k[p], d[p]

(a descriptor depends on its own keypoint only, and the firstOctave rescale leaves response alone).
The figures below were taken from the CPU oracle; the host test checks them, so that no GPU case
can pass on a list that is not cut, has no tie at the boundary or is not permuted."""
import numpy as np

import detector_cases as dc
from conftest import synth_frames

# name -> image.  The 176 x 160 detector cases (the smallest frames whose lists take several
# partition steps) and one 320 x 240 block-noise frame with more than 1024 keypoints.
IMAGES = {
    "noise": lambda: dc.noise(176, 160),
    "tiled": lambda: dc.tiled(),
    "block_noise": lambda: dc.block_noise(176, 160, 2),
    "block_noise_320": lambda: dc.block_noise(320, 240, 3),
    "tiled_shifted": lambda: dc.tiled(dc.TILE),
    "anchor": lambda: dc.anchor(),
}
FULL = {"noise": 107, "tiled": 42, "block_noise": 469, "block_noise_320": 1297}
# (image, N, kept count): cuts with and without ties at the boundary response.  block_noise's two
# weakest keypoints tie, so N = 468 keeps all 469 (permuted); noise's do not: N = 106 keeps 106.
CUTS = (("noise", 1, 1), ("noise", 2, 3), ("noise", 64, 65), ("noise", 106, 106),
        ("tiled", 1, 9), ("tiled", 16, 33),
        ("block_noise", 234, 234), ("block_noise", 468, 469),
        ("block_noise_320", 1024, 1024))

# the group test: five 176 x 160 frames at N = 16
GROUP_FRAMES = ("noise", "tiled", "block_noise", "tiled_shifted", "anchor")
GROUP_N = 16
GROUP_KEPT = (17, 33, 16, 30, 20)

# the k-NN tests: the 320 x 240 synthetic frames 0..3
SYNTH_WH = (320, 240)
SYNTH_FULL = (750, 783, 945, 1131)
SYNTH_KEPT = {300: (300, 300, 302, 300), 64: (64, 64, 64, 65)}

_IMG, _FULL, _EXP = {}, {}, {}


def image(name):
    """A named image, or ("synth", i): synthetic 320 x 240 frame i."""
    if name not in _IMG:
        _IMG[name] = synth_frames(*SYNTH_WH, [name[1]])[0][0] if isinstance(name, tuple) else IMAGES[name]()
    return _IMG[name]


def synth():
    """(frames uint8 [4, 240, 320], K) of the k-NN tests."""
    return synth_frames(*SYNTH_WH, range(4))


def full(oracle_mod, name):
    """The oracle's default detection of the image, computed once."""
    if name not in _FULL:
        _FULL[name] = oracle_mod.sift_detect_and_compute(image(name))
    return _FULL[name]


def perm(oracle_mod, name, n):
    k, _ = full(oracle_mod, name)
    return np.arange(len(k)) if n == 0 else oracle_mod.retain_best(k["response"], n)


def expected(oracle_mod, name, n):
    """(keypoints, descriptors) of SIFT_create(nfeatures = n) on the image, computed once."""
    if (name, n) not in _EXP:
        k, d = full(oracle_mod, name)
        p = perm(oracle_mod, name, n)
        _EXP[(name, n)] = (k[p].copy(), d[p].copy())
    return _EXP[(name, n)]


def same_features(got, want):
    """Bytes, not tolerances."""
    (kg, dg), (kw, dw) = got, want
    assert len(kg) == len(kw) and len(dg) == len(dw), (len(kg), len(kw))
    np.testing.assert_array_equal(kg.view(np.uint8), kw.view(np.uint8))
    np.testing.assert_array_equal(np.ascontiguousarray(dg).view(np.uint32), np.ascontiguousarray(dw).view(np.uint32))
