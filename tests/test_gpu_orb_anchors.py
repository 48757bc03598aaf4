"""The float64 anchors of orb_reference.py (Harris response, intensity-centroid angle, steered rBRIEF bits)
applied to what the device returns, directly and not by way of the oracle: the per-call entry point
(ops.detect_and_compute) on both images and the batched stream (FrameStream.features) on the 320 x 240
frame.  The level images the reference reads are the oracle's pyramid, which test_oracle_kats.py pins and
test_gpu_pyramid.py compares with the device.  Tolerances: orb_reference.check_features."""
import pytest

from conftest import synth_frames
import orb_reference as orbref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def images(oracle_mod):
    """(image, nfeatures, levels, blurred levels) of the two inputs, computed once."""
    frames, K = synth_frames(320, 240, [0])
    out = {}
    for name, img, nf in (("320x240", frames[0], 300), ("161x97", orbref.small_image(), 500)):
        out[name] = (img, nf, oracle_mod.pyramid(img), oracle_mod.pyramid(img, blurred=True))
    return out, K, oracle_mod.level_scales()


@pytest.mark.parametrize("name", ["320x240", "161x97"])
def test_detect_and_compute_against_float64(gpu_ctx, images, name):
    from droplet_visual_odometry_amd import ops
    table, _, scales = images
    img, nf, levels, blurred = table[name]
    kps, desc = ops.detect_and_compute(img, nf, ctx=gpu_ctx)
    octaves = orbref.check_features(kps, desc, levels, blurred, scales, f"device detect_and_compute {name}")
    if name == "320x240":
        assert octaves == set(range(8))


def test_stream_features_against_float64(gpu_ctx, images):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    table, K, scales = images
    img, nf, levels, blurred = table["320x240"]
    fs = FrameStream(320, 240, K, nfeatures=nf, max_frames=2, ctx=gpu_ctx)
    try:
        fs.process(torch.from_numpy(img[None]).cuda())
        fs.sync()
        kps, desc = fs.features(0)
    finally:
        fs.close()
    assert orbref.check_features(kps, desc, levels, blurred, scales, "device FrameStream 320x240") == set(range(8))
