"""Colour-frame input without a GPU: the six entry points are declared in
include/dvo.h and bound in _native._SIGNATURES, and the Python layer refuses
malformed colour frames with ValueError before it makes any library call (the
objects under test are built without their constructors, so they hold no context:
a library call would fail with AttributeError, not ValueError)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["dvo_bgr2gray", "dvo_bgr2gray_image", "dvo_undistort_apply_bgr", "dvo_undistort_image_bgr",
           "dvo_stream_process_bgr", "dvo_stream_submit_bgr"]


def test_colour_symbols_declared_and_bound():
    from droplet_visual_odometry_amd import _native
    src = open(os.path.join(ROOT, "include", "dvo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(dvo_\w+)\s*\(", src, flags=re.M))
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGNATURES, name
    # the stream calls take the channel count between the row stride and the records
    args, res = _native._SIGNATURES["dvo_stream_process_bgr"]
    assert len(args) == 8 and _native._SIGNATURES["dvo_stream_submit_bgr"] == (args, res)
    assert len(_native._SIGNATURES["dvo_bgr2gray"][0]) == 12
    assert len(_native._SIGNATURES["dvo_undistort_apply_bgr"][0]) == 10


def _bare_stream(w=16, h=8):
    from droplet_visual_odometry_amd.stream import FrameStream
    fs = FrameStream.__new__(FrameStream)  # no context, no library handle
    fs.width, fs.height, fs.max_frames, fs.nfeatures = w, h, 4, 500
    fs.h = None
    return fs


def _bad_colour_batches(w=16, h=8):
    good = torch.zeros((2, h, w, 3), dtype=torch.uint8)
    return {
        "float dtype": torch.zeros((2, h, w, 3), dtype=torch.float32),
        "int32 dtype": torch.zeros((2, h, w, 3), dtype=torch.int32),
        "two channels": torch.zeros((2, h, w, 2), dtype=torch.uint8),
        "five channels": torch.zeros((2, h, w, 5), dtype=torch.uint8),
        "one channel": torch.zeros((2, h, w, 1), dtype=torch.uint8),
        "planar (channel stride != 1)": torch.zeros((2, 3, h, w), dtype=torch.uint8).permute(0, 2, 3, 1),
        "pixel stride != C": torch.zeros((2, h, w, 4), dtype=torch.uint8)[..., :3],
        "columns strided": torch.zeros((2, h, 2 * w, 3), dtype=torch.uint8)[:, :, ::2],
        "host tensor": good,
    }


@pytest.mark.parametrize("name", list(_bad_colour_batches()))
def test_frame_stream_refuses_bad_colour_frames(name):
    fs = _bare_stream()
    frames = _bad_colour_batches()[name]
    assert frames.dim() == 4
    rec = torch.zeros(4 * 256, dtype=torch.uint8)
    with pytest.raises(ValueError):
        fs.process(frames)
    with pytest.raises(ValueError):
        fs.submit(frames, rec)


def test_frame_stream_refuses_other_sizes_and_mono_submit_undistort():
    fs = _bare_stream(16, 8)
    rec = torch.zeros(4 * 256, dtype=torch.uint8)
    wrong = torch.zeros((2, 8, 20, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="frame size"):
        fs.process(wrong)
    with pytest.raises(ValueError, match="frame size"):
        fs.submit(wrong, rec)
    with pytest.raises(ValueError, match="colour"):
        fs.submit(torch.zeros((2, 8, 16), dtype=torch.uint8), rec, undistort=object())
    # the mono8 checks are the old ones
    with pytest.raises(ValueError, match=r"\[n, H, W\]"):
        fs.process(torch.zeros((2, 8, 16), dtype=torch.float32))


def test_ops_refuse_bad_colour_input():
    from droplet_visual_odometry_amd import ops
    for bad in (np.zeros((8, 16), np.uint8), np.zeros((8, 16, 2), np.uint8), np.zeros((8, 16, 5), np.uint8),
                np.zeros((8, 16, 3), np.float32), np.zeros((0, 16, 3), np.uint8), np.zeros((2, 8, 16, 3), np.uint8)):
        with pytest.raises(ValueError):
            ops.bgr2gray(bad)
    dst = torch.zeros((2, 8, 16), dtype=torch.uint8)
    for name, frames in _bad_colour_batches().items():
        with pytest.raises(ValueError):
            ops.bgr2gray_device(frames, dst)
    with pytest.raises(ValueError):
        ops.bgr2gray_device(np.zeros((2, 8, 16, 3), np.uint8), dst)


def test_undistorter_refuses_bad_colour_input():
    from droplet_visual_odometry_amd import ops
    u = ops.Undistorter.__new__(ops.Undistorter)  # no context, no remap table
    u.w, u.h, u.h_ = 16, 8, None
    for bad in (np.zeros((8, 16, 2), np.uint8), np.zeros((8, 16, 5), np.uint8), np.zeros((8, 16, 3), np.int16),
                np.zeros((8, 20, 3), np.uint8), np.zeros((9, 16, 4), np.uint8)):
        with pytest.raises(ValueError):
            u.image(bad)
    dst = torch.zeros((2, 8, 16), dtype=torch.uint8)
    for name, frames in _bad_colour_batches().items():
        with pytest.raises(ValueError):
            u.apply(frames, dst)
    with pytest.raises(ValueError, match="undistorter size"):
        u.apply(torch.zeros((2, 8, 20, 3), dtype=torch.uint8), dst)
