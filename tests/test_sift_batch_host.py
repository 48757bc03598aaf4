"""dvo_sift_batch_bytes: the group SIFT detector's scratch (include/dvo.h, the formula at
dvo_sift_batch_create), recomputed here; and the argument checks that need no device."""
import math

import pytest


def _lib():
    from droplet_visual_odometry_amd import _native
    return _native.load_library()


def _formula(w, h, group):
    """include/dvo.h: S = the octaves' pixels, octave 0 = 2w x 2h, halved with truncation."""
    ow, oh = 2 * w, 2 * h
    noct = max(1, min(round(math.log2(min(ow, oh)) - 2) + 1, 16))
    S = 0
    for _ in range(noct):
        if ow < 1 or oh < 1:
            break
        S += ow * oh
        ow, oh = ow // 2, oh // 2
    frame = 4 * (6 * S + 5 * S + 2 * w * 2 * h) + 16 * 262144 + 28 * 65536 + 4 * 65536 + 16
    return group * frame + 400


@pytest.mark.parametrize("wh", [(640, 480), (161, 97), (8, 8)])
def test_bytes_equal_the_documented_formula(wh):
    w, h = wh
    lib = _lib()
    b1, b16 = lib.dvo_sift_batch_bytes(w, h, 1), lib.dvo_sift_batch_bytes(w, h, 16)
    assert b1 == _formula(w, h, 1) and b16 == _formula(w, h, 16)
    # linear in the group: every further frame costs what the first does, the taps table is shared
    assert b16 - b1 == 15 * (b1 - 400)
    assert lib.dvo_sift_batch_bytes(w, h, 2) - b1 == b1 - 400


def test_documented_sizes():
    lib = _lib()
    assert round(lib.dvo_sift_batch_bytes(640, 480, 1) / 1e6, 1) == 83.3
    assert round(lib.dvo_sift_batch_bytes(1280, 720, 1) / 1e6, 1) == 237.3
    # a group's pyramid passes 2^31 bytes at small groups: the frame bases are 64-bit
    assert lib.dvo_sift_batch_bytes(1280, 720, 16) > 2 ** 31


def test_python_wrapper():
    from droplet_visual_odometry_amd import ops
    assert ops.SiftBatch.scratch_bytes(161, 97, 4) == _formula(161, 97, 4)
    with pytest.raises(ValueError):
        ops.SiftBatch.scratch_bytes(161, 97, 0)


@pytest.mark.parametrize("args", [(0, 8, 1), (8, 0, 1), (4096, 8, 1), (8, 4096, 1), (8, 8, 0), (8, 8, 65), (8, 8, -1)])
def test_bytes_rejects_what_create_rejects(args):
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    assert _lib().dvo_sift_batch_bytes(*args) == DVO_EINVAL


def test_null_handles_are_einval():
    import ctypes
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    lib = _lib()
    h = ctypes.c_void_p()
    assert lib.dvo_sift_batch_create(None, 8, 8, 1, ctypes.byref(h)) == DVO_EINVAL and not h.value
    assert lib.dvo_sift_batch_detect(None, None, 1, 64, 8, 16, None, None, None) == DVO_EINVAL
    assert lib.dvo_knn_stream_set_detect_group(None, 4) == DVO_EINVAL
    assert not lib.dvo_sift_batch_hip_stream(None)
    lib.dvo_sift_batch_destroy(None)  # a no-op
