"""entropy="device_split" on the GPU (jpeg_entropy_split_kernel): long entropy-coded segments
decoded by a workgroup each.  The reference is the one-lane decoder throughout,
ops.jpeg_entropy_host for coefficients and entropy="host" for bytes (pinned to Pillow by
tests/test_gpu_jpeg.py), and equality is exact.  The same inputs pass the host model of the
kernel's functions under the sanitizers in tests/test_jpeg_split_host.py (CPU suite)."""
import hashlib

import numpy as np
import pytest

from jpeg_cases import by_name, gray_np, load_cases

pytestmark = pytest.mark.gpu

ROSBOT_DIST = np.array([0.142541, -0.248887, -0.005254, -0.005417, 0.0])  # rosbot_calibration.yaml:22
ROSBOT_K = np.array([[606.811009, 0, 325.199941], [0, 611.104701, 227.591593], [0, 0, 1.0]])
SPLITS = [16, None]  # None: the decoder's default


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _set(decoder, split):
    from droplet_visual_odometry_amd import ops
    decoder.split_bytes = ops.JPEG_SPLIT_BYTES_DEFAULT if split is None else split
    return decoder.split_bytes


@pytest.fixture(scope="module")
def host():
    """ops.jpeg_entropy_host of every fixture it parses, computed once: name -> (coefficients, status)."""
    from droplet_visual_odometry_amd import ops
    out = {}
    for c in load_cases():
        if c.probe_status == 0:
            _, coef, st = ops.jpeg_entropy_host(c.blob)
            coef.setflags(write=False)
            out[c.name] = (coef, st)
    return out


@pytest.fixture(scope="module")
def decoder(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    d = ops.JpegDecoder(67, 50, group_frames=32, ctx=gpu_ctx)
    yield d
    d.close()


@pytest.fixture(scope="module")
def stream_decoder(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    d = ops.JpegDecoder(320, 240, group_frames=64, ctx=gpu_ctx)
    yield d
    d.close()


@pytest.mark.parametrize("split", SPLITS)
def test_every_small_fixture(decoder, host, split):
    """Files with restart markers ride along: at 16 bytes many of their segments are split too,
    the others take the one-lane kernel in the same group."""
    import torch
    _set(decoder, split)
    groups = {}
    for c in load_cases():
        if c.kind == "small":
            groups.setdefault(c.rgb.shape[:2], []).append(c)
    taken = 0
    for (h, w), cases in groups.items():
        assert len(cases) <= decoder.group_frames  # one group: coefficients() reaches every frame
        out = decoder.decode([c.blob for c in cases], color="gray", entropy="device_split")
        torch.cuda.synchronize()
        assert not decoder.status().any()  # no false DVO_ECORRUPT from the bits after the last block
        got = out.cpu().numpy()
        for i, c in enumerate(cases):
            np.testing.assert_array_equal(decoder.coefficients(i), host[c.name][0], err_msg=c.name)
            np.testing.assert_array_equal(got[i], gray_np(c.rgb[..., ::-1]), err_msg=c.name)
        _, segments, fallbacks = decoder.split_info()
        assert fallbacks == 0
        taken += segments
    assert taken >= (8 if split == 16 else 1)  # the split kernel did run: at least the long restart-free scans


@pytest.mark.parametrize("split", SPLITS)
def test_stream_frames_in_one_call(stream_decoder, host, split):
    """At 16 bytes per lane a scan is 1,722 to 1,938 runs: two chunks of a workgroup's lanes, with
    the state, the block ordinal and the DC sums carried over."""
    import torch
    d = stream_decoder
    s = _set(d, split)
    cases = [by_name(f"stream_{i}") for i in range(4)]
    gray = d.decode([c.blob for c in cases], color="gray", entropy="device_split").cpu().numpy()
    torch.cuda.synchronize()
    assert not d.status().any()
    passes, segments, fallbacks = d.split_info()
    assert (segments, fallbacks) == (4, 0) and 1 <= passes <= 31_003 // s + 1
    print(f"split_bytes {s}: at most {passes} synchronisation passes on the stream frames")
    for i, c in enumerate(cases):
        np.testing.assert_array_equal(d.coefficients(i), host[c.name][0], err_msg=c.name)
        assert _sha(gray[i]) == c.sha_gray
    bgr = d.decode([c.blob for c in cases], color="bgr", entropy="device_split").cpu().numpy()
    for i, c in enumerate(cases):
        assert _sha(bgr[i]) == c.sha_bgr


def test_many_workgroups_at_once(stream_decoder):
    import torch
    d = stream_decoder
    _set(d, None)
    c = by_name("stream_1")
    got = d.decode([c.blob] * 64, color="gray", entropy="device_split")
    torch.cuda.synchronize()
    assert not d.status().any()
    assert d.split_info()[1:] == (64, 0)
    assert (got == got[0]).all().item()
    assert _sha(got[0].cpu().numpy()) == _sha(got[63].cpu().numpy()) == c.sha_gray


@pytest.mark.parametrize("split", SPLITS)
def test_corrupt_frames_equal_host_entropy(decoder, split):
    """Statuses and all five pictures, the corrupt files' partial ones included."""
    import torch
    from droplet_visual_odometry_amd._native import DVO_ECORRUPT
    _set(decoder, split)
    good = [c for c in load_cases() if c.kind == "small" and c.rgb.shape[:2] == (50, 67)][:3]
    batch = [good[0].blob, by_name("neg_truncated").blob, good[1].blob, by_name("neg_random_scan").blob, good[2].blob]
    want = decoder.decode(batch, color="bgr", entropy="host").cpu().numpy()
    torch.cuda.synchronize()
    assert list(decoder.status()) == [0, DVO_ECORRUPT, 0, DVO_ECORRUPT, 0]
    got = decoder.decode(batch, color="bgr", entropy="device_split").cpu().numpy()
    torch.cuda.synchronize()
    assert list(decoder.status()) == [0, DVO_ECORRUPT, 0, DVO_ECORRUPT, 0]
    np.testing.assert_array_equal(got, want)
    _, segments, fallbacks = decoder.split_info()
    if split == 16:  # both corrupt scans were split, found corrupt and given to one lane
        assert segments >= 2 and fallbacks == 2
    for i, c in zip((0, 2, 4), good):
        np.testing.assert_array_equal(got[i], c.rgb[..., ::-1], err_msg=c.name)


@pytest.mark.parametrize("split", SPLITS)
def test_mixed_batch_in_short_groups(gpu_ctx, split):
    """All 67x50 files (gray, 4:4:4, 4:2:2, 4:2:0; no restart markers, one per MCU, per 3 MCUs,
    per row; the nine restart-free 4:2:0 ones) in groups of 3."""
    import torch
    from droplet_visual_odometry_amd import ops
    cases = [c for c in load_cases() if c.kind == "small" and c.name.startswith("67x50_")]
    assert len(cases) == 25 and sum("_420_" in c.name and c.name.endswith("_none") for c in cases) == 9
    d = ops.JpegDecoder(67, 50, group_frames=3, ctx=gpu_ctx, split_bytes=None if split is None else split)
    try:
        for color in ("gray", "bgr"):
            want = d.decode([c.blob for c in cases], color=color, entropy="host").cpu().numpy()
            got = d.decode([c.blob for c in cases], color=color, entropy="device_split").cpu().numpy()
            torch.cuda.synchronize()
            assert not d.status().any()
            np.testing.assert_array_equal(got, want)
    finally:
        d.close()


@pytest.mark.parametrize("undistorted", [False, True])
def test_stream_process_and_submit_jpeg_split(gpu_ctx, undistorted):
    """FrameStream.process_jpeg / submit_jpeg with entropy="device_split" against the default call."""
    import torch
    from droplet_visual_odometry_amd import cv, ops
    from droplet_visual_odometry_amd.stream import FrameStream
    blobs = [by_name(f"stream_{i}").blob for i in range(4)]
    K = ROSBOT_K * np.array([[0.5], [0.5], [1.0]])  # the rosbot camera at half size
    u = None
    if undistorted:
        newK, _ = cv.getOptimalNewCameraMatrix(K, ROSBOT_DIST, (320, 240), 1, (320, 240))
        u = ops.Undistorter(K, ROSBOT_DIST, newK, 320, 240, ctx=gpu_ctx)
    a = FrameStream(320, 240, K, nfeatures=500, max_frames=4, ctx=gpu_ctx)
    b = FrameStream(320, 240, K, nfeatures=500, max_frames=4, ctx=gpu_ctx)

    def same(ra, rb, n):
        a.sync()
        b.sync()
        np.testing.assert_array_equal(FrameStream.records_numpy(ra, n - 1), FrameStream.records_numpy(rb, n - 1))
        for i in range(n):
            (ka, da), (kb, db) = a.features(i), b.features(i)
            assert len(ka) > 0
            np.testing.assert_array_equal(ka, kb)
            np.testing.assert_array_equal(da, db)
    try:
        same(a.process_jpeg(blobs, undistort=u, entropy="device_split"), b.process_jpeg(blobs, undistort=u), 4)
        assert not a.jpeg_decoder.status().any()
        assert a.jpeg_decoder.split_info()[1] == 4 and b.jpeg_decoder.split_info()[1] == 0
        same(a.process_jpeg(blobs[:1], undistort=u), b.process_jpeg(blobs[:1], undistort=u), 1)
        assert a.jpeg_decoder.split_info()[1] == 1  # the mode stays until it is set again
        ra, rb = a.new_records(3), b.new_records(3)
        torch.cuda.synchronize()
        got = a.submit_jpeg(blobs, ra, undistort=u, entropy="device_split") + a.drain()
        want = b.submit_jpeg(blobs, rb, undistort=u, entropy="device") + b.drain()
        assert [p for _, p in got] == [p for _, p in want] == [3]
        a.sync()
        b.sync()
        np.testing.assert_array_equal(FrameStream.records_numpy(ra, 3), FrameStream.records_numpy(rb, 3))
        assert (FrameStream.records_numpy(ra, 3)["n_matches"] > 0).all()
        assert a.jpeg_decoder.split_info()[1] == 4
    finally:
        a.close()
        b.close()
        if u is not None:
            u.close()


def test_arguments(decoder):
    import ctypes
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    lib = decoder.ctx.lib
    _set(decoder, None)
    assert decoder.split_bytes == ops.JPEG_SPLIT_BYTES_DEFAULT
    for bad in (0, 8, 24, 8192):
        assert lib.dvo_jpeg_set_split(decoder.h_, bad) == DVO_EINVAL
        with pytest.raises(DVOError):
            decoder.split_bytes = bad
    assert decoder.split_bytes == ops.JPEG_SPLIT_BYTES_DEFAULT
    assert lib.dvo_jpeg_set_stream_entropy(decoder.h_, ops.JPEG_ENTROPY["host"]) == DVO_EINVAL
    assert lib.dvo_jpeg_set_stream_entropy(decoder.h_, 3) == DVO_EINVAL
    assert lib.dvo_jpeg_set_stream_entropy(decoder.h_, ops.JPEG_ENTROPY["device_split"]) == 0
    assert lib.dvo_jpeg_set_stream_entropy(decoder.h_, ops.JPEG_ENTROPY["device"]) == 0
    c = by_name("67x50_422_noise_q100_none")
    a = np.frombuffer(c.blob, np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_int64 * 1)(a.size)
    out = torch.full((1, 50, 67), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.dvo_jpeg_decode(decoder.h_, ptrs, lens, 1, 1, out.data_ptr(), out.stride(0), out.stride(1), 3, None)
    assert rc == DVO_EINVAL
    torch.cuda.synchronize()
    assert (out == 0xA5).all().item()
    with pytest.raises(ValueError):
        decoder.decode([c.blob], entropy="split")
    # "device" is what it was, whatever split_bytes says
    before = decoder.decode([c.blob], color="bgr", entropy="device").cpu().numpy()
    decoder.split_bytes = 16
    after = decoder.decode([c.blob], color="bgr", entropy="device").cpu().numpy()
    torch.cuda.synchronize()
    assert not decoder.status().any()
    np.testing.assert_array_equal(before[0], c.rgb[..., ::-1])
    np.testing.assert_array_equal(after, before)
    _set(decoder, None)
