"""The JPEG decoder on the GPU against Pillow / libjpeg-turbo, byte for byte
(tests/golden/jpeg_cases.npz): every fixture as gray, BGR and BGRA with host and device entropy
decoding, pitched and padded destinations, a mixed batch in short groups, host against device
coefficients, corrupt and unsupported files, the stream entry points and the drop-in."""
import hashlib
import os
import sys
import types

import numpy as np
import pytest

from jpeg_cases import by_name, gray_np, load_cases, pillow_rgb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROSBOT_DIST = np.array([0.142541, -0.248887, -0.005254, -0.005417, 0.0])  # rosbot_calibration.yaml:22
ROSBOT_K = np.array([[606.811009, 0, 325.199941], [0, 611.104701, 227.591593], [0, 0, 1.0]])
COLORS = {"gray": 1, "bgr": 3, "bgra": 4}
ENTROPY = ["host", "device"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _expected(bgr, color):
    if color == "gray":
        return gray_np(bgr)
    if color == "bgr":
        return bgr
    return np.concatenate([bgr, np.full(bgr.shape[:2] + (1,), 255, np.uint8)], -1)


def _by_size():
    """The small fixtures grouped by size: one decoder call per size."""
    groups = {}
    for c in load_cases():
        if c.kind == "small":
            groups.setdefault(c.rgb.shape[:2], []).append(c)
    return groups


@pytest.fixture(scope="module")
def decoder(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    d = ops.JpegDecoder(67, 50, group_frames=8, ctx=gpu_ctx)
    yield d
    d.close()


@pytest.mark.parametrize("entropy", ENTROPY)
@pytest.mark.parametrize("color", list(COLORS))
def test_every_small_fixture(decoder, color, entropy):
    import torch
    for (h, w), cases in _by_size().items():
        out = decoder.decode([c.blob for c in cases], color=color, entropy=entropy)
        torch.cuda.synchronize()
        assert not decoder.status().any()
        got = out.cpu().numpy()
        assert got.shape[:3] == (len(cases), h, w)
        for i, c in enumerate(cases):
            np.testing.assert_array_equal(got[i], _expected(c.rgb[..., ::-1], color), err_msg=f"{c.name} {color} {entropy}")


@pytest.mark.parametrize("entropy", ENTROPY)
@pytest.mark.parametrize("name", ["large_320x240", "large_640x480"])
def test_large_fixtures(gpu_ctx, name, entropy):
    """More than 64 and more than 1,024 segments: several waves of the entropy kernel."""
    import torch
    from droplet_visual_odometry_amd import ops
    c = by_name(name)
    w, h, _, _ = ops.jpeg_probe(c.blob)
    d = ops.JpegDecoder(w, h, group_frames=2, ctx=gpu_ctx)
    try:
        live = pillow_rgb(c.blob)
        for color in COLORS:
            got = d.decode([c.blob, c.blob, c.blob], color=color, entropy=entropy).cpu().numpy()  # two groups
            torch.cuda.synchronize()
            assert not d.status().any()
            for i in range(3):
                if color == "gray":
                    assert _sha(got[i]) == c.sha_gray
                elif color == "bgr":
                    assert _sha(got[i]) == c.sha_bgr
                if live is not None:
                    np.testing.assert_array_equal(got[i], _expected(live[..., ::-1], color))
    finally:
        d.close()


def test_more_segments_than_waves(gpu_ctx):
    """28 x 600 segments in one group: more than the entropy kernel's 16,384 waves, so waves carry
    two segments, of the first and of the last frame (the plan then stays in global memory)."""
    import torch
    from droplet_visual_odometry_amd import ops
    c = by_name("large_640x480")
    d = ops.JpegDecoder(640, 480, group_frames=28, ctx=gpu_ctx)
    try:
        got = d.decode([c.blob] * 28, color="gray", entropy="device")
        torch.cuda.synchronize()
        assert not d.status().any()
        assert (got == got[0]).all().item()
        assert _sha(got[0].cpu().numpy()) == _sha(got[27].cpu().numpy()) == c.sha_gray
    finally:
        d.close()


def test_more_segments_than_lanes_of_a_launch(gpu_ctx):
    """256 gray 640x480 frames with a restart marker after every MCU are 1,228,800 segments in
    one group, more than the 64 x 16,384 lanes of the entropy launch: lanes take a second round."""
    pytest.importorskip("PIL")  # the file is made here
    import io
    import torch
    from PIL import Image
    from droplet_visual_odometry_amd import ops
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:480, 0:640]
    img = np.clip(128 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 10, (480, 640)), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=50, restart_marker_blocks=1)
    blob = buf.getvalue()
    lay, _, _ = ops.jpeg_entropy_host(blob)
    assert lay.segments == 4800 and 256 * lay.segments > 64 * 16384
    assert len(blob) <= 640 * 480 // 2  # so that 256 of them are one group of the decoder
    want = gray_np(pillow_rgb(blob)[..., ::-1])
    d = ops.JpegDecoder(640, 480, group_frames=256, ctx=gpu_ctx)
    try:
        got = d.decode([blob] * 256, color="gray", entropy="device")
        torch.cuda.synchronize()
        assert not d.status().any()
        assert d.coefficients(255).size == lay.coef_count  # frame 255 is in the last group: there was one group
        assert (got == got[0]).all().item()
        np.testing.assert_array_equal(got[0].cpu().numpy(), want)
        np.testing.assert_array_equal(got[255].cpu().numpy(), want)
    finally:
        d.close()


@pytest.mark.parametrize("entropy", ENTROPY)
@pytest.mark.parametrize("color", list(COLORS))
def test_destinations(decoder, color, entropy):
    """Pitches w c and w c + 3, a padded frame stride, 0xA5 guards: only the pixels are written."""
    import torch
    cases = [c for c in load_cases() if c.kind == "small" and c.rgb.shape[:2] == (31, 33)][:3]
    n, h, w, ch = len(cases), 31, 33, COLORS[color]
    for pitch in (w * ch, w * ch + 3):
        fstride = pitch * h + 37
        guard = 64
        raw = torch.full((guard + n * fstride + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        view = raw[guard:guard + n * fstride].as_strided((n, h, w, ch), (fstride, pitch, ch, 1))
        if ch == 1:
            view = view[..., 0]
        decoder.decode([c.blob for c in cases], color=color, entropy=entropy, out=view)
        torch.cuda.synchronize()
        got = raw.cpu().numpy()
        want = np.full_like(got, 0xA5)
        for i, c in enumerate(cases):
            e = _expected(c.rgb[..., ::-1], color).reshape(h, w * ch)
            for y in range(h):
                o = guard + i * fstride + y * pitch
                want[o:o + w * ch] = e[y]
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("entropy", ENTROPY)
def test_mixed_batch_in_short_groups(gpu_ctx, entropy):
    """gray / 4:4:4 / 4:2:2 / 4:2:0 and restart forms in one batch of 5 at group_frames = 2."""
    import torch
    from droplet_visual_odometry_amd import ops
    pick = ["33x31_gray_", "33x31_444_", "33x31_422_", "33x31_420_"]
    small = [c for c in load_cases() if c.kind == "small"]
    cases = [next(c for c in small if c.name.startswith(p) and f"_{r}" in c.name)
             for p, r in zip(pick, ["mcu1", "row1", "mcu3", "none"])]
    cases.append(next(c for c in small if c.name.startswith("33x31_420_") and "_mcu1" in c.name))
    d = ops.JpegDecoder(40, 40, group_frames=2, ctx=gpu_ctx)
    try:
        for color in COLORS:
            got = d.decode([c.blob for c in cases], color=color, entropy=entropy).cpu().numpy()
            torch.cuda.synchronize()
            assert not d.status().any()
            for i, c in enumerate(cases):
                np.testing.assert_array_equal(got[i], _expected(c.rgb[..., ::-1], color), err_msg=c.name)
    finally:
        d.close()


def test_host_and_device_coefficients_agree(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd import ops
    d = ops.JpegDecoder(640, 480, group_frames=1, ctx=gpu_ctx)
    try:
        for c in load_cases():
            if c.kind == "negative":
                continue
            _, want, st = ops.jpeg_entropy_host(c.blob)
            assert st == 0
            coefs = []
            for entropy in ENTROPY:
                d.decode([c.blob], color="gray", entropy=entropy)
                coefs.append(d.coefficients(0))
            np.testing.assert_array_equal(coefs[0], want, err_msg=c.name)
            np.testing.assert_array_equal(coefs[1], want, err_msg=c.name)
    finally:
        d.close()


@pytest.mark.parametrize("entropy", ENTROPY)
def test_corrupt_frames_have_a_status_and_spare_the_others(decoder, entropy):
    """The same bytes pass tests/test_jpeg_entropy_host.py under the sanitizers, in the CPU
    suite, which runs before this one (README.md, `tests/`)."""
    import torch
    from droplet_visual_odometry_amd._native import DVO_ECORRUPT
    good = [c for c in load_cases() if c.kind == "small" and c.rgb.shape[:2] == (50, 67)][:3]
    batch = [good[0].blob, by_name("neg_truncated").blob, good[1].blob, by_name("neg_random_scan").blob, good[2].blob]
    got = decoder.decode(batch, color="bgr", entropy=entropy).cpu().numpy()
    torch.cuda.synchronize()
    assert list(decoder.status()) == [0, DVO_ECORRUPT, 0, DVO_ECORRUPT, 0]
    for i, c in zip((0, 2, 4), good):
        np.testing.assert_array_equal(got[i], c.rgb[..., ::-1], err_msg=c.name)


@pytest.mark.parametrize("name,code", [("neg_progressive", -7), ("neg_440", -7), ("neg_dht_cut", -8)])
def test_unsupported_files_raise_before_any_launch(decoder, name, code):
    import torch
    from droplet_visual_odometry_amd._native import DVOError
    good = next(c for c in load_cases() if c.kind == "small" and c.rgb.shape[:2] == (50, 67))
    out = torch.full((2, 50, 67, 3), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(DVOError, match="frame 1") as e:
        decoder.decode([good.blob, by_name(name).blob], color="bgr", out=out)
    assert e.value.code == code
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()  # nothing ran, not even for the good frame


def test_decode_image_and_bad_arguments(decoder):
    from droplet_visual_odometry_amd._native import DVOError
    c = next(c for c in load_cases() if c.kind == "small" and c.name.startswith("67x50_422_"))
    np.testing.assert_array_equal(decoder.decode_image(c.blob, "bgr"), c.rgb[..., ::-1])
    np.testing.assert_array_equal(decoder.decode_image(c.blob, "gray"), gray_np(c.rgb[..., ::-1]))
    with pytest.raises(DVOError) as e:
        decoder.decode_image(by_name("neg_truncated").blob)
    assert e.value.code == -8
    with pytest.raises(DVOError) as e:  # larger than the decoder's maximum
        decoder.decode([by_name("stream_0").blob])
    assert e.value.code == -1
    with pytest.raises(DVOError) as e:  # sizes differ within a batch
        decoder.decode([c.blob, next(x for x in load_cases() if x.name.startswith("33x31_")).blob])
    assert e.value.code == -1


# ---- stream -------------------------------------------------------------------------------------
def _stream_frames():
    """4 colour JPEG frames at 320x240 and Pillow's BGR of each: synth_frames encoded here where
    Pillow is installed, the stored files (and the decoder's own BGR, once its hash is the
    stored one) elsewhere."""
    from conftest import synth_frames
    frames, K = synth_frames(320, 240, range(4))
    try:
        import io
        from PIL import Image
        rgb = np.ascontiguousarray(np.stack([frames, np.roll(frames, 3, axis=2), 255 - frames], -1))
        blobs = []
        for f in rgb:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, "JPEG", quality=90, subsampling=2)
            blobs.append(buf.getvalue())
        bgr = np.stack([pillow_rgb(b)[..., ::-1] for b in blobs])
    except ImportError:
        from droplet_visual_odometry_amd import ops
        cases = [by_name(f"stream_{i}") for i in range(4)]
        blobs = [c.blob for c in cases]
        d = ops.JpegDecoder(320, 240, group_frames=4)
        bgr = np.stack([d.decode_image(b, "bgr") for b in blobs])
        d.close()
        for c, f in zip(cases, bgr):
            assert _sha(f) == c.sha_bgr
    return blobs, np.ascontiguousarray(bgr), K


def _assert_same_batch(a, ra, b, rb, n):
    from droplet_visual_odometry_amd.stream import FrameStream
    a.sync()
    b.sync()
    np.testing.assert_array_equal(FrameStream.records_numpy(ra, n - 1), FrameStream.records_numpy(rb, n - 1))
    for i in range(n):
        (ka, da), (kb, db) = a.features(i), b.features(i)
        assert len(ka) > 0
        np.testing.assert_array_equal(ka, kb)
        np.testing.assert_array_equal(da, db)


@pytest.mark.parametrize("undistorted", [False, True])
def test_stream_process_and_submit_jpeg(gpu_ctx, undistorted):
    import torch
    from droplet_visual_odometry_amd import cv, ops
    from droplet_visual_odometry_amd.stream import FrameStream
    blobs, bgr, _ = _stream_frames()
    K = ROSBOT_K * np.array([[0.5], [0.5], [1.0]])  # the rosbot camera at half size
    u = None
    if undistorted:
        newK, _ = cv.getOptimalNewCameraMatrix(K, ROSBOT_DIST, (320, 240), 1, (320, 240))
        u = ops.Undistorter(K, ROSBOT_DIST, newK, 320, 240, ctx=gpu_ctx)
    dbgr = torch.from_numpy(bgr).cuda()
    a = FrameStream(320, 240, K, nfeatures=500, max_frames=4, ctx=gpu_ctx)
    b = FrameStream(320, 240, K, nfeatures=500, max_frames=4, ctx=gpu_ctx)
    try:
        _assert_same_batch(a, a.process_jpeg(blobs, undistort=u), b, b.process(dbgr, undistort=u), 4)
        assert not a.jpeg_decoder.status().any()
        _assert_same_batch(a, a.process_jpeg(blobs[:1], undistort=u), b, b.process(dbgr[:1], undistort=u), 1)
        ra, rb = a.new_records(3), b.new_records(3)
        torch.cuda.synchronize()
        got = a.submit_jpeg(blobs, ra, undistort=u) + a.drain()
        want = b.submit(dbgr, rb, undistort=u) + b.drain()
        assert [p for _, p in got] == [p for _, p in want] == [3]
        a.sync()
        b.sync()
        np.testing.assert_array_equal(FrameStream.records_numpy(ra, 3), FrameStream.records_numpy(rb, 3))
        assert (FrameStream.records_numpy(ra, 3)["n_matches"] > 0).all()
    finally:
        a.close()
        b.close()
        if u is not None:
            u.close()


# ---- drop-in ------------------------------------------------------------------------------------
def _yaml(K, dist):
    d = ", ".join(repr(float(v)) for v in K.ravel())
    k = ", ".join(repr(float(v)) for v in dist)
    return (f"camera_matrix:\n  rows: 3\n  cols: 3\n  data: [{d}]\n"
            f"distortion_coefficients:\n  rows: 1\n  cols: 5\n  data: [{k}]\n")


@pytest.mark.parametrize("name,size,fused", [("large_640x480", (640, 480), True), ("neg_progressive", (67, 50), False)])
def test_dropin_compressed_message(gpu_ctx, tmp_path, monkeypatch, name, size, fused):
    """A "compressed" message gives the same image through the fused call as through imdecode ->
    _undistort_bgr2gray; the progressive file takes the second route by itself."""
    pytest.importorskip("PIL")  # the host route is cv.imdecode
    from droplet_visual_odometry_amd import cv
    sys.path.insert(0, os.path.join(ROOT, "droplet_visual_odometry_amd", "dropin"))
    try:
        import visual_odometry_v3 as v3
    finally:
        sys.path.pop(0)
    y = tmp_path / "cal.yaml"
    y.write_text(_yaml(ROSBOT_K, ROSBOT_DIST))
    vo = v3.VisualOdometry(mode="orb", calibration_file_path=str(y), controlled=True, real_marker_length=0.1)
    vo.frame_width, vo.frame_height = size
    msg = types.SimpleNamespace(data=by_name(name).blob)
    calls = []
    real = cv._undistort_jpeg2gray

    def spy(*a, **k):
        calls.append(real(*a, **k))
        return calls[-1]
    monkeypatch.setattr(cv, "_undistort_jpeg2gray", spy)
    got = vo.ros_img_msg_to_opencv_image(msg, "compressed")
    assert len(calls) == 1 and (calls[0] is not None) == fused
    monkeypatch.setattr(cv, "_undistort_jpeg2gray", lambda *a, **k: None)  # the fused branch disabled
    want = vo.ros_img_msg_to_opencv_image(msg, "compressed")
    assert got.dtype == np.uint8 and got.shape == size[::-1]
    np.testing.assert_array_equal(got, want)
    assert (want != gray_np(pillow_rgb(msg.data)[..., ::-1])).any()  # the calibration does distort
