"""The JPEG decoder without a GPU: the host parser and Huffman decoder
(dvo_jpeg_probe, dvo_jpeg_entropy_host) against Pillow / libjpeg-turbo on the fixtures of
tests/golden/jpeg_cases.npz.  The coefficients the library decodes are pushed through a numpy
restatement, kept in this file, of libjpeg-turbo's default arithmetic (jidctint.c, jdsample.c,
jdcolor.c) and must give Pillow's RGB byte for byte; the entry points are declared and bound;
FrameStream refuses malformed JPEG batches with ValueError before any library call."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from jpeg_cases import by_name, gray_np, load_cases, pillow_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["dvo_jpeg_probe", "dvo_jpeg_entropy_host", "dvo_jpeg_create", "dvo_jpeg_destroy", "dvo_jpeg_decode",
           "dvo_jpeg_status", "dvo_jpeg_decode_image", "dvo_undistort_image_jpeg", "dvo_stream_process_jpeg",
           "dvo_stream_submit_jpeg", "dvo_jpeg_get_coefficients"]

DECODABLE = [c for c in load_cases() if c.kind != "negative"]


# ---- libjpeg-turbo's default decode from coefficients, in numpy ---------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(v, axis, n):
    """One 1-D pass of jpeg_idct_islow over the 8 entries of `axis`, descaled by n."""
    v = np.moveaxis(v, axis, 0).astype(np.int64)
    v0, v1, v2, v3, v4, v5, v6, v7 = v
    z1 = (v2 + v6) * 4433
    t2 = z1 - v6 * 15137
    t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = v7, v5, v3, v1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d])
    return np.moveaxis(_descale(out, n), 0, axis)


def _plane(lay, coef, c):
    bw, bh = lay.blocks_w[c], lay.blocks_h[c]
    q = np.array(lay.quant[c][:], np.int64).reshape(8, 8)
    blk = coef[lay.coef_offset[c]:lay.coef_offset[c] + bw * bh * 64].astype(np.int64).reshape(bh, bw, 8, 8) * q
    blk = _idct_pass(blk, 2, 11)  # columns: along the rows of each block
    blk = _idct_pass(blk, 3, 18)  # rows
    return np.clip(blk + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _shift(p, d, axis):
    """p moved by d along axis with its edge replicated."""
    idx = np.clip(np.arange(p.shape[axis]) - d, 0, p.shape[axis] - 1)
    return np.take(p, idx, axis=axis)


def _up_h2v1(p):
    if p.shape[1] <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + _shift(p, 1, 1) + 1) >> 2
    out[:, 1::2] = (3 * p + _shift(p, -1, 1) + 2) >> 2
    return out


def _up_h2v2(p):
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    cs = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    cs[0::2] = 3 * p + _shift(p, 1, 0)
    cs[1::2] = 3 * p + _shift(p, -1, 0)
    out = np.empty((cs.shape[0], 2 * cs.shape[1]), np.int64)
    out[:, 0::2] = (3 * cs + _shift(cs, 1, 1) + 8) >> 4
    out[:, 1::2] = (3 * cs + _shift(cs, -1, 1) + 7) >> 4
    return out


def rgb_from_coefficients(lay, coef):
    W, H = lay.width, lay.height
    Y = _plane(lay, coef, 0)[:H, :W]
    if lay.components == 1:
        return np.repeat(Y[..., None], 3, axis=2).astype(np.uint8)
    hs, vs = lay.sampling >> 4, lay.sampling & 15
    cw, ch = -(-W // hs), -(-H // vs)
    chroma = []
    for c in (1, 2):
        p = _plane(lay, coef, c)[:ch, :cw]
        if (hs, vs) == (2, 1):
            p = _up_h2v1(p)
        elif (hs, vs) == (2, 2):
            p = _up_h2v2(p)
        chroma.append(p[:H, :W] - 128)
    cb, cr = chroma
    R = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
    G = np.clip(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    B = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
    return np.stack([R, G, B], -1).astype(np.uint8)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the entry points ----------------------------------------------------------------------------
def test_jpeg_symbols_declared_and_bound():
    from droplet_visual_odometry_amd import _native
    src = open(os.path.join(ROOT, "include", "dvo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^\s*(?:int|void)\s+(dvo_\w+)\s*\(", src, flags=re.M))
    lib = _native.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _native._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert _native._SIGNATURES["dvo_stream_process_jpeg"] == _native._SIGNATURES["dvo_stream_submit_jpeg"]
    assert len(_native._SIGNATURES["dvo_jpeg_decode"][0]) == 10
    assert (_native.DVO_EUNSUPPORTED, _native.DVO_ECORRUPT) == (-7, -8)
    assert "#define DVO_EUNSUPPORTED (-7)" in src and "#define DVO_ECORRUPT (-8)" in src


def test_fixture_covers_the_issue():
    cases = load_cases()
    small = [c for c in cases if c.kind == "small"]
    assert 180 <= len(small) <= 230
    sizes = ["1x1", "3x2", "4x5", "5x7", "6x3", "9x2", "8x8", "16x16", "17x9", "33x31", "67x50"]
    for s in sizes:
        for f in ("gray", "444", "422", "420"):
            forms = {c.name.split("_")[4] for c in small if c.name.startswith(f"{s}_{f}_")}
            assert forms == {"none", "mcu1", "mcu3", "row1"}, (s, f, forms)
    assert any(c.name.endswith("_opt") for c in small)
    assert {c.name for c in cases if c.kind == "negative"} == {"neg_progressive", "neg_440", "neg_truncated",
                                                               "neg_random_scan", "neg_dht_cut"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")) < 1 << 20


@pytest.mark.parametrize("case", DECODABLE, ids=lambda c: c.name)
def test_host_entropy_through_numpy_equals_pillow(case):
    """The test that fails without the feature: the library's coefficients, through the
    numpy restatement above, are Pillow's decode byte for byte."""
    from droplet_visual_odometry_amd import ops
    lay, coef, st = ops.jpeg_entropy_host(case.blob)
    assert st == 0
    rgb = rgb_from_coefficients(lay, coef)
    if case.rgb is not None:
        assert rgb.shape == case.rgb.shape
        np.testing.assert_array_equal(rgb, case.rgb)
    else:
        assert _sha(rgb[..., ::-1]) == case.sha_bgr
        assert _sha(gray_np(rgb[..., ::-1])) == case.sha_gray


def test_pillow_live_equals_stored():
    pytest.importorskip("PIL")
    for case in DECODABLE:
        rgb = pillow_rgb(case.blob)
        if case.rgb is not None:
            np.testing.assert_array_equal(rgb, case.rgb, err_msg=case.name)
        else:
            assert _sha(rgb[..., ::-1]) == case.sha_bgr, case.name


def test_probe_statuses_and_sizes():
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    for case in load_cases():
        if case.probe_status:
            with pytest.raises(DVOError) as e:
                ops.jpeg_probe(case.blob)
            assert e.value.code == case.probe_status, case.name
            with pytest.raises(DVOError) as e:
                ops.jpeg_entropy_host(case.blob)
            assert e.value.code == case.probe_status, case.name
            continue
        w, h, nc, sampling = ops.jpeg_probe(case.blob)
        if case.kind == "small":
            size, fmt = case.name.split("_")[:2]
            assert f"{w}x{h}" == size, case.name
            assert (h, w) == case.rgb.shape[:2]
            assert (nc, sampling) == {"gray": (1, 0x11), "444": (3, 0x11), "422": (3, 0x21), "420": (3, 0x22)}[fmt]
        elif case.kind == "large":
            assert f"large_{w}x{h}" == case.name and (nc, sampling) == (3, 0x22)
        elif case.kind == "stream":
            assert (w, h, nc, sampling) == (320, 240, 3, 0x22)


def test_segments_follow_the_restart_interval():
    from droplet_visual_odometry_amd import ops
    lay, _, _ = ops.jpeg_entropy_host(by_name("large_320x240").blob)
    assert lay.restart_interval == 2 and lay.segments == 150 > 64  # 20 x 15 MCUs
    lay, _, _ = ops.jpeg_entropy_host(by_name("large_640x480").blob)
    assert lay.restart_interval == 2 and lay.segments == 600
    lay, _, _ = ops.jpeg_entropy_host(by_name("stream_0").blob)
    assert lay.restart_interval == 0 and lay.segments == 1


def test_corrupt_scans_are_reported_and_stay_in_bounds():
    from droplet_visual_odometry_amd import ops
    for name in ("neg_truncated", "neg_random_scan"):
        lay, coef, st = ops.jpeg_entropy_host(by_name(name).blob)
        assert st == -8, name
        assert (lay.width, lay.height, lay.components, lay.sampling) == (67, 50, 3, 0x22)
        assert coef.size == lay.coef_count == 64 * sum(lay.blocks_w[c] * lay.blocks_h[c] for c in range(3))
        assert coef[:64].any()  # the first block was decoded
    # the cut file ends half way: what follows the first bad block stays zero
    lay, coef, _ = ops.jpeg_entropy_host(by_name("neg_truncated").blob)
    last_row = coef[lay.coef_offset[0]:lay.coef_offset[1]].reshape(lay.blocks_h[0], lay.blocks_w[0], 64)[-1]
    assert not last_row.any()


# ---- the Python layer refuses malformed batches before any library call --------------------------
def _bare_stream(w=16, h=8):
    from droplet_visual_odometry_amd.stream import FrameStream
    fs = FrameStream.__new__(FrameStream)  # no context, no library handle
    fs.width, fs.height, fs.max_frames, fs.nfeatures = w, h, 4, 500
    fs.h = None
    return fs


@pytest.mark.parametrize("name,blobs", [
    ("not a list", b"\xff\xd8\xff"), ("an array", np.zeros(8, np.uint8)), ("empty list", []), ("a string", ["abc", "def"]),
    ("an int", [1, 2]), ("None inside", [b"\xff\xd8", None]), ("empty blob", [b"\xff\xd8", b""]),
    ("2-D array", [np.zeros((2, 2), np.uint8)] * 2), ("float array", [np.zeros(4, np.float32)] * 2),
    ("too many frames", [b"\xff\xd8"] * 5), ("None", None)])
def test_frame_stream_refuses_bad_jpeg_batches(name, blobs):
    fs = _bare_stream()
    rec = torch.zeros(4 * 256, dtype=torch.uint8)
    with pytest.raises(ValueError):
        fs.process_jpeg(blobs)
    with pytest.raises(ValueError):
        fs.submit_jpeg(blobs, rec)


def test_frame_stream_refuses_short_batches_and_other_sizes():
    fs = _bare_stream()
    rec = torch.zeros(4 * 256, dtype=torch.uint8)
    with pytest.raises(ValueError, match=">= 2"):
        fs.submit_jpeg([b"\xff\xd8"], rec)
    u = type("U", (), {"w": 20, "h": 8, "h_": None})()
    with pytest.raises(ValueError, match="undistorter size"):
        fs.process_jpeg([b"\xff\xd8"] * 2, undistort=u)
    with pytest.raises(ValueError, match="undistorter size"):
        fs.submit_jpeg([b"\xff\xd8"] * 2, rec, undistort=u)


def test_decoder_refuses_bad_arguments_before_any_call():
    from droplet_visual_odometry_amd import ops
    d = ops.JpegDecoder.__new__(ops.JpegDecoder)  # no context
    d.max_w, d.max_h, d.h_ = 16, 8, None
    for kw in ({"color": "rgb"}, {"entropy": "gpu"}):
        with pytest.raises(ValueError):
            d.decode([b"\xff\xd8"], **kw)
    with pytest.raises(ValueError):
        d.decode([])
    with pytest.raises(ValueError):
        d.decode(b"\xff\xd8")
