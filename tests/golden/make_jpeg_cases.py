"""Writes tests/golden/jpeg_cases.npz: JPEG files made by Pillow (libjpeg-turbo) with
Pillow's own decode of each, the oracle of the JPEG decoder's tests.

    python tests/golden/make_jpeg_cases.py

Cases (see jpeg_cases.load_cases for the reader):
  small     11 sizes x gray / 4:4:4 / 4:2:2 / 4:2:0, each with four restart forms (none, every
            1 and 3 MCUs, every MCU row), content (noise, gradient, saturating checker),
            quality (30, 90, 100) and optimised tables cycling; plus every content x quality at
            33x31 and 67x50 in 4:2:0.  Stored: the file and Pillow's RGB.
  large     320x240 and 640x480 textured frames, 4:2:0, a restart marker every 2 MCUs (more than
            64 and more than 1,024 segments).  Stored: the file, sha256 of the expected BGR and gray.
  stream    4 frames of the synthetic scene at 320x240 as colour JPEGs.  Stored as `large`.
  negative  progressive and 4:4:0 (unsupported); a file cut at half its scan and one whose scan
            is random from the middle on (corrupt entropy-coded data); a DHT cut short (corrupt header).
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "jpeg_cases.npz")

SIZES = [(1, 1), (3, 2), (4, 5), (5, 7), (6, 3), (9, 2), (8, 8), (16, 16), (17, 9), (33, 31), (67, 50)]  # (w, h)
FORMATS = ["gray", "444", "422", "420"]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
CONTENTS = ["noise", "gradient", "checker"]
QUALITIES = [30, 90, 100]
RESTARTS = ["none", "mcu1", "mcu3", "row1"]


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1),
                         ((x + y) * 255) // max(w + h - 2, 1)], -1).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]  # checker of 3 x 2 cells between saturated colours
    on = ((x // 3 + y // 2) & 1).astype(bool)
    a, b = rng.integers(0, 2, 3) * 255, rng.integers(0, 2, 3) * 255
    if (a == b).all():
        b = 255 - a
    return np.where(on[..., None], a, b).astype(np.uint8)


def encode(rgb, fmt, quality, restart="none", optimize=False, **kw):
    im = Image.fromarray(rgb).convert("L") if fmt == "gray" else Image.fromarray(rgb)
    opts = dict(quality=quality, optimize=optimize, **kw)
    if fmt != "gray":
        opts["subsampling"] = SUBSAMPLING[fmt]
    if restart == "mcu1":
        opts["restart_marker_blocks"] = 1
    elif restart == "mcu3":
        opts["restart_marker_blocks"] = 3
    elif restart == "mcu2":
        opts["restart_marker_blocks"] = 2
    elif restart == "row1":
        opts["restart_marker_rows"] = 1
    buf = io.BytesIO()
    im.save(buf, "JPEG", **opts)
    return buf.getvalue()


def decode(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def gray_of_rgb(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def hashes(rgb):
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    return hashlib.sha256(bgr.tobytes()).hexdigest(), hashlib.sha256(gray_of_rgb(rgb).tobytes()).hexdigest()


def texture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(6):
            fx, fy, ph = rng.uniform(0.01, 0.4), rng.uniform(0.01, 0.4), rng.uniform(0, 6.28)
            out[..., c] += rng.uniform(10, 40) * np.sin(fx * x + fy * y + ph)
    out += 128 + rng.normal(0, 12, out.shape)
    return np.clip(out, 0, 255).astype(np.uint8)


def scan_start(blob):
    """Offset of the first entropy-coded byte."""
    i = 2
    while True:
        assert blob[i] == 0xFF
        m, n = blob[i + 1], int.from_bytes(blob[i + 2:i + 4], "big")
        if m == 0xDA:
            return i + 2 + n
        i += 2 + n


def find_marker(blob, marker):
    i = 2
    while True:
        assert blob[i] == 0xFF
        if blob[i + 1] == marker:
            return i
        i += 2 + int.from_bytes(blob[i + 2:i + 4], "big")


def stream_frames():
    """4 frames of the synthetic scene at 320x240 with three different channels, as RGB."""
    sys.path.insert(0, ROOT)
    from droplet_visual_odometry_amd.synth import SceneStream
    st = SceneStream(320, 240)
    fr = np.stack([st.render(i).numpy() for i in range(4)])
    return np.ascontiguousarray(np.stack([fr, np.roll(fr, 3, axis=2), 255 - fr], -1))


def encode_stream_frame(rgb):
    return encode(rgb, "420", 90)


def main():
    cases = []  # (name, kind, blob, rgb or None, probe status, entropy status, sha_bgr, sha_gray)

    def small(w, h, fmt, kind, q, rst, opt, seed):
        blob = encode(content(kind, w, h, seed), fmt, q, rst, opt)
        cases.append((f"{w}x{h}_{fmt}_{kind}_q{q}_{rst}{'_opt' if opt else ''}", "small", blob, decode(blob), 0, 0, "", ""))

    idx = 0
    for (w, h) in SIZES:
        for fmt in FORMATS:
            for r, rst in enumerate(RESTARTS):
                small(w, h, fmt, CONTENTS[(idx + r) % 3], QUALITIES[(idx // 3 + 2 * r) % 3], rst, (idx + r) % 2 == 1,
                      1000 + 4 * idx + r)
            idx += 1
    for (w, h) in [(33, 31), (67, 50)]:
        for kind in CONTENTS:
            for q in QUALITIES:
                small(w, h, "420", kind, q, "none", False, 5000 + w + q)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), "duplicate case"

    for (w, h) in [(320, 240), (640, 480)]:
        blob = encode(texture(w, h, w), "420", 85, "mcu2")
        rgb = decode(blob)
        cases.append((f"large_{w}x{h}", "large", blob, None, 0, 0, *hashes(rgb)))
    for i, rgb in enumerate(stream_frames()):
        blob = encode_stream_frame(rgb)
        cases.append((f"stream_{i}", "stream", blob, None, 0, 0, *hashes(decode(blob))))

    base = content("noise", 67, 50, 77)
    cases.append(("neg_progressive", "negative", encode(base, "420", 90, progressive=True), None, -7, 0, "", ""))
    b422 = bytearray(encode(base, "422", 90))
    sof = find_marker(b422, 0xC0)
    assert b422[sof + 11] == 0x21  # Y sampling 2x1 -> 1x2: the header of a 4:4:0 file (Pillow writes none)
    b422[sof + 11] = 0x12
    cases.append(("neg_440", "negative", bytes(b422), None, -7, 0, "", ""))
    good = encode(base, "420", 90)
    s0 = scan_start(good)
    cases.append(("neg_truncated", "negative", good[:s0 + (len(good) - s0) // 2], None, 0, -8, "", ""))
    rnd = bytearray(good)
    mid = s0 + (len(good) - 2 - s0) // 2
    rnd[mid:len(good) - 2] = np.random.default_rng(5).integers(0, 256, len(good) - 2 - mid, dtype=np.uint8).tobytes()
    for i in range(mid, len(good) - 2):
        if rnd[i] == 0xFF:
            rnd[i + 1] = 0  # FF xx -> FF 00 (the last one may overwrite the FF of EOI: still a marker-free scan)
    if rnd[len(good) - 2] != 0xFF:
        rnd[len(good) - 3] = 0x7F
        rnd[len(good) - 2] = 0xFF
    cases.append(("neg_random_scan", "negative", bytes(rnd), None, 0, -8, "", ""))
    dht = find_marker(good, 0xC4)
    cases.append(("neg_dht_cut", "negative", good[:dht + 12], None, -8, 0, "", ""))

    blobs = [np.frombuffer(c[2], np.uint8) for c in cases]
    rgbs = [c[3].reshape(-1) if c[3] is not None else np.zeros(0, np.uint8) for c in cases]
    np.savez_compressed(
        OUT,
        names=np.array([c[0] for c in cases]), kinds=np.array([c[1] for c in cases]),
        blob_data=np.concatenate(blobs), blob_off=np.cumsum([0] + [b.size for b in blobs]).astype(np.int64),
        rgb_data=np.concatenate(rgbs), rgb_off=np.cumsum([0] + [r.size for r in rgbs]).astype(np.int64),
        shapes=np.array([c[3].shape[:2] if c[3] is not None else (0, 0) for c in cases], np.int32),
        probe_status=np.array([c[4] for c in cases], np.int32), entropy_status=np.array([c[5] for c in cases], np.int32),
        sha_bgr=np.array([c[6] for c in cases]), sha_gray=np.array([c[7] for c in cases]))
    print(OUT, len(cases), "cases,", os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
