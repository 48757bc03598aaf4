"""Float64 reference of ORB's Harris response, intensity-centroid angle and steered rBRIEF descriptor,
written from the ORB paper (Rublee et al. 2011) and OpenCV's documented definitions, NOT from oracle/orb.cpp
or orb.hip, and the checks test_orb_anchors.py (oracle) and test_gpu_orb_anchors.py (device) share.

The level images are inputs: oracle.pyramid(img) and oracle.pyramid(img, blurred=True), which
test_oracle_kats.py pins and test_gpu_pyramid.py compares with the device.  Everything here works at the
keypoint's level position (x, y) = round(pt / scale[octave])."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HALF_PATCH = 15
HARRIS_K = 0.04
HARRIS_NORM = (4.0 * 7 * 255) ** 4   # (2^(3-1) * blockSize * 255)^4: Sobel 3 scale, 7 x 7 block, 8-bit range
ANGLE_TOL_DEG = 0.3                  # the accuracy OpenCV documents for fastAtan2
TIE_EPS = 1e-4                       # half-integer neighbourhood of a rotated pattern coordinate
TIE_SHARE_MAX = 0.005


def umax_table(half=HALF_PATCH):
    """Half-width of each row of the circular patch (the construction test_umax_table_matches_formula pins)."""
    vmax = math.floor(half * np.sqrt(np.float32(2)) / 2 + 1)
    vmin = math.ceil(half * np.sqrt(np.float32(2)) / 2)
    umax = [0] * (half + 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(half * half - v * v)))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:half + 1]


def load_pattern():
    """data/orb_bit_pattern_31.inc as int64[256, 4]: (x0, y0, x1, y1) per test pair."""
    vals = []
    for line in open(os.path.join(HERE, "..", "data", "orb_bit_pattern_31.inc")):
        line = line.split("//")[0]
        vals += [int(t) for t in line.replace(",", " ").split()]
    pat = np.array(vals, np.int64).reshape(-1, 4)
    assert pat.shape == (256, 4)
    return pat


def level_position(kp, scales):
    """Integer level coordinates of a keypoint (pt = level position * scale of its octave)."""
    s = float(scales[int(kp["octave"])])
    return int(np.rint(float(kp["x"]) / s)), int(np.rint(float(kp["y"]) / s))


def harris(level, x, y):
    """(R, a, b, c): Sobel-3 gradients over the 7 x 7 block centred on (x, y);
    R = (a b - c^2 - 0.04 (a + b)^2) / (4 * 7 * 255)^4."""
    I = level.astype(np.float64)
    a = b = c = 0.0
    for j in range(y - 3, y + 4):
        for i in range(x - 3, x + 4):
            ix = 2 * (I[j, i + 1] - I[j, i - 1]) + (I[j - 1, i + 1] - I[j - 1, i - 1]) + (I[j + 1, i + 1] - I[j + 1, i - 1])
            iy = 2 * (I[j + 1, i] - I[j - 1, i]) + (I[j + 1, i - 1] - I[j - 1, i - 1]) + (I[j + 1, i + 1] - I[j - 1, i + 1])
            a += ix * ix
            b += iy * iy
            c += ix * iy
    return (a * b - c * c - HARRIS_K * (a + b) ** 2) / HARRIS_NORM, a, b, c


def ic_angle(level, x, y, umax):
    """Orientation of the intensity centroid, degrees in [0, 360): atan2(m01, m10), u right, v down."""
    I = level.astype(np.float64)
    m10 = m01 = 0.0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = umax[abs(v)]
        u = np.arange(-d, d + 1)
        row = I[y + v, x - d:x + d + 1]
        m10 += float((u * row).sum())
        m01 += v * float(row.sum())
    return math.degrees(math.atan2(m01, m10)) % 360.0


def descriptor(blurred, x, y, angle_deg, pattern):
    """(bits uint8[256], tie bool[256]): bit k is I(p0) < I(p1) for pattern pair k, each point rotated by the
    keypoint's angle to (px cos - py sin, px sin + py cos) and rounded half to even; tie marks the pairs with
    a rotated coordinate within TIE_EPS of a half-integer."""
    t = math.radians(float(angle_deg))
    ca, sa = math.cos(t), math.sin(t)
    px = pattern[:, [0, 2]].astype(np.float64)
    py = pattern[:, [1, 3]].astype(np.float64)
    rx, ry = px * ca - py * sa, px * sa + py * ca
    tie = np.zeros(256, bool)
    for r in (rx, ry):
        tie |= (np.abs(r - np.floor(r) - 0.5) < TIE_EPS).any(axis=1)
    ix, iy = np.rint(rx).astype(np.int64), np.rint(ry).astype(np.int64)
    val = blurred[y + iy, x + ix].astype(np.int64)
    return (val[:, 0] < val[:, 1]).astype(np.uint8), tie


def unpack_bits(desc):
    """uint8[n, 32] -> uint8[n, 256] with pair 8 i + b at bit b (the least significant first) of byte i."""
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little")


HARRIS_ROUNDINGS = 18


def check_features(kps, desc, levels, blurred, scales, label):
    """The three anchors on one set of features; prints what it measured and returns the octaves met.

    Angle: within 0.3 degrees of atan2 (a documented accuracy: OpenCV's for fastAtan2).

    Response: |R - ref| <= n 2^-24 (|a b| + c^2 + 0.04 (a + b)^2) / (4 * 7 * 255)^4, a counted rounding bound
    of the float32 expression ((float)a * b - (float)c * c - k * ((float)a + b) * ((float)a + b)) * s^4 with
    s = 1 / (4 * 7 * 255.f).  Roundings that reach each term, first order: the conversions of its two
    integer sums and their product (3: a b and c^2); k, the two conversions and the sum in each of the two
    factors (a + b), and the two products (1 + 3 + 3 + 2 = 9: the k term); then the subtractions after the
    term (2, 2, 1), s^4 (the division in each of four factors and three products: 7) and the last product
    (1).  That is 13, 13 and 18; n = 18 covers every term.

    Descriptor: every bit equals the reference except pairs with a rotated coordinate within 1e-4 of a
    half-integer.  The float32 angle in radians (<= 2 pi, two roundings), cos and sin and the products and
    sum of a coordinate of magnitude <= 18.4 move it by < 2e-5, so 1e-4 is a 5 x margin; the excluded share
    is capped at 0.5 % of all bits, asserted on the reference's count before the bits are compared."""
    pattern, umax = load_pattern(), umax_table()
    n = len(kps)
    assert n > 0 and desc.shape == (n, 32)
    want_bits = np.zeros((n, 256), np.uint8)
    tie = np.zeros((n, 256), bool)
    ang_err = np.zeros(n)
    resp_ratio = np.zeros(n)
    for i, kp in enumerate(kps):
        o = int(kp["octave"])
        x, y = level_position(kp, scales)
        lh, lw = levels[o].shape
        assert 18 <= x < lw - 18 and 18 <= y < lh - 18, (label, i, x, y, o)
        ang_err[i] = abs((float(kp["angle"]) - ic_angle(levels[o], x, y, umax) + 180.0) % 360.0 - 180.0)
        R, a, b, c = harris(levels[o], x, y)
        unit = 2.0 ** -24 * (abs(a * b) + c * c + HARRIS_K * (a + b) ** 2) / HARRIS_NORM
        resp_ratio[i] = abs(float(kp["response"]) - R) / unit
        want_bits[i], tie[i] = descriptor(blurred[o], x, y, kp["angle"], pattern)
    assert tie.mean() <= TIE_SHARE_MAX, (label, tie.mean())  # the cap, before any bit of `desc` is looked at
    got_bits = unpack_bits(desc)
    wrong = (got_bits != want_bits) & ~tie
    print(f"{label}: {n} keypoints, octaves {sorted(set(int(o) for o in kps['octave']))}; angle error max "
          f"{ang_err.max():.4f} deg; response error max {resp_ratio.max():.2f} * 2^-24 of the terms; "
          f"{int(tie.sum())} of {tie.size} bits excluded as ties, {int(((got_bits != want_bits) & tie).sum())} of "
          f"them differ; {int(wrong.sum())} other bits differ")
    assert ang_err.max() <= ANGLE_TOL_DEG, (label, int(ang_err.argmax()), ang_err.max())
    assert resp_ratio.max() <= HARRIS_ROUNDINGS, (label, int(resp_ratio.argmax()), resp_ratio.max())
    assert not wrong.any(), (label, np.argwhere(wrong)[:8].tolist())
    return set(int(o) for o in kps["octave"])


def small_image():
    """The 161 x 97 image of test_gpu_edge.py's test_detect_small_and_odd_sizes."""
    w, h = 161, 97
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return np.ascontiguousarray(np.clip(img.astype(np.int32) // 2 + np.add.outer(np.arange(h), np.arange(w)) % 128,
                                        0, 255).astype(np.uint8))
