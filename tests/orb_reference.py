"""Float64 reference of ORB's Harris response, intensity-centroid angle and steered rBRIEF descriptor,
written from the ORB paper (Rublee et al. 2011) and OpenCV's documented definitions, NOT from oracle/orb.cpp
or orb.hip, and the checks test_orb_anchors.py (oracle) and test_gpu_orb_anchors.py (device) share.

The level images are inputs to these three: oracle.pyramid(img) and oracle.pyramid(img, blurred=True).  The
second half of the module pins those too, and the keypoint positions: the resize, the blur and FAST from
their definitions (test_detection_anchors.py, test_gpu_detection_anchors.py).  Everything here works at the
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


# ---------------------------------------------------------------------------------------------------------------
# Detection: the pyramid, the descriptor's blur and FAST, from their definitions.  With these the level images
# stop being an input that only the oracle vouches for: test_detection_anchors.py holds oracle.pyramid and
# oracle.fast to them, test_gpu_detection_anchors.py the device's levels and keypoints.
#
#   resize   level l is the bilinear resample of level l - 1: destination d samples the source at
#            (d + 0.5) src / dst - 0.5 on each axis, indices clamped (resize_f64); rounded to 8 bits.
#   blur     the 7-tap Gaussian of sigma 2 with taps rounded to 8 fractional bits, round(256 g / sum g) =
#            [18, 34, 49, 55, 49, 34, 18] (they sum to 257: the gain test_oracle_kats.py documents),
#            REFLECT_101, both passes summed exactly and the result rounded once to 8 bits and saturated
#            (blur_exact returns the unrounded value).
#   FAST     Rosten and Drummond's segment test on the Bresenham circle of radius 3 (16 pixels): a corner has
#            9 contiguous circle pixels all brighter than v + t or all darker than v - t; its score is the
#            largest t at which it is still a corner, i.e. max over the 16 arcs of the arc's smallest
#            difference, less 1; strict 3 x 3 non-maximum suppression on the score (a pixel that is no corner
#            scores 0); rows and columns 3 to size - 4.  Exact integers.
#   ORB      FAST at t = 20 on every level, kept where 31 <= x < w - 31 and 31 <= y < h - 31 (edgeThreshold 31);
#            with nfeatures so high that no level reaches its quota these are the returned keypoints.
#
# Bounds of the resize against resize_f64, in grey levels, 0.5 for the final rounding plus a derived term:
#   4.x  the interpolation weights are rounded to 8 fractional bits and sum to 1, so each pass moves the
#        value by at most 2^-9 |p1 - p0| <= 255 * 2^-9; both passes are otherwise exact: RESIZE_TERM["4.x"]
#        = 2 * 255 * 2^-9 = 0.996.
#   3.2  11-bit weights: 2 * 255 * 2^-12 = 0.125; float32 coordinates: one rounding of a position below 512
#        (2^-15 px) times at most 255 grey / px per axis, 0.016; and the vertical pass truncates the row sums to
#        1 / 128 grey and each of its two products to a quarter grey (test_oracle_kats.py
#        test_opencv32_pyramid_kats), 0.5 + 1 / 128 downwards: RESIZE_TERM["3.2"] = 0.649.  The truncations
#        are OpenCV 3.2's code and not a definition: in them the model is not independent.
# Measured on the committed oracle (test_detection_anchors.py prints them): 1.177 of 1.496 (4.x), 0.782 of
# 1.148 (3.2); blur 0.5 of 0.5 (exact ties, which may round either way).
FAST_THRESHOLD = 20
EDGE_THRESHOLD = 31
RESIZE_TERM = {"4.x": 2 * 255 * 2.0 ** -9, "3.2": 2 * 255 * 2.0 ** -12 + 2 * 255 * 2.0 ** -15 + 0.5 + 1.0 / 128}
BLUR_BOUND = 0.5


def level_shape(w, h, level):
    """(rows, columns) of a level: the side over float32(1.2^level), divided in float32 as OpenCV does (333 / 1.2
    is 277.5 there and rounds to 278), rounded half to even."""
    s = np.float32(1.2 ** level)
    return int(np.rint(np.float32(h) / s)), int(np.rint(np.float32(w) / s))


def resize_f64(src, dh, dw, half_pixel=True):
    out = np.asarray(src).astype(np.float64)
    for axis, dst in ((0, dh), (1, dw)):
        n = out.shape[axis]
        s = (np.arange(dst) + 0.5) * n / dst - 0.5 if half_pixel else np.arange(dst) * (n / dst)
        i0 = np.floor(s).astype(np.int64)
        f = s - i0
        lo, hi = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1)
        shape = [1, 1]
        shape[axis] = -1
        f = f.reshape(shape)
        out = np.take(out, lo, axis=axis) * (1.0 - f) + np.take(out, hi, axis=axis) * f
    return out


def check_pyramid(levels, opencv, label, half_pixel=True):
    """Every level above 0 against the float64 resample of the level below; returns the largest error."""
    worst = 0.0
    for l in range(1, len(levels)):
        want = resize_f64(levels[l - 1], *levels[l].shape, half_pixel=half_pixel)
        worst = max(worst, float(np.abs(levels[l].astype(np.float64) - want).max()))
    print(f"{label} ({opencv}): {len(levels)} levels, resize error max {worst:.3f} grey (bound {0.5 + RESIZE_TERM[opencv]:.3f})")
    return worst


def blur_taps(sigma=2.0):
    g = np.exp(-np.arange(-3, 4) ** 2 / (2.0 * sigma * sigma))
    return np.rint(256.0 * g / g.sum()).astype(np.int64)


def blur_exact(level, sigma=2.0, border="reflect"):
    """The blurred level before its one rounding, as an exact multiple of 2^-16."""
    k = blur_taps(sigma)
    a = np.asarray(level).astype(np.int64)
    h, w = a.shape
    p = np.pad(a, ((0, 0), (3, 3)), mode=border)
    a = sum(k[t] * p[:, t:t + w] for t in range(7))
    p = np.pad(a, ((3, 3), (0, 0)), mode=border)
    return sum(k[t] * p[t:t + h, :] for t in range(7)) / 65536.0


def check_blur(levels, blurred, label, **perturb):
    worst = 0.0
    for L, B in zip(levels, blurred):
        worst = max(worst, float(np.abs(B.astype(np.float64) - np.minimum(blur_exact(L, **perturb), 255.0)).max()))
    print(f"{label}: {len(levels)} levels, blur error max {worst:.4f} grey (bound {BLUR_BOUND})")
    return worst


def bresenham_circle(radius):
    """The circle's pixels (dx, dy) in order around it, from the midpoint algorithm's first octant."""
    x, y, d, octant = 0, radius, 1 - radius, []
    while x <= y:
        octant.append((x, y))
        if d < 0:
            d += 2 * x + 3
        else:
            d += 2 * (x - y) + 5
            y -= 1
        x += 1
    pts = set()
    for x, y in octant:
        pts |= {(x, y), (y, x), (-x, y), (-y, x), (x, -y), (y, -x), (-x, -y), (-y, -x)}
    return sorted(pts, key=lambda p: math.atan2(p[1], p[0]))


assert len(bresenham_circle(3)) == 16 and (1, 3) in bresenham_circle(3) and (2, 2) in bresenham_circle(3)


def fast_scores(img, radius=3, arc=9):
    """int64[h, w]: the largest threshold at which each pixel is still a corner (-1: at none), 0 in the border."""
    circle = bresenham_circle(radius)
    n, b = len(circle), 3
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    out = np.zeros((h, w), np.int64)
    if h <= 2 * b or w <= 2 * b:
        return out
    c = a[b:h - b, b:w - b]
    d = np.stack([a[b + dy:h - b + dy, b + dx:w - b + dx] - c for dx, dy in circle])
    best = np.full(c.shape, -256, np.int64)
    for s in range(n):
        idx = [(s + t) % n for t in range(arc)]
        best = np.maximum(best, np.maximum(d[idx].min(axis=0), (-d[idx]).min(axis=0)))
    out[b:h - b, b:w - b] = best - 1
    return out


def fast(img, threshold=FAST_THRESHOLD, radius=3, arc=9, strict=True):
    """Sorted list of (x, y, score) of the corners that survive non-maximum suppression."""
    s = fast_scores(img, radius, arc)
    s = np.where(s >= threshold, s, 0)
    h, w = s.shape
    p = np.pad(s, 1)
    nb = np.stack([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]).max(axis=0)
    corner = np.zeros((h, w), bool)
    corner[3:h - 3, 3:w - 3] = fast_scores(img, radius, arc)[3:h - 3, 3:w - 3] >= threshold
    keep = corner & ((s > nb) if strict else (s >= nb))
    return sorted((int(x), int(y), int(s[y, x])) for y, x in np.argwhere(keep))


def orb_positions(levels, edge=EDGE_THRESHOLD, **perturb):
    """Per level, the sorted (x, y) of definition-FAST inside the edge threshold."""
    out = []
    for L in levels:
        h, w = L.shape
        out.append(sorted((x, y) for x, y, _ in fast(L, **perturb) if edge <= x < w - edge and edge <= y < h - edge))
    return out


def keypoint_positions(kps, nlevels=8):
    """Per octave, the sorted level positions (x, y) of returned keypoints."""
    scales = [np.float32(1.2 ** l) for l in range(nlevels)]
    out = [[] for _ in range(nlevels)]
    for kp in kps:
        out[int(kp["octave"])].append(level_position(kp, scales))
    return [sorted(p) for p in out]
