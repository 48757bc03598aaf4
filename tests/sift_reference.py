"""Float64 model of SIFT's scale space, orientation assignment, descriptor and sub-pixel refinement, written
from Lowe (2004) and OpenCV's documented definitions of SIFT_create(), NOT from oracle/sift.cpp or sift.hip,
and the check test_descriptor_anchors.py (oracle) and test_gpu_descriptor_anchors.py (device) share.  The
last part of the module is the detection model (which keypoints exist), described where it begins.

The model takes the 8-bit image and the keypoint records only.  Everything is a function of the pixels:

  scale space   2x bilinear upscale (half-pixel mapping, edge samples clamped), blur by sqrt(1.6^2 - 4 0.5^2),
                octaves of 6 layers with sigmas sqrt((1.6 k^i)^2 - (1.6 k^(i-1))^2), k = 2^(1/3), kernel length
                round(8 sigma + 1) | 1, taps normalised, REFLECT_101; layer 0 of the next octave is every second
                pixel of layer 3.  OpenCV builds round(log2(min side of the upscaled image) - 2) octaves (plus
                the upscaled one); the model builds an octave when a keypoint names it.
  keypoint      octave = signed low byte, layer = bits 8..15, scale = 2^-octave, level (octave + 1) * 6 + layer,
                level point = pt * scale, s = size * scale / 2, descriptor angle 360 - kp.angle.
  orientation   36 bins of the angle of (right - left, up - down) over radius round(4.5 s), weight
                exp(-(i^2 + j^2) / (2 (1.5 s)^2)) * magnitude, [1 4 6 4 1] / 16 circular smoothing, peaks that are
                local maxima >= 0.8 max, parabolic interpolation, angle = 360 - 10 bin.
  descriptor    4 x 4 x 8 trilinear histogram over radius round(3 s sqrt(2) 2.5) (at most the level's diagonal),
                sample (i, j) at (j cos - i sin, j sin + i cos) / (3 s) + 1.5 bins, weight exp(-r^2 / 8), interior
                pixels only, circular orientation bins, normalise, clip at 0.2 of the norm, renormalise to 512.
  refinement    at the keypoint's octave, layer and rounded level position: DoG value D, gradient g and Hessian
                H by the central differences of Lowe section 4 (pixels scaled to [0, 1]), offset x = -H^-1 g.

Bin ties.  OpenCV takes the sample angle from fastAtan2 and the bin from round(angle / 10).  fastAtan2 is a
published degree-7 polynomial, within 0.00955 degrees of atan2 (fast_atan2_error(); the documentation says
"about 0.3 degrees"); the model evaluates it in float64 (fast_atan2), so what is left between the model's
sample angle and a float32 implementation's is the float32 evaluation (FAST_ATAN2_EVAL_DEG) and the float32
pyramid under the gradient (2 sqrt(2) PYR_ERR / magnitude, in radians).  A sample whose angle lies within that
of a bin boundary, or whose |dx| and |dy| agree to within 4 PYR_ERR (the polynomial's two branches give
44.9904 and 45.0096 degrees there, either side of a boundary), can fall in either bin.  The histogram is
built three times (such samples to the lower bin, to the upper bin, to the nearest) and a keypoint is
DECIDED when the three give the same number of peaks and corresponding peaks lie within 0.3 degrees of each
other.  Radial gradient fields (symmetric blobs) have samples at exactly 45, 135, ... degrees and a nearly flat
histogram: they are undecided by construction.  A band of 0.3 degrees around every boundary, the documented
accuracy taken literally, holds 6 % of all samples; sending them all down or all up is the same as moving
every boundary by 0.3 degrees, which moves every peak by about as much, and 129 of the 150 keypoints of the
cases are then undecided by the model alone, whatever the detector returns.

Not from a paper or the documentation: the floor max(sigma^2 - 4 0.5^2, 0.01) under the first blur's square root,
the rounding of the level position half to even and the polynomial's coefficients are OpenCV's source, which
the oracle restates too.  The first two change nothing at sigma 1.6; the third is tied to atan2 by
fast_atan2_error(), which test_descriptor_anchors.py asserts.  In these details the model is not independent."""
import math

import numpy as np

N_LAYERS = 3                 # nOctaveLayers; 6 Gaussian layers per octave
ORI_BINS = 36
DECIDED_DEG = 0.3

# Tolerances of check_features.  Each is at most 4 x the maximum measured on the committed oracle over the
# cases of test_descriptor_anchors.py (printed there and repeated in its docstring), under a ceiling: 0.05 of an
# 8-bit count for the float32 accumulation of the descriptor, 0.3 degrees for an angle.
EPS = 0.04                   # measured 0.0102 (edge_blobs); 4 x is 0.0408, ceiling 0.05
TOL_DEG = 0.0003             # measured 0.000077 on decided keypoints (anchor); 4 x is 0.00031, ceiling 0.3
COND_MAX = 100.0             # refinement: Hessians worse conditioned than this are skipped (and counted)


def gaussian_taps(sigma):
    n = int(np.rint(8.0 * sigma + 1.0)) | 1
    x = np.arange(n) - (n - 1) / 2.0
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return k / k.sum()


def blur(a, sigma):
    """Separable Gaussian, REFLECT_101 (numpy's 'reflect')."""
    k = gaussian_taps(sigma)
    r = len(k) // 2
    h, w = a.shape
    p = np.pad(a, ((0, 0), (r, r)), mode="reflect")
    a = sum(k[t] * p[:, t:t + w] for t in range(len(k)))
    p = np.pad(a, ((r, r), (0, 0)), mode="reflect")
    return sum(k[t] * p[t:t + h, :] for t in range(len(k)))


def upscale2(a):
    """2x bilinear: destination d samples the source at (d + 0.5) / 2 - 0.5, indices clamped."""
    out = a
    for axis in (0, 1):
        n = out.shape[axis]
        s = (np.arange(2 * n) + 0.5) / 2.0 - 0.5
        i0 = np.floor(s).astype(np.int64)
        f = s - i0
        lo, hi = np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1)
        shape = [1, 1]
        shape[axis] = -1
        f = f.reshape(shape)
        out = np.take(out, lo, axis=axis) * (1.0 - f) + np.take(out, hi, axis=axis) * f
    return out


class ScaleSpace:
    """Gaussian levels of one image, octaves built on demand; level(octave, layer) with octave from -1."""

    def __init__(self, img, base_sigma=1.6):
        self.sigma = float(base_sigma)
        up = upscale2(np.asarray(img).astype(np.float64))
        self.octaves = [self._octave(blur(up, math.sqrt(max(self.sigma ** 2 - 4 * 0.5 ** 2, 0.01))))]

    def _octave(self, base):
        k = 2.0 ** (1.0 / N_LAYERS)
        layers = [base]
        for i in range(1, N_LAYERS + 3):
            prev, total = self.sigma * k ** (i - 1), self.sigma * k ** i
            layers.append(blur(layers[-1], math.sqrt(total * total - prev * prev)))
        return layers

    def level(self, octave, layer):
        assert octave >= -1 and 0 <= layer < N_LAYERS + 3
        while len(self.octaves) <= octave + 1:
            src = self.octaves[-1][N_LAYERS]
            h, w = src.shape
            assert h // 2 >= 1 and w // 2 >= 1
            self.octaves.append(self._octave(src[0:2 * (h // 2):2, 0:2 * (w // 2):2]))
        return self.octaves[octave + 1][layer]

    def dog(self, octave, layer):
        return self.level(octave, layer + 1) - self.level(octave, layer)


def unpack(kp):
    """(octave, layer, interpolated-layer byte, scale, level x, level y, s)."""
    o = int(kp["octave"])
    octave, layer, xi_byte = o & 255, (o >> 8) & 255, (o >> 16) & 255
    if octave >= 128:
        octave -= 256
    scale = 2.0 ** -octave
    return octave, layer, xi_byte, scale, float(kp["x"]) * scale, float(kp["y"]) * scale, float(kp["size"]) * scale * 0.5


def _gradients(L, y, x):
    dx = L[y, x + 1] - L[y, x - 1]
    dy = L[y - 1, x] - L[y + 1, x]
    return np.degrees(np.arctan2(dy, dx)) % 360.0, np.hypot(dx, dy)


def _smooth_matrix():
    """The [1 4 6 4 1] / 16 circular smoothing as a 36 x 36 matrix."""
    S = np.zeros((ORI_BINS, ORI_BINS))
    for j in range(ORI_BINS):
        for d, c in ((-2, 1.0), (-1, 4.0), (0, 6.0), (1, 4.0), (2, 1.0)):
            S[j, (j + d) % ORI_BINS] += c / 16.0
    return S


SMOOTH = _smooth_matrix()


def _peaks(raw):
    """Keypoint angles (degrees) of the peaks of a raw 36-bin histogram."""
    n = ORI_BINS
    h = SMOOTH @ raw
    out = []
    for j in range(n):
        l, r = h[(j - 1) % n], h[(j + 1) % n]
        if h[j] > l and h[j] > r and h[j] >= 0.8 * h.max():
            b = (j + 0.5 * (l - r) / (l - 2.0 * h[j] + r)) % n
            out.append((360.0 - 10.0 * b) % 360.0)
    return np.array(sorted(out))


def circ_diff(a, b):
    return np.abs((np.asarray(a) - np.asarray(b) + 180.0) % 360.0 - 180.0)


FAST_ATAN2_P = (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)
# float32 evaluation of fast_atan2: the quotient, its square, four multiply-adds and the last product carry at
# most 12 roundings relative to a value <= 45 degrees, and 90 - a, 180 - a, 360 - a one each of a value <= 360:
# 12 * 2^-24 * 45 + 3 * 2^-24 * 360 = 9.7e-5 degrees.
FAST_ATAN2_EVAL_DEG = 1e-4


def fast_atan2(y, x, branch=None):
    """The polynomial OpenCV publishes for fastAtan2, in float64, degrees in [0, 360): with c the smaller of
    |x|, |y| over the larger, a = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c * 180 / pi where |x| >= |y| (branch 0),
    90 - that otherwise (branch 1), then 180 - a where x < 0 and 360 - a where y < 0.  branch forces one."""
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay if branch is None else np.full(np.shape(ax), branch == 0)
    c = np.where(first, ay, ax) / np.maximum(np.where(first, ax, ay), 1e-300)
    c2 = c * c
    p1, p3, p5, p7 = FAST_ATAN2_P
    a = np.degrees((((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c)
    a = np.where(first, a, 90.0 - a)
    a = np.where(x < 0, 180.0 - a, a)
    return np.where(y < 0, 360.0 - a, a) % 360.0


def fast_atan2_error():
    """Largest distance, in degrees, of fast_atan2 from atan2 (the documentation says "about 0.3 degrees"):
    0.00955.  The model's sample angles are anchored to atan2 by this."""
    t = np.radians(np.linspace(0.0, 360.0, 720001))
    y, x = np.sin(t), np.cos(t)
    return float(circ_diff(fast_atan2(y, x), np.degrees(t) % 360.0).max())


class Orientation:
    """The orientation model of one keypoint position: variants = the peaks with tie samples sent to the
    nearest bin, to the lower and to the upper; decided; and the data reachable() needs."""

    def __init__(self, L, px, py, s):
        rows, cols = L.shape
        c, r = int(np.rint(px)), int(np.rint(py))
        radius = int(np.rint(4.5 * s))
        i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
        y, x = r + i, c + j
        m = (y > 0) & (y < rows - 1) & (x > 0) & (x < cols - 1)
        i, j, y, x = i[m], j[m], y[m], x[m]
        dx, dy = L[y, x + 1] - L[y, x - 1], L[y - 1, x] - L[y + 1, x]
        mag = np.hypot(dx, dy)
        w = np.exp(-(i * i + j * j) / (2.0 * (1.5 * s) ** 2)) * mag
        t = fast_atan2(dy, dx) / 10.0
        lo = np.floor(t)
        noise = FAST_ATAN2_EVAL_DEG + np.degrees(2.0 * math.sqrt(2.0) * PYR_ERR / np.maximum(mag, 1e-300))
        tie = np.abs(t - lo - 0.5) * 10.0 < noise
        nearest = np.rint(t)
        # |dx| = |dy| to within the pyramid's error: either branch of the polynomial, which lie on the two
        # sides of the bin boundary at 45, 135, 225, 315 degrees
        either = np.abs(np.abs(dx) - np.abs(dy)) <= 4.0 * PYR_ERR
        b0, b1 = np.rint(fast_atan2(dy, dx, 0) / 10.0), np.rint(fast_atan2(dy, dx, 1) / 10.0)
        swap = either & (b0 != b1)
        lo, tie = np.where(swap, np.minimum(b0, b1), lo), tie | swap

        def hist(b, weights=w):
            return np.bincount(b.astype(np.int64) % ORI_BINS, weights=weights, minlength=ORI_BINS)

        self.raw_lower = hist(np.where(tie, lo, nearest))
        self.tie_weight = hist(lo[tie], w[tie])      # [b]: weight that may move from bin b to bin b + 1
        self.tie_share = float(w[tie].sum() / max(w.sum(), 1e-300))
        self.variants = [_peaks(hist(nearest)), _peaks(self.raw_lower), _peaks(hist(np.where(tie, lo + 1, nearest)))]
        a = self.variants[0]
        self.decided = all(len(v) == len(a) and all(circ_diff(p, a).min() <= DECIDED_DEG for p in v) and
                           all(circ_diff(p, v).min() <= DECIDED_DEG for p in a) for v in self.variants[1:])

    def reachable(self, angle, tol):
        """Whether some split of the tie weights gives a peak within tol of `angle`.  Moving m[b] in
        [0, tie_weight[b]] from bin b to b + 1 makes the smoothed histogram h = SMOOTH (raw_lower + M m), linear
        in m.  A peak at bin j with offset d = position - j needs (l - r) / 2 - d (l - 2 h[j] + r) = 0 with
        |d| <= 0.5, h[j] > l, h[j] > r and h[j] >= 0.8 h[k] for every k.  Each of these is linear in m, so
        its range over the box of m is a sum of per-coordinate extremes; the test asks that 0 lies in the
        range of the first for some d within tol, and that each inequality can hold on its own.  It is a
        necessary condition only (the box contains every discrete assignment, and the inequalities are not
        required to hold together), and a loose one where the histogram is flat: at the pixel-centred blob of
        detector_cases.anchor() (5.7 % of the weight in ties) it accepts 36 % of the circle at a step of
        0.25 degrees, at the undecided positions of corner_blobs_96 0.2 to 3 %, where the union of the
        variants' peaks within TOL_DEG covers about 0.001 %.  check_features therefore uses it only for
        keypoints its caller names."""
        n = ORI_BINS
        M = np.zeros((n, n))
        for b in range(n):
            M[b, b] -= 1.0
            M[(b + 1) % n, b] += 1.0
        h0, dh = SMOOTH @ self.raw_lower, (SMOOTH @ M) * self.tie_weight[None, :]   # h = h0 + dh @ u, u in [0, 1]^36

        def span(row0, row):
            return row0 + np.minimum(row, 0.0).sum(), row0 + np.maximum(row, 0.0).sum()

        pos = ((360.0 - angle) / 10.0) % n
        for j in {int(np.floor(pos)) % n, int(np.ceil(pos)) % n}:
            l, r = (j - 1) % n, (j + 1) % n
            d = (pos - j + n / 2.0) % n - n / 2.0
            if not all(span(h0[j] - h0[k], dh[j] - dh[k])[1] > 0 for k in (l, r)):
                continue
            if not all(span(h0[j] - 0.8 * h0[k], dh[j] - 0.8 * dh[k])[1] >= 0 for k in range(n)):
                continue
            lows, highs = [], []
            for dd in (d - tol / 10.0, d + tol / 10.0):
                if abs(dd) > 0.5 + tol / 10.0:
                    continue
                f_lo, f_hi = span(0.5 * (h0[l] - h0[r]) - dd * (h0[l] - 2 * h0[j] + h0[r]),
                                  0.5 * (dh[l] - dh[r]) - dd * (dh[l] - 2 * dh[j] + dh[r]))
                lows.append(f_lo)
                highs.append(f_hi)
            if lows and min(lows) <= 0.0 <= max(highs):
                return True
        return False


def descriptor(L, px, py, ori_deg, s):
    """The 128 entries before rounding to 8 bits, entry (row cell * 4 + column cell) * 8 + orientation bin."""
    rows, cols = L.shape
    c, r = int(np.rint(px)), int(np.rint(py))
    hw = 3.0 * s
    radius = min(int(np.rint(hw * math.sqrt(2.0) * 2.5)), int(math.sqrt(cols * cols + rows * rows)))
    t = math.radians(ori_deg)
    ct, st = math.cos(t) / hw, math.sin(t) / hw
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    c_rot, r_rot = j * ct - i * st, j * st + i * ct
    rbin, cbin = r_rot + 1.5, c_rot + 1.5
    y, x = r + i, c + j
    m = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (y > 0) & (y < rows - 1) & (x > 0) & (x < cols - 1)
    rbin, cbin, c_rot, r_rot, y, x = rbin[m], cbin[m], c_rot[m], r_rot[m], y[m], x[m]
    ang, mag = _gradients(L, y, x)
    mag = mag * np.exp(-(c_rot * c_rot + r_rot * r_rot) / 8.0)
    obin = (ang - ori_deg) * 8.0 / 360.0
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    hist = np.zeros((6, 6, 8))
    for dr, wr in ((0, 1.0 - fr), (1, fr)):
        for dc, wc in ((0, 1.0 - fc), (1, fc)):
            for do, wo in ((0, 1.0 - fo), (1, fo)):
                np.add.at(hist, (r0 + 1 + dr, c0 + 1 + dc, (o0 + do) % 8), mag * wr * wc * wo)
    v = hist[1:5, 1:5, :].reshape(128)
    v = np.minimum(v, 0.2 * math.sqrt(float((v * v).sum())))
    return v * 512.0 / max(math.sqrt(float((v * v).sum())), 1e-30)


def refinement(ss, octave, layer, c, r):
    """(D, g, H, x) of the DoG at (c, r, layer): central differences, pixels scaled to [0, 1]; x = -H^-1 g,
    ordered (column, row, layer)."""
    p, q, n = ss.dog(octave, layer - 1) / 255.0, ss.dog(octave, layer) / 255.0, ss.dog(octave, layer + 1) / 255.0
    g = np.array([(q[r, c + 1] - q[r, c - 1]) / 2.0, (q[r + 1, c] - q[r - 1, c]) / 2.0, (n[r, c] - p[r, c]) / 2.0])
    v2 = 2.0 * q[r, c]
    dxx, dyy, dss = q[r, c + 1] + q[r, c - 1] - v2, q[r + 1, c] + q[r - 1, c] - v2, n[r, c] + p[r, c] - v2
    dxy = (q[r + 1, c + 1] - q[r + 1, c - 1] - q[r - 1, c + 1] + q[r - 1, c - 1]) / 4.0
    dxs = (n[r, c + 1] - n[r, c - 1] - p[r, c + 1] + p[r, c - 1]) / 4.0
    dys = (n[r + 1, c] - n[r - 1, c] - p[r + 1, c] + p[r - 1, c]) / 4.0
    H = np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])
    return float(q[r, c]), g, H, -np.linalg.solve(H, g)


# The float32 pyramid against the float64 one, PYR_ERR grey levels per level sample.  A worst-case count is
# useless here (27 taps, two passes per blur and a dozen blurs in a chain give over 100 roundings of 255), so this is
# a statistical estimate, as the refinement and the tie band of the orientation need one.  With U = 2^-24, a pass
# forms n <= 27 products t[k] v[k] and n - 1 sums, each rounded by at most U relative to its result, U / sqrt(3)
# rms.  The products add U / sqrt(3) * v * sqrt(sum t^2) <= 0.3 U v; the partial sums are at most v, so the
# sums add at most U / sqrt(3) * v * sqrt(26) = 2.9 U v: 3 U v rms per pass, v <= 255.  The next pass averages
# the error it is handed, which is white: its rms falls by sqrt(sum t^2) = sqrt(1 / (2 sigma sqrt(pi))) <= 0.5 at
# sigma >= 1.2, so a chain of passes carries at most 3 U v / sqrt(1 - 0.25) = 3.5 U v rms.  Four standard
# deviations (one sample in 16000; no case has that many that matter): PYR_ERR = 14 U * 255.
#
# Refinement: in [0, 1] units a DoG sample carries e = 2 PYR_ERR / 255, g e per entry, H at most 4 e per entry
# (row sums at most 12 e), and to first order |dx| <= |H^-1|_inf (|dg|_inf + |dH|_inf |x|_inf)
#   <= |H^-1|_inf (e + 12 e * 0.5).  D + g.x / 2 moves by at most e + 3 (e * 0.5 + |g|_inf |dx|) / 2.
PYR_ERR = 14 * 2.0 ** -24 * 255


def check_refinement(ss, kp):
    """None when the Hessian is worse conditioned than COND_MAX; else (position error / its bound, size error
    / its bound, response error / its bound, layer-byte error in counts)."""
    octave, layer, xi_byte, scale, px, py, _ = unpack(kp)
    c, r = int(np.rint(px)), int(np.rint(py))
    D, g, H, x = refinement(ss, octave, layer, c, r)
    if np.linalg.cond(H) > COND_MAX:
        return None
    e = 2.0 * PYR_ERR / 255.0
    dx = float(np.abs(np.linalg.inv(H)).sum(axis=1).max()) * 7.0 * e
    pos = max(abs(px - (c + x[0])), abs(py - (r + x[1]))) / (dx + 2.0 ** -23 * max(px, py, 1.0))
    byte = abs(xi_byte - (x[2] + 0.5) * 255.0) / (0.5 + 255.0 * dx)
    want_size = 1.6 * 2.0 ** ((layer + x[2]) / 3.0) * 2.0 ** octave * 2.0
    size = abs(float(kp["size"]) / want_size - 1.0) / (math.log(2.0) / 3.0 * dx * 1.01 + 2.0 ** -20)
    dresp = e + 1.5 * (0.5 * e + float(np.abs(g).max()) * dx) + 2.0 ** -20
    resp = abs(float(kp["response"]) - abs(D + 0.5 * float(g @ x))) / dresp
    return pos, size, resp, byte


def group_key(kp):
    return (float(kp["x"]), float(kp["y"]), float(kp["size"]), int(kp["octave"]))


def check_features(img, kps, desc, label, base_sigma=1.6, max_keypoints=None, refine=True, split_ok=()):
    """The SIFT anchors on one image's features; prints what it measured and returns the figures.

    Descriptor: every entry d satisfies |d - min(v64, 255)| <= 0.5 + EPS, v64 the model's unrounded entry
    computed for the keypoint's own angle: d is v64 rounded to 8 bits and saturated.  No entry is exempt.
    Orientation: a decided keypoint's angle lies within TOL_DEG of a model peak, and every model peak is the
    angle of a keypoint with the same position, size and octave field (duplicates that removeDuplicatedSorted
    merges have the same angle, so the set is unchanged); an undecided keypoint's angle lies within TOL_DEG
    of a peak of one of the three variants.  split_ok names keypoints (x, y, angle) for which, failing that,
    Orientation.reachable may stand in: an angle that some split of the tie weights between the two bins
    can reach (the three variants are three corners of that set, and an implementation may send each tie
    sample either way).  That test is far looser than the union (reachable's docstring says how far), so it
    is open to no keypoint that the caller does not name, and the names used are returned (by_split).
    Refinement (refine=True): the stored position, layer byte, size and response against x = -H^-1 g, each
    within the first-order bound stated at PYR_ERR; ill-conditioned Hessians are skipped and counted.
    max_keypoints: check that many keypoints, chosen at a fixed stride over the list."""
    n = len(kps)
    assert n > 0 and desc.shape == (n, 128), (label, n, desc.shape)
    ss = ScaleSpace(img, base_sigma)
    chosen = np.arange(n) if not max_keypoints or n <= max_keypoints else np.arange(max_keypoints) * n // max_keypoints
    groups = {}
    for kp in kps:
        groups.setdefault(group_key(kp), []).append(float(kp["angle"]))
    model = {}
    entry_err, ang_err, und_err, undecided, by_split, skipped, saturated, bad = 0.0, 0.0, 0.0, 0, [], 0, 0, []
    ref_worst = np.zeros(4)
    octaves, layers = set(), set()
    for i in chosen:
        kp = kps[i]
        octave, layer, _, _, px, py, s = unpack(kp)
        octaves.add(octave)
        layers.add(layer)
        L = ss.level(octave, layer)
        v = descriptor(L, px, py, 360.0 - float(kp["angle"]), s)
        saturated += int((v > 255.0).sum())
        err = np.abs(desc[i].astype(np.float64) - np.minimum(v, 255.0))
        if err.max() > 0.5 + EPS:
            bad.append(("descriptor", int(i), int(err.argmax()), float(err.max()) - 0.5))
        entry_err = max(entry_err, float(err.max()) - 0.5)
        key = group_key(kp)
        if key not in model:
            model[key] = Orientation(L, px, py, s)
        variants, decided = model[key].variants, model[key].decided
        if decided:
            d = float(circ_diff(float(kp["angle"]), variants[0]).min())
            ang_err = max(ang_err, d)
            if d > TOL_DEG:
                bad.append(("angle", int(i), float(kp["angle"]), variants[0].tolist()))
            for p in variants[0]:
                d = float(circ_diff(p, groups[key]).min())
                ang_err = max(ang_err, d)
                if d > TOL_DEG:
                    bad.append(("model peak without keypoint", int(i), float(p), groups[key]))
        else:
            undecided += 1
            union = np.concatenate(variants)
            d = float(circ_diff(float(kp["angle"]), union).min()) if len(union) else 360.0
            if d <= TOL_DEG:
                und_err = max(und_err, d)
            else:
                named = any(abs(float(kp["x"]) - x) <= 0.01 and abs(float(kp["y"]) - y) <= 0.01 and
                            circ_diff(float(kp["angle"]), a) <= 0.001 for x, y, a in split_ok)
                if named and model[key].reachable(float(kp["angle"]), TOL_DEG):
                    by_split.append((int(i), float(kp["angle"]), d))
                else:
                    bad.append(("angle (undecided)", int(i), float(kp["angle"]), d, union.tolist()))
        if refine:
            res = check_refinement(ss, kp)
            if res is None:
                skipped += 1
            else:
                ref_worst = np.maximum(ref_worst, res)
    print(f"{label}: {len(chosen)} of {n} keypoints, octaves {sorted(octaves)}, layers {sorted(layers)}; descriptor "
          f"|d - v64| - 0.5 max {entry_err:.4f}, {saturated} entries above 255; angle error max {ang_err:.6f} deg on "
          f"decided keypoints, {undecided} undecided (those held to a variant's peak within {und_err:.6f}; held to a split of the tie "
          f"weights instead: {[(i, round(a, 3), round(d, 4)) for i, a, d in by_split]}); refinement {skipped} skipped, error / bound: position "
          f"{ref_worst[0]:.3f} size {ref_worst[1]:.3f} response {ref_worst[2]:.3f} layer byte {ref_worst[3]:.3f}")
    assert not bad, (label, len(bad), bad[:6])
    assert ref_worst.max() <= 1.0, (label, "refinement", ref_worst.tolist())
    return dict(checked=len(chosen), undecided=undecided, skipped=skipped, entry_err=entry_err, ang_err=ang_err,
                octaves=octaves, layers=layers, saturated=saturated, by_split=by_split)


# ---------------------------------------------------------------------------------------------------------------
# Detection: which keypoints exist, as a function of the pixels (Lowe 2004 sections 3 to 4.1, OpenCV's
# documented SIFT_create(nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10)).
#
#   search      every octave from -1 upward while rows and columns beyond a border of 5 remain, DoG layers 1 to 3
#   candidate   |D| (in grey levels) above floor(0.5 * 0.04 / 3 * 255) = 1 and, with D > 0, D >= each of the 26
#               neighbours of the 3 x 3 x 3 cube (D < 0: <=)
#   refinement  x = -H^-1 g (refinement() above); accepted when all three |x| < 0.5, otherwise the cell moves by
#               round(x) and the solve is repeated, five solves at the most; a cell that leaves layers 1 to 3 or
#               the border is rejected, and so is a fifth solve that still asks for a move
#   contrast    |D + g.x / 2| * 3 >= 0.04, pixels scaled to [0, 1]
#   edge        on the 2 x 2 spatial Hessian: det > 0 and tr^2 * 10 < 11^2 * det
#
# Every comparison is made with the error its operands carry in a float32 implementation: a DoG sample carries
# e = 2 PYR_ERR / 255 (PYR_ERR above), a difference of two 2 e, x carries dx = |H^-1|_inf * 7 e, the contrast
# e + 1.5 (e / 2 + |g|_inf dx), as derived at PYR_ERR; the spatial second differences carry 4 e (dxx, dyy) and e
# (dxy), so det carries 4 e (|dxx| + |dyy|) + 2 e |dxy| and 121 det - 10 tr^2 carries 121 times that plus
# 20 |tr| 8 e.  A comparison whose margin exceeds its error is decided; a candidate all of whose comparisons
# are decided is DECIDED present or absent; any comparison inside its error makes every cell the candidate
# can still reach UNDECIDED: both outcomes are followed, a move whose rounding can go either way to both
# cells.  Where dx exceeds 1 (a Hessian too ill conditioned to say where a float32 solve goes) the 3 x 3 x 3
# cube around the cell is undecided and the path ends.
#
# Not from the paper or the documentation: >= rather than > in the extremum test (it differs on exact ties
# only, which are inside the error and so undecided), five solves rather than five moves, the floor in the
# pre-threshold, and a singular H giving x = 0 are OpenCV's source, which the oracle restates too.  The last
# cannot occur unnoticed here: a singular float64 H has dx = infinity and is undecided.
DET_BORDER = 5
DET_CONTRAST = 0.04
DET_EDGE = 10.0
DET_ACCEPT = 0.5
DET_STEPS = 5
DET_E = 2.0 * PYR_ERR / 255.0
_N26 = [(dl, dr, dc) for dl in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dl, dr, dc) != (0, 0, 0)]
_N18 = [d for d in _N26 if 0 in d]   # without the cube's eight corners
assert len(_N18) == 18


class DetectionModel:
    """The keypoint cells (octave, layer, row, column) of one image: present (decided) and undecided.
    The keyword arguments are the parameters the negative controls of test_detection_anchors.py perturb."""

    def __init__(self, img, border=DET_BORDER, neighbours=26, contrast=DET_CONTRAST, edge=DET_EDGE, accept=DET_ACCEPT,
                 prethreshold=1.0):
        self.border, self.contrast, self.edge, self.accept = border, contrast, edge, accept
        self.offsets = _N26 if neighbours == 26 else _N18
        self.pre = math.floor(0.5 * DET_CONTRAST / N_LAYERS * 255.0) * prethreshold / 255.0
        self.ss = ScaleSpace(img)
        self.present, self.undecided = set(), set()
        self.candidates = 0
        h, w = np.asarray(img).shape
        h, w, octave = 2 * h, 2 * w, -1
        while h > 2 * border and w > 2 * border:
            self._octave(octave)
            h, w, octave = h // 2, w // 2, octave + 1
        self.octaves = octave + 1   # searched: -1 .. octave - 1
        self.undecided -= self.present

    def _octave(self, octave):
        b, e = self.border, DET_E
        D = np.stack([self.ss.dog(octave, l) for l in range(N_LAYERS + 2)]) / 255.0
        self.D = D
        _, h, w = D.shape
        core = D[1:N_LAYERS + 1, b:h - b, b:w - b]
        nb = np.stack([D[1 + dl:N_LAYERS + 1 + dl, b + dr:h - b + dr, b + dc:w - b + dc] for dl, dr, dc in self.offsets])
        hi, lo = nb.max(axis=0), nb.min(axis=0)
        # possible: no comparison decided against; certain: every comparison decided for
        pos_p = (core > self.pre - e) & (core > -e) & (core >= hi - 2 * e)
        neg_p = (core < -self.pre + e) & (core < e) & (core <= lo + 2 * e)
        pos_c = (core > self.pre + e) & (core >= hi + 2 * e)
        neg_c = (core < -self.pre - e) & (core <= lo - 2 * e)
        certain = pos_c | neg_c
        for l, r, c in np.argwhere(pos_p | neg_p):
            self.candidates += 1
            self._refine(octave, int(l) + 1, int(r) + b, int(c) + b, 0, bool(certain[l, r, c]))

    def _at(self, layer, r, c):
        """(D, g, H) at a cell of self.D (the same differences as refinement())."""
        p, q, n = self.D[layer - 1], self.D[layer], self.D[layer + 1]
        g = np.array([(q[r, c + 1] - q[r, c - 1]) / 2.0, (q[r + 1, c] - q[r - 1, c]) / 2.0, (n[r, c] - p[r, c]) / 2.0])
        v2 = 2.0 * q[r, c]
        dxx, dyy, dss = q[r, c + 1] + q[r, c - 1] - v2, q[r + 1, c] + q[r - 1, c] - v2, n[r, c] + p[r, c] - v2
        dxy = (q[r + 1, c + 1] - q[r + 1, c - 1] - q[r - 1, c + 1] + q[r - 1, c - 1]) / 4.0
        dxs = (n[r, c + 1] - n[r, c - 1] - p[r, c + 1] + p[r, c - 1]) / 4.0
        dys = (n[r + 1, c] - n[r - 1, c] - p[r + 1, c] + p[r - 1, c]) / 4.0
        return float(q[r, c]), g, np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]])

    def _inside(self, layer, r, c):
        _, h, w = self.D.shape
        return 1 <= layer <= N_LAYERS and self.border <= r < h - self.border and self.border <= c < w - self.border

    def _refine(self, octave, layer, r, c, step, sure):
        e = DET_E
        D, g, H = self._at(layer, r, c)
        try:
            Hi = np.linalg.inv(H)
            x = -Hi @ g
            dx = float(np.abs(Hi).sum(axis=1).max()) * 7.0 * e
        except np.linalg.LinAlgError:
            x, dx = np.zeros(3), np.inf
        if not np.isfinite(dx) or dx > 1.0 or not np.isfinite(x).all():
            for dl, dr, dc in _N26 + [(0, 0, 0)]:
                if self._inside(layer + dl, r + dr, c + dc):
                    self.undecided.add((octave, layer + dl, r + dr, c + dc))
            return
        ax = np.abs(x)
        may_accept, must_accept = bool((ax < self.accept + dx).all()), bool((ax < self.accept - dx).all())
        if may_accept:
            self._tests(octave, layer, r, c, D, g, H, x, dx, sure and must_accept)
        if must_accept or step + 1 >= DET_STEPS or ax.max() > 1e6:
            return
        # the move: each coordinate to round(x), or to either neighbour where x is within dx of a half-integer
        # (a coordinate that stays while another moves is round(x) = 0 like any other)
        options = []
        for v in x:
            options.append(sorted({int(np.rint(v - dx)), int(np.rint(v)), int(np.rint(v + dx))}))
        n_opt = len(options[0]) * len(options[1]) * len(options[2])
        for mc in options[0]:
            for mr in options[1]:
                for ml in options[2]:
                    if (mc, mr, ml) == (0, 0, 0):
                        continue   # no move is the acceptance, followed above
                    if self._inside(layer + ml, r + mr, c + mc):
                        self._refine(octave, layer + ml, r + mr, c + mc, step + 1, sure and not may_accept and n_opt == 1)

    def _tests(self, octave, layer, r, c, D, g, H, x, dx, sure):
        e = DET_E
        contr = abs(D + 0.5 * float(g @ x)) * N_LAYERS
        dcontr = (e + 1.5 * (0.5 * e + float(np.abs(g).max()) * dx)) * N_LAYERS
        dxx, dyy, dxy = H[0, 0], H[1, 1], H[0, 1]
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        ddet = 4.0 * e * (abs(dxx) + abs(dyy)) + 2.0 * e * abs(dxy)
        f = (self.edge + 1.0) ** 2 * det - self.edge * tr * tr
        df = (self.edge + 1.0) ** 2 * ddet + 2.0 * self.edge * abs(tr) * 8.0 * e
        margins = (contr - self.contrast, dcontr), (det, ddet), (f, df)
        if any(m <= -d for m, d in margins):
            return
        cell = (octave, layer, r, c)
        if sure and all(m > d for m, d in margins):
            self.present.add(cell)
        else:
            self.undecided.add(cell)


def keypoint_cells(kps):
    """The cell (octave, layer, row, column) of each returned keypoint: unpack's level position, rounded."""
    out = []
    for kp in kps:
        octave, layer, _, _, px, py, _ = unpack(kp)
        out.append((octave, layer, int(np.rint(py)), int(np.rint(px))))
    return out


def check_detection(img, kps, label, model=None, **perturb):
    """The detection anchor on one image's keypoints: every decided-present cell is the cell of a returned
    keypoint (else missing) and every returned keypoint's cell is decided present or undecided (else
    unexplained).  Prints and returns the counts; `bad` lists the violations, which the caller asserts empty
    (the negative controls assert the opposite)."""
    m = model if model is not None else DetectionModel(img, **perturb)
    cells = set(keypoint_cells(kps))
    missing = sorted(m.present - cells)
    unexplained = sorted(cells - m.present - m.undecided)
    und = len(cells & m.undecided)
    print(f"{label}: {len(kps)} keypoints in {len(cells)} cells, octaves -1 .. {m.octaves - 2} searched, {m.candidates} candidates; "
          f"{len(m.present)} decided present, {len(m.undecided)} undecided cells ({und} of them returned), "
          f"{len(missing)} missing, {len(unexplained)} unexplained")
    return dict(keypoints=len(kps), cells=len(cells), present=len(m.present), undecided=len(m.undecided), undecided_returned=und,
                missing=missing, unexplained=unexplained, bad=missing + unexplained)
