"""Float64 model of SURF's orientation assignment and 64-entry descriptor, written from Bay et al. (2008) and
the documented behaviour of OpenCV's SURF_create(extended=False, upright=False), NOT from oracle/surf.cpp or
surf.hip, and the check test_descriptor_anchors.py (oracle) and test_gpu_descriptor_anchors.py (device)
share.  The model takes the 8-bit image and the keypoint records only.  The last part of the module is the
fast Hessian (which keypoints exist), described where it begins.

Orientation.  s = size * 1.2 / 9; Haar wavelets of side g = 2 round(2 s): dx = mean of the right half minus
mean of the left half, dy = mean of the top half minus mean of the bottom half, from an exact integer integral
image, at the 113 offsets (i, j) with i^2 + j^2 <= 36 (OpenCV's test, which keeps the four axis points at
distance exactly 6), the box's corner at round(pt + (i, j) s - (g - 1) / 2), weighted by G[i + 6] G[j + 6], G the
13-tap Gaussian of sigma 2.5; boxes that leave the image are dropped.
Each sample's angle atan2(dy, dx) is rounded to a degree; for every window centre 0, 5, ..., 355 the samples
within (-30, 30) degrees are summed, the window with the largest |sum|^2 wins (the first, on equality) and
the direction is atan2(-sum_y, sum_x), in degrees, x right and y down.

Descriptor, for the keypoint's own stored angle t.  n = int(21 s); window pixel (i, j), u = j - (n - 1) / 2,
v = i - (n - 1) / 2, samples the image at (x + u cos t - v sin t, y + u sin t + v cos t): bilinear where the floor of
the position has a right and a lower neighbour, else the nearest pixel clamped; rounded to 8 bits.  The
positions are formed with OpenCV's types (window()): the angle in radians, cos, sin, the first sample and the
step from row to row in float32, the steps along a row in double.  A float64 position would differ from that
by up to 1e-4 px at the last rows, which on noise makes every tenth window pixel uncertain.  The window is area-averaged to 21 x 21 (output
k covers [k n / 21, (k + 1) n / 21) on each axis) and rounded to 8 bits: the patch P.  DX[i][j] = (P[i][j+1] -
P[i][j] + P[i+1][j+1] - P[i+1][j]) W[i] W[j] and DY[i][j] = (P[i+1][j] - P[i][j] + P[i+1][j+1] - P[i][j+1]) W[i] W[j],
W the 20-tap Gaussian of sigma 3.3; entry 4 (4 a + b) + (0, 1, 2, 3) is the sum of (DX, DY, |DX|, |DY|) over
rows 5 a .. 5 a + 4 and columns 5 b .. 5 b + 4; the 64 entries are scaled to unit norm.

Uncertain pixels and the per-entry bound.  The two roundings to 8 bits are discontinuities, so the model
says which of its pixels a float32 implementation may round the other way, and what that can do.  With
U = 2^-24:
  position  formed as the implementation forms it, so what is left is the last place of cos and sin and of
            the products with (n - 1) / 2, carried over the steps, and the float32 fraction:
            DP = ((n - 1) + i + j) U + U / 2.
  window    bilinear: |dw| <= GX DP + GY DP + R, GX and GY the largest horizontal and vertical
            differences of neighbouring pixels in the 3 x 3 cells around the sample, qmax the largest of its
            four pixels, and R = U (7 t0 + 6 t1 + 5 t2 + 3 t3) for the roundings of the float32 expression
            t0 + t1 + t2 + t3 = q0 (1 - a) (1 - b) + q1 a (1 - b) + q2 (1 - a) b + q3 a b summed left to right: 1 - a,
            1 - b and the two products of t0 (4), three of t1 and t2, two of t3, and the sums t0 + t1,
            + t2, + t3 (one rounding of each partial sum).  A pixel whose value before rounding
            is within |dw| of a half-integer may round to the other neighbour: it may go up by 1 or down
            by 1, whichever the model did not choose.  A clamped sample, or one within DP of where the
            two regimes meet, whose position is within DP of a half-integer (or of the meeting line) may
            take a neighbouring pixel: up or down by max(GX, GY).
  patch     the area average A has weights a >= 0 that sum to 1, so the float32 one lies in
            [A - sum a down - E_A, A + sum a up + E_A].  Every term and partial sum of the float32 average is
            non-negative and at most the result, so each rounding is relative to it: a term meets its two
            weights (2 roundings each), two products and at most ceil(n / 21) additions per axis, and
            E_A = (2 (ceil(n / 21) + 2) + 4) U (A + sum a up).  A patch pixel is uncertain when that interval holds a half-integer
            (an end point counts), and may then take any 8-bit value the interval rounds to.  At n = 42
            the average of 2 x 2 8-bit values is taken in integers, (a + b + c + d + 2) >> 2: E_A = 0 and
            a half rounds up.
  entries   P[r][c] enters DX[i][j] and DY[i][j] for i in {r - 1, r}, j in {c - 1, c} with coefficient +-1, so
            a change of P[r][c] by at most m moves each of the four sums of cell (a, b) by at most
            m * sum of W[i] W[j] over those (i, j) that lie in the cell (||x + d| - |x|| <= |d| covers the
            absolute sums).  Summed over the uncertain pixels this is dV[e]; with V the model's unnormalised
            vector and D = |dV|_2, the unit vector moves by at most (dV[e] + |d[e]| D) / (|V|_2 - D)
            (from d' - d = dV / |V'| + V (1 / |V'| - 1 / |V|) and |V'| >= |V| - D), to which F32 is added.
  F32       with no uncertain pixel: W[i] W[j] carries <= 8 roundings, a sum of 25 terms <= 25, each relative
            to the cell's absolute sum <= |V|_2; the norm, its reciprocal and the product 4 more; doubled
            for the propagation through the norm: F32 = 80 U = 4.8e-6.
No number above is fitted to results.

Not from a paper or the documentation: the float32 / double mix of the window positions, the half-up integer
average at n = 42, the <= in the orientation offsets and the first-of-equal-maxima rule are OpenCV's source,
which the oracle restates too.  Their effect is at most 1e-4 px or one rounding tie, so no structural error
(an axis, a sign, an order, a weight) can hide behind them; but in these details the model is not independent."""
import math

import numpy as np

U = 2.0 ** -24
F32 = 80 * U
ORI_TOL_DEG = 0.3            # fastAtan2's documented accuracy
ORI_EXCLUDED_MAX = 0.02
DESC_BOUND_MAX = 0.02        # a keypoint whose derived bound exceeds this in any entry is excluded
DESC_EXCLUDED_MAX = 0.10
# Two windows whose |sum|^2 agree to this relative amount cannot be told apart by float32 sums of up to 113
# terms (each sum within 113 U of its terms' absolute sum, the square twice that, doubled as a margin): a
# centred symmetric blob makes eight windows exactly equal, and the direction of any of them is accepted.
WINDOW_TIE = 4 * 113 * U


def gaussian(n, sigma):
    x = np.arange(n) - (n - 1) / 2.0
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    return k / k.sum()


G_ORI, G_DESC = gaussian(13, 2.5), gaussian(20, 3.3)
ORI_SAMPLES = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36]
assert len(ORI_SAMPLES) == 113


def integral(img):
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    s[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return s


def _box(S, x0, y0, x1, y1):
    return S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]


def orientation(S, kp):
    """Three lists of directions in degrees, for the samples within 0.3 degrees of a half-degree rounded to the
    nearest degree, down and up: the direction of the first largest window, then those of the other windows
    within WINDOW_TIE of it."""
    s = float(kp["size"]) * 1.2 / 9.0
    g = 2 * int(np.rint(2.0 * s))
    rows, cols = S.shape
    X, Y = [], []
    for i, j in ORI_SAMPLES:
        x = int(np.rint(float(kp["x"]) + i * s - (g - 1) / 2.0))
        y = int(np.rint(float(kp["y"]) + j * s - (g - 1) / 2.0))
        if y < 0 or y >= rows - g or x < 0 or x >= cols - g:
            continue
        wgt = G_ORI[i + 6] * G_ORI[j + 6] / (g * g / 2.0)
        X.append(wgt * (_box(S, x + g // 2, y, x + g, y + g) - _box(S, x, y, x + g // 2, y + g)))
        Y.append(wgt * (_box(S, x, y, x + g, y + g // 2) - _box(S, x, y + g // 2, x + g, y + g)))
    X, Y = np.array(X, np.float64), np.array(Y, np.float64)
    assert len(X) > 0
    ang = np.degrees(np.arctan2(Y, X)) % 360.0
    lo = np.floor(ang)
    tie = np.abs(ang - lo - 0.5) < ORI_TOL_DEG
    centres = np.arange(0, 360, 5)
    out = []
    for deg in (np.rint(ang), np.where(tie, lo, np.rint(ang)), np.where(tie, lo + 1, np.rint(ang))):
        d = np.abs(deg[None, :] - centres[:, None])
        inside = (d < 30) | (d > 330)
        sx, sy = inside @ X, inside @ Y
        mod = sx * sx + sy * sy
        k = int(np.argmax(mod))   # the first of equal maxima
        near = [c for c in np.flatnonzero(mod >= mod[k] * (1 - WINDOW_TIE)) if c != k]
        out.append([math.degrees(math.atan2(-sy[c], sx[c])) % 360.0 for c in [k] + near])
    return out


def _maxpool3(a):
    p = np.pad(a, 1, mode="edge")
    return np.max([p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3)], axis=0)


def window(img, kp):
    """(n x n window values before rounding, amount each may go down, up, when rounded to 8 bits)."""
    h, w = img.shape
    I = img.astype(np.float64)
    s = float(kp["size"]) * 1.2 / 9.0
    n = int(21 * s)
    # positions with OpenCV's types: float32 angle, cos, sin, first position and row steps, double columns
    f32 = np.float32
    t = f32(kp["angle"]) * f32(math.pi / 180.0)
    sin_dir, cos_dir = -f32(math.sin(float(t))), f32(math.cos(float(t)))
    off = -f32(n - 1) / f32(2)
    sx, sy = np.empty(n, f32), np.empty(n, f32)
    sx[0] = f32(kp["x"]) + off * cos_dir + off * sin_dir
    sy[0] = f32(kp["y"]) - off * sin_dir + off * cos_dir
    for r in range(1, n):
        sx[r], sy[r] = sx[r - 1] + sin_dir, sy[r - 1] + cos_dir
    i, j = np.mgrid[0:n, 0:n]
    px = sx.astype(np.float64)[:, None] + j * float(cos_dir)
    py = sy.astype(np.float64)[:, None] - j * float(sin_dir)
    dpx = dpy = ((n - 1) + i + j) * U + U / 2
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inside = (ix >= 0) & (ix < w - 1) & (iy >= 0) & (iy < h - 1)
    # the largest neighbour differences in the 3 x 3 cells around each pixel
    gx = np.zeros((h, w))
    gx[:, :-1] = np.abs(I[:, 1:] - I[:, :-1])
    gy = np.zeros((h, w))
    gy[:-1, :] = np.abs(I[1:, :] - I[:-1, :])
    gx, gy = _maxpool3(_maxpool3(gx)), _maxpool3(_maxpool3(gy))
    jx, jy = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    a, b = px - ix, py - iy
    q = [I[jy, jx], I[jy, jx + 1], I[jy + 1, jx], I[jy + 1, jx + 1]]
    bil = q[0] * (1 - a) * (1 - b) + q[1] * a * (1 - b) + q[2] * (1 - a) * b + q[3] * a * b
    rx, ry = np.clip(np.rint(px), 0, w - 1).astype(np.int64), np.clip(np.rint(py), 0, h - 1).astype(np.int64)
    val = np.where(inside, bil, I[ry, rx])
    t0, t1, t2, t3 = q[0] * (1 - a) * (1 - b), q[1] * a * (1 - b), q[2] * (1 - a) * b, q[3] * a * b
    dw = gx[jy, jx] * dpx + gy[jy, jx] * dpy + U * (7 * t0 + 6 * t1 + 5 * t2 + 3 * t3)
    frac = val - np.floor(val)
    near = inside & (np.abs(frac - 0.5) <= dw)
    rounded_up = np.rint(val) > np.floor(val)
    down = np.where(near & rounded_up, 1.0, 0.0)
    up = np.where(near & ~rounded_up, 1.0, 0.0)
    # the regimes' meeting lines and, in the clamped regime, the half-integer positions
    edge = (np.minimum(np.abs(px), np.abs(px - (w - 1))) <= dpx) | (np.minimum(np.abs(py), np.abs(py - (h - 1))) <= dpy)
    half = ~inside & ((np.abs(px - np.floor(px) - 0.5) <= dpx) | (np.abs(py - np.floor(py) - 0.5) <= dpy))
    jump = np.where(edge | half, gx[ry, rx] + gy[ry, rx], 0.0)
    return val, np.maximum(down, jump), np.maximum(up, jump)


def area_weights(n, m=21):
    """[m, n]: the share of input cell c in output cell k, exact area average."""
    sc = n / m
    k, c = np.arange(m)[:, None], np.arange(n)[None, :]
    return np.clip(np.minimum(c + 1, (k + 1) * sc) - np.maximum(c, k * sc), 0.0, None) / sc


def descriptor(img, kp):
    """(d float64[64], bound float64[64], uncertain patch pixels)."""
    val, down, up = window(img, kp)
    n = val.shape[0]
    assert n >= 21, n   # below, INTER_AREA would enlarge
    A = area_weights(n)
    W = np.rint(val)
    avg = A @ W @ A.T
    lo, hi = avg - A @ down @ A.T, avg + A @ up @ A.T
    if n == 42:   # the 2 x 2 average of 8-bit values is taken in integers, (a + b + c + d + 2) >> 2: half up, exact
        P, p_lo, p_hi = np.floor(avg + 0.5), np.floor(lo + 0.5), np.floor(hi + 0.5)
    else:         # float32 accumulation, rounded half to even: the 8-bit values the widened interval rounds to
        e_a = (2 * (math.ceil(n / 21) + 2) + 4) * U * hi
        P, p_lo, p_hi = np.rint(avg), np.ceil(lo - e_a - 0.5), np.floor(hi + e_a + 0.5)
    move = np.maximum(P - p_lo, p_hi - P)
    assert (move >= 0).all()
    dw = np.outer(G_DESC, G_DESC)
    DX = (P[:-1, 1:] - P[:-1, :-1] + P[1:, 1:] - P[1:, :-1]) * dw
    DY = (P[1:, :-1] - P[:-1, :-1] + P[1:, 1:] - P[:-1, 1:]) * dw
    V = np.zeros((4, 4, 4))
    dV = np.zeros((4, 4))
    for a in range(4):
        for b in range(4):
            cx, cy = DX[5 * a:5 * a + 5, 5 * b:5 * b + 5], DY[5 * a:5 * a + 5, 5 * b:5 * b + 5]
            V[a, b] = cx.sum(), cy.sum(), np.abs(cx).sum(), np.abs(cy).sum()
    for r, c in np.argwhere(move > 0):
        for i in (r - 1, r):
            for j in (c - 1, c):
                if 0 <= i < 20 and 0 <= j < 20:
                    dV[i // 5, j // 5] += move[r, c] * dw[i, j]
    V, dV = V.reshape(64), np.repeat(dV.reshape(16), 4)
    norm, D = math.sqrt(float((V * V).sum())), math.sqrt(float((dV * dV).sum()))
    d = V / norm
    bound = np.full(64, np.inf) if D >= norm else (dV + np.abs(d) * D) / (norm - D)
    return d, bound + F32, int((move > 0).sum())


def check_features(img, kps, desc, label, smooth=False, max_keypoints=None):
    """The SURF anchors on one image's features; prints what it measured and returns the figures.

    Orientation: |kp.angle - model| <= 0.3 degrees, the model being the direction of the first largest window
    with sample angles rounded to the nearest degree, or of a window within WINDOW_TIE of it (counted and
    printed: other_window).  A keypoint that misses that is left out of this comparison only when the
    direction of the winning window under one of the other two roundings (samples within 0.3 degrees of a
    half-degree all down, all up) is within 0.3 degrees of its angle, which shows that such a sample decides
    between two windows; it is counted as excluded, at most 2 % of the keypoints checked, none when smooth.
    An angle that fits no rounding's window fails.
    Descriptor, against the model for the keypoint's own angle: |d - model| <= the derived per-entry bound (F32
    where the keypoint has no uncertain patch pixel).  A keypoint whose bound exceeds 0.02 in any entry is
    excluded, at most 10 % of the keypoints checked; when smooth, every keypoint has no uncertain pixel."""
    n = len(kps)
    assert n > 0 and desc.shape == (n, 64), (label, n, desc.shape)
    S = integral(img)
    chosen = np.arange(n) if not max_keypoints or n <= max_keypoints else np.arange(max_keypoints) * n // max_keypoints
    ori_err, ori_excluded, other_window, clean, clean_err, unc_ratio, unc_err, desc_excluded, bad = 0.0, 0, 0, 0, 0.0, 0.0, 0.0, 0, []
    for i in chosen:
        kp = kps[i]
        variants = orientation(S, kp)
        errs = [[abs((float(kp["angle"]) - a + 180.0) % 360.0 - 180.0) for a in v] for v in variants]
        err = min(errs[0])
        if err <= ORI_TOL_DEG:
            ori_err = max(ori_err, err)
            other_window += errs[0][0] > ORI_TOL_DEG
        elif min(min(e) for e in errs[1:]) <= ORI_TOL_DEG:
            ori_excluded += 1
        else:
            bad.append(("angle", int(i), float(kp["angle"]), variants))
        d, bound, uncertain = descriptor(img, kp)
        err = np.abs(desc[i].astype(np.float64) - d)
        if uncertain == 0:
            clean += 1
            clean_err = max(clean_err, float(err.max()))
        elif bound.max() > DESC_BOUND_MAX:
            desc_excluded += 1
            continue
        else:
            unc_err = max(unc_err, float(err.max()))
            unc_ratio = max(unc_ratio, float((err / bound).max()))
        if (err > bound).any():
            bad.append(("descriptor", int(i), int((err / bound).argmax()), float(err.max()), float(bound.max()), uncertain))
    m = len(chosen)
    print(f"{label}: {m} of {n} keypoints; angle error max {ori_err:.4f} deg, {other_window} by a window tied with the first largest, {ori_excluded} excluded; descriptor: {clean} "
          f"keypoints without uncertain pixels, error max {clean_err:.2e} (bound {F32:.1e}); {m - clean - desc_excluded} "
          f"with, error max {unc_err:.2e}, at most {unc_ratio:.3f} of the derived bound; {desc_excluded} excluded")
    assert not bad, (label, len(bad), bad[:6])
    assert ori_excluded <= ORI_EXCLUDED_MAX * m and desc_excluded <= DESC_EXCLUDED_MAX * m, (label, ori_excluded, desc_excluded, m)
    if smooth:
        assert ori_excluded == 0 and clean == m, (label, ori_excluded, clean, m)
    return dict(checked=m, ori_err=ori_err, ori_excluded=ori_excluded, other_window=other_window, clean=clean, clean_err=clean_err,
                unc_err=unc_err, desc_excluded=desc_excluded)


# ---------------------------------------------------------------------------------------------------------------
# Detection: the fast Hessian of Bay et al. (2008) section 3 with the documented defaults of SURF_create
# (nOctaves 4, nOctaveLayers 3): which keypoints exist, where, with what size, sign and response.
#
#   layout     octave o has five layers of size (9 + 6 layer) 2^o sampled every 2^o pixels; a window of that size
#              with its corner at (j, i) 2^o is sample (i + m, j + m) of the layer, m = (size / 2) / 2^o in
#              integers, so that the samples of an octave's layers with equal index are (nearly) concentric.
#              A layer larger than the image has no samples.
#   filters    the 9 x 9 masks of the paper's figure (corner coordinates x0, y0, x1, y1, weight):
#                Dxx (0, 2, 3, 7, 1) (3, 2, 6, 7, -2) (6, 2, 9, 7, 1), Dyy its transpose,
#                Dxy (1, 1, 4, 4, 1) (5, 1, 8, 4, -1) (1, 5, 4, 8, -1) (5, 5, 8, 8, 1),
#              each coordinate c scaled to round(c size / 9).  No product c size / 9 is a half-integer:
#              2 size c = 9 (2 k + 1) would have an even left and an odd right side, so the rounding mode cannot
#              matter.  Each lobe is the box sum (exact, from the integer integral image) times weight / area.
#              det = Dxx Dyy - 0.81 Dxy^2, trace = Dxx + Dyy.
#   maxima     in the three middle layers: a sample above the threshold and strictly above its 26 neighbours,
#              at least (size of the next layer / 2) / 2^o + 1 samples from every side of the layer's grid of
#              (rows / 2^o) x (columns / 2^o).
#   keypoint   x = -A^-1 b from the central differences of det over (sample column, sample row, layer); kept
#              when x != 0 and every |x| <= 1; centre = window corner + (size - 1) / 2 + x 2^o, size = round(size +
#              x[2] (size - size of the layer below)), class_id = sign of the trace, response = det, octave = o.
#
# Float32 bound of det, counted.  Box sums are exact integers below 2^24 (255 * 176 * 160 < 2^23 for every
# image used; asserted).  With U = 2^-24 and A = sum over lobes of |weight / area * box sum|: a lobe's weight is
# one rounding, its product one, and the (lobes - 1) additions one each of a partial sum that is at most A, so
# |dDxx| <= 4 U Axx, |dDyy| <= 4 U Ayy, |dDxy| <= 5 U Axy.  Then
#   d(det) <= |Dyy| dDxx + |Dxx| dDyy + U |Dxx Dyy|            (the product)
#           + 0.81 (2 |Dxy| dDxy + 3 U Dxy^2)                    (0.81 itself and two products)
#           + U (|Dxx Dyy| + 0.81 Dxy^2)                         (the subtraction),
# and d(trace) <= dDxx + dDyy + U |trace|.  An implementation that accumulates in double or fuses a
# multiply-add makes fewer roundings, none more.
# Interpolation, to first order as sift_reference.check_refinement: with E the largest d(det) of the 27
# samples, b carries E per entry and A at most 4 E per entry (row sums 6 E); a float32 LU solve is backward
# stable with a perturbation of at most 12 U |A|_inf in A's row sums and 2 U |b|_inf in b (3 x 3, partial
# pivoting), so |dx| <= |A^-1|_inf ((E + 2 U |b|_inf) + (6 E + 12 U |A|_inf) max(|x|_inf, 1)).
# A comparison whose margin exceeds its error is decided.  A model keypoint is DECIDED when the threshold, all
# 26 neighbour comparisons, the three |x| <= 1, the rounding of the size and the sign of the trace are; a
# possible maximum that no decided comparison rejects is UNDECIDED.
#
# Not from the paper or the documentation: the masks' integer scaling, the margins, x != 0 and the form of
# the size interpolation are OpenCV's source, which the oracle restates too.  The negative controls of
# test_detection_anchors.py show that each of them is observable.
HESSIAN_OCTAVES, HESSIAN_LAYERS = 4, 5
DXX = ((0, 2, 3, 7, 1.0), (3, 2, 6, 7, -2.0), (6, 2, 9, 7, 1.0))
DYY = tuple((y0, x0, y1, x1, wt) for x0, y0, x1, y1, wt in DXX)
DXY = ((1, 1, 4, 4, 1.0), (5, 1, 8, 4, -1.0), (1, 5, 4, 8, -1.0), (5, 5, 8, 8, 1.0))


class FastHessian:
    """keypoints: list of dicts (octave, x, y, size, class_id, response and the bounds dresp, dpos; cx, cy the
    sample's own centre; decided).  The keyword arguments are what the negative controls perturb."""

    def __init__(self, img, threshold, weight=0.81, floor_lobes=False, margin_extra=1, layers=HESSIAN_LAYERS,
                 trace_sign=1, accept=1.0):
        self.S = integral(img)
        self.h, self.w = img.shape
        assert 255 * self.h * self.w < 2 ** 24
        self.weight, self.floor_lobes, self.accept, self.trace_sign = weight, floor_lobes, accept, trace_sign
        self.keypoints, self.layers_skipped, self.maxima = [], 0, 0
        for octave in range(HESSIAN_OCTAVES):
            step = 2 ** octave
            sizes = [(9 + 6 * l) * step for l in range(layers)]
            resp = [self._layer(s, step) for s in sizes]
            self.layers_skipped += sum(r is None for r in resp)
            for l in range(1, layers - 1):
                self._maxima(octave, step, sizes, resp, l, threshold, margin_extra)

    def _pattern(self, mask, size, step, ni, nj):
        val, mag = np.zeros((ni, nj)), np.zeros((ni, nj))
        ys, xs = np.arange(ni)[:, None] * step, np.arange(nj)[None, :] * step
        for x0, y0, x1, y1, wt in mask:
            if self.floor_lobes:
                x0, y0, x1, y1 = (c * size // 9 for c in (x0, y0, x1, y1))
            else:
                assert all((2 * c * size) % 9 != 0 or (2 * c * size // 9) % 2 == 0 for c in (x0, y0, x1, y1))
                x0, y0, x1, y1 = (int(np.rint(c * size / 9.0)) for c in (x0, y0, x1, y1))
            box = (self.S[ys + y1, xs + x1] - self.S[ys + y0, xs + x1] - self.S[ys + y1, xs + x0] + self.S[ys + y0, xs + x0])
            t = box * (wt / ((x1 - x0) * (y1 - y0)))
            val += t
            mag += np.abs(t)
        return val, mag

    def _layer(self, size, step):
        """(det, d(det), trace, d(trace)) on the octave's grid, NaN where the layer has no sample."""
        if size > self.h or size > self.w:
            return None
        ni, nj = 1 + (self.h - size) // step, 1 + (self.w - size) // step
        dxx, axx = self._pattern(DXX, size, step, ni, nj)
        dyy, ayy = self._pattern(DYY, size, step, ni, nj)
        dxy, axy = self._pattern(DXY, size, step, ni, nj)
        k = self.weight
        det, tr = dxx * dyy - k * dxy * dxy, dxx + dyy
        ddxx, ddyy, ddxy = 4 * U * axx, 4 * U * ayy, 5 * U * axy
        ddet = (np.abs(dyy) * ddxx + np.abs(dxx) * ddyy + U * np.abs(dxx * dyy) + k * (2 * np.abs(dxy) * ddxy + 3 * U * dxy * dxy)
                + U * (np.abs(dxx * dyy) + k * dxy * dxy))
        dtr = ddxx + ddyy + U * np.abs(tr)
        m = (size // 2) // step
        out = []
        for a in (det, ddet, tr, dtr):
            g = np.full((self.h // step, self.w // step), np.nan)
            g[m:m + ni, m:m + nj] = a
            out.append(g)
        return out

    def _maxima(self, octave, step, sizes, resp, l, threshold, margin_extra):
        if resp[l + 1] is None:
            return  # its margin exceeds half the grid: nothing to search
        size = sizes[l]
        rows, cols = self.h // step, self.w // step
        margin = (sizes[l + 1] // 2) // step + margin_extra
        if rows - 2 * margin <= 0 or cols - 2 * margin <= 0:
            return
        sl = (slice(margin, rows - margin), slice(margin, cols - margin))
        v, dv = resp[l][0][sl], resp[l][1][sl]
        possible, certain = v > threshold - dv, v > threshold + dv
        for dl in (-1, 0, 1):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (dl, di, dj) == (0, 0, 0):
                        continue
                    s2 = (slice(margin + di, rows - margin + di), slice(margin + dj, cols - margin + dj))
                    n, dn = resp[l + dl][0][s2], resp[l + dl][1][s2]
                    if margin_extra == 1:
                        assert not np.isnan(n).any(), (octave, l, "a neighbour outside its layer")
                    else:   # the control without the + 1 reads where the next layer has no sample: taken as 0
                        n, dn = np.nan_to_num(n), np.nan_to_num(dn)
                    possible &= v > n - (dv + dn)
                    certain &= v > n + (dv + dn)
        m0 = (size // 2) // step
        for i, j in np.argwhere(possible):
            sure = bool(certain[i, j])
            i, j = int(i) + margin, int(j) + margin
            self.maxima += 1
            N = np.nan_to_num(np.stack([resp[l + dl][0][i - 1:i + 2, j - 1:j + 2] for dl in (-1, 0, 1)]))
            E = float(max(np.nan_to_num(resp[l + dl][1][i - 1:i + 2, j - 1:j + 2]).max() for dl in (-1, 0, 1)))
            b = -np.array([(N[1, 1, 2] - N[1, 1, 0]) / 2, (N[1, 2, 1] - N[1, 0, 1]) / 2, (N[2, 1, 1] - N[0, 1, 1]) / 2])
            c2 = 2 * N[1, 1, 1]
            dxy = (N[1, 2, 2] - N[1, 2, 0] - N[1, 0, 2] + N[1, 0, 0]) / 4
            dxs = (N[2, 1, 2] - N[2, 1, 0] - N[0, 1, 2] + N[0, 1, 0]) / 4
            dys = (N[2, 2, 1] - N[2, 0, 1] - N[0, 2, 1] + N[0, 0, 1]) / 4
            A = np.array([[N[1, 1, 0] + N[1, 1, 2] - c2, dxy, dxs], [dxy, N[1, 0, 1] + N[1, 2, 1] - c2, dys],
                          [dxs, dys, N[0, 1, 1] + N[2, 1, 1] - c2]])
            try:
                Ai = np.linalg.inv(A)
                x = Ai @ b
                a_inf = float(np.abs(A).sum(axis=1).max())
                dx = float(np.abs(Ai).sum(axis=1).max()) * ((E + 2 * U * float(np.abs(b).max())) +
                                                           (6 * E + 12 * U * a_inf) * max(float(np.abs(x).max()), 1.0))
            except np.linalg.LinAlgError:
                x, dx = np.zeros(3), np.inf
            if not np.isfinite(x).all() or not np.isfinite(dx):
                x, dx = np.zeros(3), np.inf
            ax = np.abs(x)
            if (ax > self.accept + dx).any():
                continue  # decided absent
            sure = sure and bool((ax < self.accept - dx).all())
            ds = size - sizes[l - 1]
            fsize = size + x[2] * ds
            sure = sure and abs(fsize - math.floor(fsize) - 0.5) > dx * ds
            tr, dtr = resp[l][2][i, j], resp[l][3][i, j]
            sure = sure and abs(tr) > dtr
            cx, cy = step * (j - m0) + (size - 1) / 2.0, step * (i - m0) + (size - 1) / 2.0
            px, py = cx + x[0] * step, cy + x[1] * step
            self.keypoints.append(dict(octave=octave, layer=l, x=px, y=py, cx=cx, cy=cy, step=step, size=int(np.rint(fsize)),
                                       class_id=self.trace_sign * (1 if tr > 0 else -1), response=float(N[1, 1, 1]),
                                       dresp=float(resp[l][1][i, j]), dpos=dx * step + 2.0 ** -22 * max(px, py, 1.0), decided=sure))


def check_detection(img, kps, threshold, label, **perturb):
    """The detection anchor on one image's keypoints.  A returned keypoint matches a model keypoint when the
    octaves are equal, the response lies within d(det) (and one float32 place) and the position within |dx| 2^o
    per axis; for an undecided model keypoint, whose |dx| may be anything, within (1 + accept) 2^o of the sample's
    own centre.  Every decided model keypoint has a match of equal size and class_id (else missing); every
    returned keypoint matches a model keypoint (else unexplained).  Prints and returns the counts; `bad`
    lists the violations."""
    m = FastHessian(img, threshold, **perturb)
    decided = [k for k in m.keypoints if k["decided"]]
    rx, ry, rr = kps["x"].astype(np.float64), kps["y"].astype(np.float64), kps["response"].astype(np.float64)
    explained = np.zeros(len(kps), bool)
    by_undecided = np.zeros(len(kps), bool)
    missing, worst_pos, worst_resp = [], 0.0, 0.0
    for k in m.keypoints:
        near = (kps["octave"] == k["octave"]) & (np.abs(rr - k["response"]) <= k["dresp"] + 2.0 ** -23 * abs(k["response"]))
        if k["decided"]:
            near &= (np.abs(rx - k["x"]) <= k["dpos"]) & (np.abs(ry - k["y"]) <= k["dpos"])
            full = near & (kps["size"] == k["size"]) & (kps["class_id"] == k["class_id"])
            if not full.any():
                missing.append((k["octave"], k["layer"], round(k["x"], 3), round(k["y"], 3), k["size"], k["class_id"], k["response"]))
            for i in np.flatnonzero(full):
                worst_pos = max(worst_pos, max(abs(rx[i] - k["x"]), abs(ry[i] - k["y"])) / k["dpos"])
                worst_resp = max(worst_resp, abs(rr[i] - k["response"]) / (k["dresp"] + 2.0 ** -23 * abs(k["response"])))
            explained |= full
        else:
            reach = (1.0 + perturb.get("accept", 1.0)) * k["step"] + min(k["dpos"], k["step"])
            near &= (np.abs(rx - k["cx"]) <= reach) & (np.abs(ry - k["cy"]) <= reach)
            by_undecided |= near
    by_undecided &= ~explained
    unexplained = [(int(k["octave"]), float(k["x"]), float(k["y"]), float(k["size"]), int(k["class_id"]), float(k["response"]))
                   for k in kps[~explained & ~by_undecided]]
    print(f"{label} threshold {threshold:g}: {len(kps)} keypoints, {m.layers_skipped} layers larger than the image, {m.maxima} possible "
          f"maxima; {len(decided)} decided, {len(m.keypoints) - len(decided)} undecided ({int(by_undecided.sum())} keypoints held to those), "
          f"{len(missing)} missing, {len(unexplained)} unexplained; position error / bound {worst_pos:.3f}, response error / bound {worst_resp:.3f}")
    return dict(keypoints=len(kps), decided=len(decided), undecided=len(m.keypoints) - len(decided), by_undecided=int(by_undecided.sum()),
                layers_skipped=m.layers_skipped, missing=missing, unexplained=unexplained, bad=missing + unexplained,
                worst_pos=worst_pos, worst_resp=worst_resp)
