"""Float64 / long double reference of the undistortion model, written from OpenCV's documentation of
initUndistortRectifyMap, undistortPoints and getOptimalNewCameraMatrix and NOT from oracle/undistort.cpp
or undistort.hip, and the case table shared by test_undistort_anchors.py (oracle, CPU) and
test_gpu_undistort.py (device).

Forward model of a destination pixel (u, v), new matrix K' = (f'x, f'y, c'x, c'y), matrix K, no
rectification:
    x = (u - c'x) / f'x,  y = (v - c'y) / f'y,  r2 = x^2 + y^2
    x" = x (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
         + 2 p1 x y + p2 (r2 + 2 x^2) + s1 r2 + s2 r2^2
    y" = y (same ratio) + p1 (r2 + 2 y^2) + 2 p2 x y + s3 r2 + s4 r2^2
    source position = (x" fx + cx, y" fy + cy)
with the coefficient vector k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]."""
import numpy as np

LD = np.longdouble
NAMES = ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "s1", "s2", "s3", "s4")


def coefficients(dist):
    """The named coefficients of a vector of 0, 4, 5, 8 or 12 values; those it does not hold are 0."""
    d = [float(v) for v in np.asarray(dist, np.float64).ravel()]
    assert len(d) in (0, 4, 5, 8, 12)
    c = dict.fromkeys(NAMES, 0.0)
    c.update(zip(NAMES, d))
    return c


def distort(x, y, dist):
    """Normalised undistorted (x, y) -> normalised distorted (x", y"), in the arrays' own precision."""
    c = coefficients(dist)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    ratio = (1 + c["k1"] * r2 + c["k2"] * r4 + c["k3"] * r6) / (1 + c["k4"] * r2 + c["k5"] * r4 + c["k6"] * r6)
    xd = x * ratio + 2 * c["p1"] * x * y + c["p2"] * (r2 + 2 * x * x) + c["s1"] * r2 + c["s2"] * r4
    yd = y * ratio + c["p1"] * (r2 + 2 * y * y) + 2 * c["p2"] * x * y + c["s3"] * r2 + c["s4"] * r4
    return xd, yd


def model_map(K, dist, newK, w, h):
    """Source position (mx, my), float64 [h, w] each, of every destination pixel (long double inside)."""
    K = np.asarray(K, np.float64)
    P = K if newK is None else np.asarray(newK, np.float64)
    v, u = np.mgrid[0:h, 0:w]
    x = (u.astype(LD) - LD(P[0, 2])) / LD(P[0, 0])
    y = (v.astype(LD) - LD(P[1, 2])) / LD(P[1, 1])
    xd, yd = distort(x, y, dist)
    mx = xd * LD(K[0, 0]) + LD(K[0, 2])
    my = yd * LD(K[1, 1]) + LD(K[1, 2])
    return mx.astype(np.float64), my.astype(np.float64)


# ---- tap classes of a bilinear remap with a constant border, from the model alone -------------
def quantised(m):
    """The 1/32-pixel position nearest to the model's: (integer part, fraction in 1/32)."""
    q = np.rint(m * 32).astype(np.int64)
    return q >> 5, q & 31


def tap_classes(mx, my, w, h):
    """(inside, partial, outside) masks of the model's quantised positions: all four taps in the image,
    some, none; and the four partial sides (sx = -1, sx = w - 1, sy = -1, sy = h - 1)."""
    sx, _ = quantised(mx)
    sy, _ = quantised(my)
    inside = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    outside = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    partial = ~inside & ~outside
    sides = {"sx=-1": partial & (sx == -1), "sx=w-1": partial & (sx == w - 1),
             "sy=-1": partial & (sy == -1), "sy=h-1": partial & (sy == h - 1)}
    return inside, partial, outside, sides


MAP_BOUND = 1.0 / 64 + 1e-9  # half the 1/32 quantum + the double rounding of u * 32 and of a row's additions


def safely_inside(mx, my, w, h):
    """Pixels at which every map within MAP_BOUND of the model interpolates real pixels only."""
    return (mx - MAP_BOUND >= 0) & (mx + MAP_BOUND <= w - 1) & (my - MAP_BOUND >= 0) & (my + MAP_BOUND <= h - 1)


def safely_outside(mx, my, w, h):
    """Pixels at which every map within MAP_BOUND of the model has no tap in the image."""
    return (mx - MAP_BOUND >= w) | (mx + MAP_BOUND < -1) | (my - MAP_BOUND >= h) | (my + MAP_BOUND < -1)


def plane_image(w, h):
    """I(x, y) = 2x + 2y as uint8 (mod 256), and whether it is the plane itself (bilinear then exact)."""
    y, x = np.mgrid[0:h, 0:w]
    return ((2 * x + 2 * y) & 255).astype(np.uint8), 2 * (w - 1) + 2 * (h - 1) <= 255


def noise_image(w, h, seed=11):
    return np.random.default_rng(seed + w * 31 + h).integers(0, 256, (h, w), dtype=np.uint8)


# ---- inverse of the model and getOptimalNewCameraMatrix ---------------------------------------
def undistort_normalised(xd, yd, dist, steps=None):
    """Normalised distorted -> undistorted.  steps=None: Newton on the forward model from the zero-
    distortion solution until it stops moving (residual asserted); steps=k: k steps of the fixed-point
    iteration x <- (x" - tangential - prism) / ratio that undistortPoints documents (OpenCV runs 5)."""
    c = coefficients(dist)
    xd, yd = np.asarray(xd, LD), np.asarray(yd, LD)
    x, y = xd.copy(), yd.copy()
    if steps is not None:
        for _ in range(steps):
            r2 = x * x + y * y
            r4, r6 = r2 * r2, r2 * r2 * r2
            inv = (1 + c["k4"] * r2 + c["k5"] * r4 + c["k6"] * r6) / (1 + c["k1"] * r2 + c["k2"] * r4 + c["k3"] * r6)
            dx = 2 * c["p1"] * x * y + c["p2"] * (r2 + 2 * x * x) + c["s1"] * r2 + c["s2"] * r4
            dy = c["p1"] * (r2 + 2 * y * y) + 2 * c["p2"] * x * y + c["s3"] * r2 + c["s4"] * r4
            x, y = (xd - dx) * inv, (yd - dy) * inv
        return x, y
    for _ in range(100):
        r2 = x * x + y * y
        r4, r6 = r2 * r2, r2 * r2 * r2
        N = 1 + c["k1"] * r2 + c["k2"] * r4 + c["k3"] * r6
        D = 1 + c["k4"] * r2 + c["k5"] * r4 + c["k6"] * r6
        dN = c["k1"] + 2 * c["k2"] * r2 + 3 * c["k3"] * r4
        dD = c["k4"] + 2 * c["k5"] * r2 + 3 * c["k6"] * r4
        kr, dkr = N / D, (dN * D - N * dD) / (D * D)  # ratio and its derivative by r2
        fx, fy = distort(x, y, dist)
        jxx = kr + 2 * x * x * dkr + 2 * c["p1"] * y + 6 * c["p2"] * x + 2 * c["s1"] * x + 4 * c["s2"] * r2 * x
        jxy = 2 * x * y * dkr + 2 * c["p1"] * x + 2 * c["p2"] * y + 2 * c["s1"] * y + 4 * c["s2"] * r2 * y
        jyx = 2 * x * y * dkr + 2 * c["p1"] * x + 2 * c["p2"] * y + 2 * c["s3"] * x + 4 * c["s4"] * r2 * x
        jyy = kr + 2 * y * y * dkr + 6 * c["p1"] * y + 2 * c["p2"] * x + 2 * c["s3"] * y + 4 * c["s4"] * r2 * y
        ex, ey = fx - xd, fy - yd
        det = jxx * jyy - jxy * jyx
        sx, sy = (jyy * ex - jxy * ey) / det, (jxx * ey - jyx * ex) / det
        x, y = x - sx, y - sy
        if max(np.abs(sx).max(), np.abs(sy).max()) < 1e-17:
            break
    fx, fy = distort(x, y, dist)
    assert max(np.abs(fx - xd).max(), np.abs(fy - yd).max()) < 1e-15, "the inverse did not converge"
    return x, y


def grid_rectangles(K, dist, w, h, steps=None):
    """The 9 x 9 grid over [0, w] x [0, h], undistorted to normalised coordinates: the inner rectangle
    (inscribed: the largest left / top edge value, the smallest right / bottom one) and the outer one
    (bounding box), each (x0, x1, y0, y1) in long double."""
    K = np.asarray(K, np.float64)
    gy, gx = np.mgrid[0:9, 0:9]
    xd = (gx.astype(LD) * w / 8 - LD(K[0, 2])) / LD(K[0, 0])
    yd = (gy.astype(LD) * h / 8 - LD(K[1, 2])) / LD(K[1, 1])
    x, y = undistort_normalised(xd, yd, dist, steps)
    inner = (x[:, 0].max(), x[:, 8].min(), y[0, :].max(), y[8, :].min())
    outer = (x.min(), x.max(), y.min(), y.max())
    return inner, outer


def _matrix_of(rect, nw, nh):
    x0, x1, y0, y1 = rect
    fx, fy = (nw - 1) / (x1 - x0), (nh - 1) / (y1 - y0)
    return np.array([fx, fy, -fx * x0, -fy * y0], LD)


def optimal_new_camera_matrix(K, dist, w, h, alpha, steps=None):
    """(fx, fy, cx, cy) of getOptimalNewCameraMatrix(K, dist, (w, h), alpha) without centring: the
    matrix that maps the inner rectangle onto the image at alpha 0, the outer one at alpha 1, blended
    linearly between.  Returns it with the float32-storage bound of the same four entries: OpenCV keeps
    the 81 undistorted points and the rectangles as float32, so each rectangle edge e carries |e| 2^-24, the
    float32 width x1 - x0 another (x1 - x0) 2^-24 and the float32 quotient (n - 1) / (x1 - x0) a third
    rounding; a focal length is then off by at most
    f ((|x0| + |x1| + (x1 - x0)) / (x1 - x0) + 1) 2^-24 =: f E (first order), and a principal point
    -f x0 by |f x0| (E + 2^-24)."""
    eps = LD(2.0) ** -24
    out, bound = np.zeros(4, LD), np.zeros(4, LD)
    for rect, wgt in zip(grid_rectangles(K, dist, w, h, steps), (1 - LD(alpha), LD(alpha))):
        x0, x1, y0, y1 = rect
        m = _matrix_of(rect, w, h)
        ex = ((abs(x0) + abs(x1) + (x1 - x0)) / (x1 - x0) + 1) * eps
        ey = ((abs(y0) + abs(y1) + (y1 - y0)) / (y1 - y0) + 1) * eps
        b = np.array([m[0] * ex, m[1] * ey, abs(m[2]) * (ex + eps), abs(m[3]) * (ey + eps)], LD)
        out += wgt * m
        bound += wgt * b
    return out.astype(np.float64), bound.astype(np.float64)


# ---- the case table ----------------------------------------------------------------------------
def camera(w, h):
    return np.array([[0.95 * w, 0, 0.51 * w - 0.3], [0, 0.96 * w, 0.47 * h + 0.2], [0, 0, 1.0]])


ONE_HOT = {"k1": -0.3, "k2": 0.15, "p1": 0.02, "p2": -0.015, "k3": 0.1, "k4": 0.2, "k5": -0.1, "k6": 0.05,
           "s1": 0.01, "s2": -0.02, "s3": 0.015, "s4": 0.01}
STRONG_BARREL = (-0.45, 0.2, 0.01, -0.01, -0.03)
PINCUSHION = (0.4, 0.1, 0.0, 0.0, 0.0)
STRIPE_DIST = (-0.2, 0.05, 0.001, 0.001, 0.0)


def _one_hot(name):
    i = NAMES.index(name)
    d = np.zeros(5 if i < 5 else (8 if i < 8 else 12))
    d[i] = ONE_HOT[name]
    return d


def small_cases():
    """[(id, dist, (w, h), alpha)]: the cases both the oracle and the device run."""
    out = []
    for size in ((50, 38), (67, 45)):
        for name in NAMES:
            out.append((f"{name}-{size[0]}x{size[1]}", _one_hot(name), size, 1.0))
    out.append(("barrel-a0", np.array(STRONG_BARREL), (61, 47), 0.0))
    out.append(("barrel-a1", np.array(STRONG_BARREL), (61, 47), 1.0))
    out.append(("pincushion", np.array(PINCUSHION), (61, 47), 1.0))
    out.append(("stripes-4100x6", np.array(STRIPE_DIST), (4100, 6), 1.0))   # one row per stripe, 17 column blocks
    out.append(("stripes-5x70", np.array(STRIPE_DIST), (5, 70), 1.0))       # one stripe, many row blocks
    return out


SMALL_CASES = small_cases()

# The calibration rows of test_gpu_undistort.py (rosbot_calibration.yaml:22, camera_calibration.yaml:22, a
# rational model) with their matrices; the oracle runs them at full size on the CPU only.
K_SMALL = np.array([[606.811009, 0, 325.199941], [0, 611.104701, 227.591593], [0, 0, 1.0]])
K_LARGE = np.array([[1173.854081, 0, 747.788206], [0, 1170.565083, 574.700374], [0, 0, 1.0]])
CALIBRATION_CASES = [
    ("zero", np.zeros(5), (640, 480), K_SMALL),
    ("rosbot", np.array([0.142541, -0.248887, -0.005254, -0.005417, 0.0]), (640, 480), K_SMALL),
    ("camera", np.array([-0.296079, 0.099771, 0.000222, 0.000109, 0.0]), (1440, 1080), K_LARGE),
    ("rational", np.array([0.1, -0.2, 0.001, -0.002, 0.05, 0.01, -0.02, 0.003]), (1280, 720), K_LARGE),
]
