"""Case builders shared by the geometry-parameter and pair-status tests
(test_geometry_cases.py checks on the CPU oracle that every builder reaches the
regime it is named for; test_gpu_geometry_params.py and test_gpu_stream_status.py
run the same cases on the device).  Plain functions, numpy only; the oracle
module is passed in where a builder needs it."""
import numpy as np

# fx != fy with an off-centre principal point, and a 1920x1080-like camera
K_SKEW = np.array([[300.0, 0, 160], [0, 310.0, 118], [0, 0, 1]])
K_HD = np.array([[1450.0, 0, 965.5], [0, 1435.0, 532.25], [0, 0, 1]])
CAMERAS = {"skew": K_SKEW, "hd": K_HD}

THRESHOLDS = (1e-3, 0.1, 0.5, 1.0, 3.0, 50.0)
PROBS = (0.5, 0.9, 0.999, 0.999999)
T_ZERO_THRESHOLD = 1e-25  # (threshold / f)^2 underflows to 0 in float: the score's fast_ok is false
M_SIZES = (6, 64, 65, 400, 1500)
MAX_ITERS = (1, 31, 32, 33, 1000)
DIST_THRESHOLDS = (0.5, 3.0, 50.0, 1e9)
POSE_M = (1, 127, 128, 129, 1000)
TRI_K = (1, 2, 255, 256, 257, 1000)

FLT_MIN = float(np.finfo(np.float32).tiny)


def score_threshold_f32(threshold, K):
    """t of the score kernel and of the oracle: (float)((threshold / ((fx + fy) / 2))^2)."""
    thr = threshold / ((K[0, 0] + K[1, 1]) / 2)
    return float(np.float32(thr * thr))


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    a = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * a + (1 - np.cos(angle)) * (a @ a)


def _px(X, K):
    """Pixel coordinates as the reference hands them over: float32 (KeyPoint_convert) widened."""
    p = X[:, :2] / X[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    return np.ascontiguousarray(p.astype(np.float32).astype(np.float64))


def correspondences(m, K, seed=0, outliers=1 / 3, noise=0.7):
    """m synthetic correspondences of one rigid motion: `outliers` of them uniform
    in the image, the rest with `noise` px of Gaussian noise."""
    rng = np.random.default_rng(1000 * seed + m)
    w, h = 2 * K[0, 2], 2 * K[1, 2]
    X = np.c_[rng.uniform(-1.5, 1.5, (m, 2)), rng.uniform(3, 8, m)]
    R = _rot([0.2, 1.0, 0.1], 0.06)
    t = np.array([0.4, 0.05, 0.1])
    p1 = _px(X, K) + rng.normal(0, noise, (m, 2))
    p2 = _px(X @ R.T + t, K) + rng.normal(0, noise, (m, 2))
    bad = rng.permutation(m)[: int(round(m * outliers))]
    p2[bad] = rng.uniform([0, 0], [w, h], (len(bad), 2))
    f32 = lambda p: np.ascontiguousarray(p.astype(np.float32).astype(np.float64))
    return f32(p1), f32(p2)


def param_grid():
    """(camera name, threshold, prob) of the findEssentialMat grid, the t = 0 case last per camera."""
    out = []
    for cam in CAMERAS:
        out += [(cam, th, pr) for th in THRESHOLDS for pr in PROBS]
        out.append((cam, T_ZERO_THRESHOLD, 0.999))
    return out


# ---- recoverPose scenes -----------------------------------------------------------------------
POSE_R = _rot([0.3, 1.0, -0.2], 0.35)
POSE_T = np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


POSE_E = skew(POSE_T) @ POSE_R
AXIS_E = skew(np.array([0.0, 0.0, 1.0]))  # R = I, t = (0, 0, 1): t has exact zero components


def decompositions(oracle, E):
    """decomposeEssentialMat as recoverPose calls it, on the oracle's Jacobi SVD:
    [(R1, t), (R2, t), (R1, -t), (R2, -t)] in recoverPose's order."""
    W, U, Vt = oracle.jacobi_svd(np.asarray(E, np.float64), full_u=True)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    Wm = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, 2].copy()
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def points_in_front(R, t, n, K, seed, zmin=0.7, zmax=20.0):
    """n correspondences whose points lie in front of both cameras of (R, t) (x2 = R x1 + t),
    at depths in (zmin, zmax) in both and within 80 degrees of both optical axes (a twisted
    pair's cameras face each other: its points lie between them, off both axes)."""
    rng = np.random.default_rng(seed)
    keep = np.zeros((0, 3))
    for _ in range(64):
        X = np.c_[rng.uniform(-12, 12, (8192, 2)), rng.uniform(zmin, zmax, 8192)]
        X2 = X @ R.T + t
        ok = (X2[:, 2] > zmin) & (X2[:, 2] < zmax) & (np.abs(X[:, :2] / X[:, 2:]).max(1) < 5.0) \
            & (np.abs(X2[:, :2] / X2[:, 2:]).max(1) < 5.0)
        keep = np.concatenate([keep, X[ok]])
        if len(keep) >= n:
            break
    if len(keep) < n:
        if zmin > 0.1:  # a twisted pair: the points between the two cameras are nearer than the baseline
            return points_in_front(R, t, n, K, seed, 0.05, 1.5)
        raise ValueError("no points in front of both cameras of this decomposition")
    X = keep[:n]
    return _px(X, K), _px(X @ R.T + t, K)


def pose_scene(oracle, E, parts, K=K_SKEW, seed=0):
    """Correspondences for E: `parts` is [(decomposition, n), ...]; n points in front of both
    cameras of each listed decomposition, concatenated."""
    dec = decompositions(oracle, E)
    p1s, p2s = [], []
    for k, (c, n) in enumerate(parts):
        a, b = points_in_front(dec[c][0], dec[c][1], n, K, 100 * seed + 7 * c + k)
        p1s.append(a)
        p2s.append(b)
    return np.concatenate(p1s), np.concatenate(p2s)


def pose_counts(oracle, E, p1, p2, K, dist_thresh, mask=None):
    """The four cheirality counts of recoverPose (host restatement on the oracle's
    triangulation; only test_geometry_cases.py uses it, to check the scenes)."""
    ax, ay = 1.0 / K[0, 0], 1.0 / K[1, 1]
    n1 = np.stack([p1[:, 0] * ax + -K[0, 2] * ax, p1[:, 1] * ay + -K[1, 2] * ay])
    n2 = np.stack([p2[:, 0] * ax + -K[0, 2] * ax, p2[:, 1] * ay + -K[1, 2] * ay])
    P0 = np.hstack((np.eye(3), np.zeros((3, 1))))
    out = []
    for R, t in decompositions(oracle, E):
        P = np.hstack((R, t.reshape(3, 1)))
        X = oracle.triangulate(P0, P, n1, n2)
        with np.errstate(all="ignore"):
            ok = X[2] * X[3] > 0
            Q = X / X[3]
            z = P[2, 0] * Q[0] + P[2, 1] * Q[1] + P[2, 2] * Q[2] + P[2, 3] * Q[3]
            ok = ok & (Q[2] < dist_thresh) & (z > 0) & (z < dist_thresh)
        if mask is not None:
            ok = ok & (np.asarray(mask).ravel() != 0)
        out.append(int(ok.sum()))
    return out


# name -> (E, parts, expected pick).  The ties hold two decompositions' points in equal number:
# a noise-free point is in front of both cameras in exactly one decomposition, so those two
# counts are equal and maximal and recoverPose's >= chain takes the lower index.
POSE_SCENES = {
    "pick0": (POSE_E, [(0, 200)], 0),
    "pick1": (POSE_E, [(1, 200)], 1),
    "pick2": (POSE_E, [(2, 200)], 2),
    "pick3": (POSE_E, [(3, 200)], 3),
    "tie01": (POSE_E, [(0, 90), (1, 90)], 0),
    "tie12": (POSE_E, [(1, 90), (2, 90)], 1),
    "tie13": (POSE_E, [(3, 90), (1, 90)], 1),
    "tie23": (POSE_E, [(3, 90), (2, 90)], 2),
    "axis": (AXIS_E, [(0, 60), (1, 60), (2, 60), (3, 61)], 3),
}


POSE_RANSAC_THRESHOLD = 1e-5  # the scenes are noise-free up to float32 pixels: a partial inlier mask


def ransac_mask(oracle, p1, p2, K):
    """findEssentialMat's 0/1 inlier mask of a pose scene (the reference passes none, v3:303)."""
    return oracle.find_essential(p1, p2, K, 0.999, POSE_RANSAC_THRESHOLD, 200)[1]


def pose_masks(m, ransac_mask, seed=0):
    """The mask_in variants of a pose case: none, findEssentialMat's 0/1 mask, the same as
    0/255, a sparse 0/1 mask, and arbitrary byte values (recoverPose ands them into its 0/255
    mask: bitwise_and(mask, mask1, mask1))."""
    rng = np.random.default_rng(seed + m)
    sparse = (rng.random(m) < 0.08).astype(np.uint8)
    mixed = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), m)
    r = np.asarray(ransac_mask, np.uint8).ravel()
    return {"none": None, "ransac01": r, "ransac255": (r * 255).astype(np.uint8), "sparse": sparse, "bytes": mixed}


# ---- triangulatePoints ------------------------------------------------------------------------
def triangulation_case(kind, k, seed=0):
    """(P1, P2, x1, x2) with x 2 x k."""
    rng = np.random.default_rng(seed * 7919 + k)
    K = K_SKEW
    X = np.c_[rng.uniform(-1.5, 1.5, (k, 2)), rng.uniform(3, 8, k)]
    Ra, Rb = _rot([0.1, -0.5, 1.0], 0.2), _rot([0.2, 1.0, 0.1], -0.15)
    ta, tb = np.array([0.1, -0.2, 0.05]), np.array([0.5, 0.05, 0.1])
    if kind == "general":
        P1, P2 = K @ np.c_[Ra, ta], K @ np.c_[Rb, tb]
    elif kind == "canonical":
        P1, P2 = K @ np.c_[np.eye(3), np.zeros(3)], K @ np.c_[Rb, tb]
    elif kind == "same":  # P1 == P2: the DLT matrix has rank 2
        P1 = P2 = K @ np.c_[Rb, tb]
    elif kind == "integer":
        P1, P2 = K @ np.c_[np.eye(3), np.zeros(3)], K @ np.c_[Rb, tb]
    else:
        raise ValueError(kind)
    Xh = np.c_[X, np.ones(k)]
    x1 = (P1 @ Xh.T)
    x2 = (P2 @ Xh.T)
    x1, x2 = x1[:2] / x1[2], x2[:2] / x2[2]
    if kind == "integer":
        x1, x2 = np.round(x1), np.round(x2)
    else:
        x1, x2 = x1 + rng.normal(0, 0.3, x1.shape), x2 + rng.normal(0, 0.3, x2.shape)
    return P1, P2, np.ascontiguousarray(x1), np.ascontiguousarray(x2)


TRI_KINDS = ("general", "canonical", "same", "integer")


# ---- few-match frames -------------------------------------------------------------------------
W, H, NF = 320, 240, 300


def square_frame(seed):
    """A 320x240 frame of constant 90 with one square of side 3-8 px and value 125-200."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 90, np.uint8)
    side = int(rng.integers(3, 9))
    val = int(rng.integers(125, 201))
    x = int(rng.integers(60, W - 60 - side))
    y = int(rng.integers(60, H - 60 - side))
    img[y:y + side, x:x + side] = val
    return img


def blank_frame():
    return np.full((H, W), 90, np.uint8)


# Seeds of square_frame: after synthetic frame 1 they give consecutive pairs with 1..4 matches,
# 5 matches (several models) and >= 6 matches (one model); test_geometry_cases.py asserts it.
SQUARE_CHAIN = (0, 18, 15)
MIXED_KINDS = ("normal", "few", "five", "model", "blank")


def mixed_batch():
    """(frames uint8[6, H, W], K): consecutive pairs are a normal pair, one with 1..4 matches,
    one with exactly 5, one with >= 6 and a model, and one against a blank frame."""
    from conftest import synth_frames
    frames, K = synth_frames(W, H, range(2))
    seq = [frames[0], frames[1]] + [square_frame(s) for s in SQUARE_CHAIN] + [blank_frame()]
    return np.ascontiguousarray(np.stack(seq)), K


def mixed_reference(oracle):
    """oracle.pair_pose of the mixed batch's pairs, each frame detected once."""
    frames, K = mixed_batch()
    refs, kp_prev = [], None
    for i in range(len(frames) - 1):
        ref = pair_reference(oracle, frames[i], frames[i + 1], K, kp_prev=kp_prev)
        kp_prev = (ref["kp_cur"], ref["desc_cur"])
        refs.append(ref)
    return refs


def pair_successful(ref):
    """The pose tail's rule on the oracle's side: findEssentialMat returned one E and recoverPose ran."""
    return ref["E"] is not None and ref["E"].shape[0] == 3 and len(ref["kp_prev"]) > 0 and len(ref["kp_cur"]) > 0


def pair_reference(oracle, prev, cur, K, kp_prev=None, **kw):
    return oracle.pair_pose(prev, cur, K, NF, kp_prev=kp_prev, **kw)


def assert_record_equals(r, ref, codes):
    """One dvo_pair_record against oracle.pair_pose's dict, every field.  codes: the module
    with the DVO_* status constants."""
    m = len(ref["q"])
    n_prev, n_cur = len(ref["kp_prev"]), len(ref["kp_cur"])
    assert r["n_kp_prev"] == n_prev and r["n_kp_cur"] == n_cur
    zero3, zero9 = np.zeros(3), np.zeros(9)
    if n_prev == 0 or n_cur == 0:
        assert r["status"] == codes.DVO_ENOFEAT
        want_E, rows, inl, iters = None, 0, 0, 0
    elif m < 5:
        assert ref["E"] is None
        assert r["status"] == codes.DVO_EFEWPTS
        want_E, rows, inl, iters = None, 0, 0, 0
    elif ref["E"] is None:
        assert r["status"] == codes.DVO_ENOMODEL
        want_E, rows, inl, iters = None, 0, 0, (1 if m == 5 else ref["iters"])
    else:
        assert r["status"] == codes.DVO_OK
        want_E, rows = ref["E"], ref["E"].shape[0]
        inl = int(ref["mask"].sum())
        iters = 1 if m == 5 else ref["iters"]
    assert r["n_matches"] == m
    assert r["n_models"] == rows // 3
    assert r["n_inliers"] == inl
    assert r["ransac_iters"] == iters
    np.testing.assert_array_equal(r["E"], zero9 if want_E is None else want_E[:3].ravel())
    if want_E is not None and rows == 3:
        np.testing.assert_array_equal(r["R"], ref["R"].ravel())
        np.testing.assert_array_equal(r["t"], ref["t_unit"].ravel())
        assert r["n_good"] == ref["good"]
    else:
        np.testing.assert_array_equal(r["R"], zero9)
        np.testing.assert_array_equal(r["t"], zero3)
        assert r["n_good"] == 0
