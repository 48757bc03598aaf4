"""Landmarks (dvo_stream_set_landmarks): the expected entries of a pair from the CPU oracle, and
seeded correspondence sets at sizes chosen around the kernel's tiles of 256 matches.

A landmark is a correspondence that findEssentialMat's mask keeps and that passes recoverPose's
tests for the decomposition recoverPose chose; its position is the dehomogenised DLT triangulation
against that decomposition's [R | t], in the previous frame's camera coordinates."""
import numpy as np

K_CASE = np.array([[525.0, 0, 319.5], [0, 525.0, 239.5], [0, 0, 1]])
SIZES = (5, 6, 63, 64, 65, 255, 256, 257, 513)


def case(m):
    """m correspondences of a scene 3 to 9 units in front of a camera that turns 0.05 rad about y
    and moves by (0.3, 0.02, 0.05): 0.3 px of noise on both sides, every fifth match an outlier
    anywhere in the second image.  float32 [m, 2] pixel coordinates twice, and K."""
    r = np.random.RandomState(7 + m)
    X = np.stack([r.uniform(-2, 2, m), r.uniform(-1.5, 1.5, m), r.uniform(3, 9, m)], 1)
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.array([0.3, 0.02, 0.05])

    def proj(P):
        return np.stack([525.0 * P[:, 0] / P[:, 2] + 319.5, 525.0 * P[:, 1] / P[:, 2] + 239.5], 1)

    p1 = proj(X)
    p2 = proj(X @ R.T + t)
    p1 = p1 + r.normal(0, 0.3, (m, 2))
    p2 = p2 + r.normal(0, 0.3, (m, 2))
    out = np.arange(m) % 5 == 4
    k = int(out.sum())
    p2[out, 0] = r.uniform(0, 640, k)
    p2[out, 1] = r.uniform(0, 480, k)
    return p1.astype(np.float32), p2.astype(np.float32), K_CASE.copy()


def masks(oracle, p1, p2, K):
    """(E, findEssentialMat's mask, recoverPose's mask without an input mask, R, t) of float64
    [m, 2] points; E is None or has other than 3 rows where the reference goes no further."""
    E, mask, _ = oracle.find_essential(p1, p2, K)
    if E is None or E.shape[0] != 3:
        return E, None, None, None, None
    _, R, t, pose = oracle.recover_pose(E, p1, p2, K)
    return E, mask, pose, R, t


def expected(oracle, p1, p2, K, rec=None):
    """The pair's landmarks: dict(count, match int32 [n], xyz float64 [n, 3], only_pose,
    only_inlier) from float64 [m, 2] points in match order.  rec (the pair's record, if given)
    must agree with the oracle on whether the pair got through, and on E."""
    p1 = np.ascontiguousarray(p1, np.float64)
    p2 = np.ascontiguousarray(p2, np.float64)
    empty = dict(count=0, match=np.zeros(0, np.int32), xyz=np.zeros((0, 3)), only_pose=0, only_inlier=0)
    E, mask, pose, R, t = masks(oracle, p1, p2, K) if len(p1) >= 5 else (None,) * 5
    ok = E is not None and E.shape[0] == 3
    if rec is not None:
        assert (rec["status"] == 0 and rec["n_models"] == 1) == ok, (rec["status"], rec["n_models"])
        if ok:
            np.testing.assert_array_equal(rec["E"].reshape(3, 3), E)
    if not ok:
        return empty
    keep = np.flatnonzero((mask != 0) & (pose != 0))
    # the oracle's normalisation (OpenCV's MatExpr): col * (1 / f) + (-c * (1 / f)), two roundings
    ax, ay = 1.0 / K[0, 0], 1.0 / K[1, 1]
    bx, by = -K[0, 2] * ax, -K[1, 2] * ay

    def norm(p):
        x = p[keep, 0] * ax
        x = x + bx
        y = p[keep, 1] * ay
        y = y + by
        return np.stack([x, y])

    xyz = np.zeros((0, 3))
    if len(keep):
        P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
        P1 = np.hstack([R + 0.0, t.reshape(3, 1)])
        X = oracle.triangulate(P0, P1, norm(p1), norm(p2))
        xyz = (X[:3] / X[3]).T.copy()
    return dict(count=len(keep), match=keep.astype(np.int32), xyz=xyz,
                only_pose=int(((mask == 0) & (pose != 0)).sum()), only_inlier=int(((mask != 0) & (pose == 0)).sum()))


def check_pair(entries, count, cap, want, p1, p2):
    """One pair's device output against `want`: the count, and the first min(count, cap) entries
    (match index, the float32 pixel coordinates, X Y Z bit for bit)."""
    assert count == want["count"], (count, want["count"])
    n = min(want["count"], cap)
    assert len(entries) == n
    np.testing.assert_array_equal(entries["match"], want["match"][:n])
    assert not entries["reserved"].any()
    idx = want["match"][:n]
    for name, col in (("x1", p1[:, 0]), ("y1", p1[:, 1]), ("x2", p2[:, 0]), ("y2", p2[:, 1])):
        np.testing.assert_array_equal(entries[name], np.asarray(col, np.float32)[idx], err_msg=name)
    got = np.stack([entries["X"], entries["Y"], entries["Z"]], 1) if n else np.zeros((0, 3))
    np.testing.assert_array_equal(got, want["xyz"][:n])


def untouched(raw, counts, cap, fill=0xA5):
    """Every byte of the entry buffer (uint8 [pairs, cap, 48]) outside the written slots holds the fill."""
    for p, c in enumerate(counts):
        assert (raw[p, min(int(c), cap):] == fill).all(), p
