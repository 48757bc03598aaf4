"""Track PnP (dvo_stream_set_track_pnp): a numpy restatement of the contract in include/dvo.h,
operation for operation (numpy float64 scalars and arrays round each operation once), and a seeded
generator of chains for the tests.

Pair p's correspondences are its raw matches, in match order, whose queryIdx is the trainIdx of a
landmark of pair p - 1: Y from that landmark and pair p - 1's record, (nu, nv) the match's float x2,
y2 normalised.  Seeded samples of three, P3P on each, the pose with the most supporters, then the
track-pose steps over its supporters and the track-pose final pass over all correspondences."""
import numpy as np

import track_cases as tc
import track_pose_cases as pc
from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE, TRACK_PNP_DTYPE

OK, NONE, DEGENERATE, NO_MODEL = 0, 1, 2, 3
F8 = np.float64

# ---- 1. the samples -----------------------------------------------------------------------------
MWC_A = 4164903690
MWC_M = MWC_A * 2 ** 32 - 1
DEFAULT_SEED = 2 ** 64 - 1


def mwc_step(s):
    return (s & 0xFFFFFFFF) * MWC_A + (s >> 32)


def mwc_jump_by(s, k):
    """The state k steps after s: s * A^k mod m, a state at or above m taking one plain step first."""
    if k == 0:
        return s
    if s >= MWC_M:
        s = mwc_step(s)
        k -= 1
    r = s - MWC_M if s >= MWC_M else s
    return r * pow(MWC_A, k, MWC_M) % MWC_M


def sample(n, h, seed=0):
    """Sample h of n correspondences: (i0, i1, i2), or None where 8 draws do not give three."""
    s = mwc_jump_by(seed or DEFAULT_SEED, 8 * h)
    got = []
    for _ in range(8):
        s = mwc_step(s)
        i = (s & 0xFFFFFFFF) % n
        if len(got) < 3 and i not in got:
            got.append(i)
    return tuple(got) if len(got) == 3 else None


def samples(n, hyps, seed=0):
    """int32 [hyps, 3]; a void sample is -1."""
    out = np.full((hyps, 3), -1, np.int32)
    for h in range(hyps):
        s = sample(n, h, seed)
        if s is not None:
            out[h] = s
    return out


# ---- 2. P3P --------------------------------------------------------------------------------------
BISECT, NEWTON = 100, 5


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _frame(z1, z2, l1):
    F1 = [z1[j] / l1 for j in range(3)]
    n = [F1[1] * z2[2] - F1[2] * z2[1], F1[2] * z2[0] - F1[0] * z2[2], F1[0] * z2[1] - F1[1] * z2[0]]
    l3 = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    F3 = [n[j] / l3 for j in range(3)]
    F2 = [F3[1] * F1[2] - F3[2] * F1[1], F3[2] * F1[0] - F3[0] * F1[2], F3[0] * F1[1] - F3[1] * F1[0]]
    return F1, F2, F3


def p3p(Y, nunv):
    """Y [3, 3], nunv [3, 2] -> (R [k, 3, 3], t [k, 3]) of the kept solutions, in the header's order."""
    Y = [[F8(v) for v in row] for row in np.asarray(Y, F8).reshape(3, 3)]
    nunv = np.asarray(nunv, F8).reshape(3, 2)
    with np.errstate(all="ignore"):
        f = []
        for i in range(3):
            nu, nv = F8(nunv[i, 0]), F8(nunv[i, 1])
            ln = np.sqrt((nu * nu + nv * nv) + 1)
            f.append([nu / ln, nv / ln, 1 / ln])
        c01, c02, c12 = _dot(f[0], f[1]), _dot(f[0], f[2]), _dot(f[1], f[2])
        e1 = [Y[1][j] - Y[0][j] for j in range(3)]
        e2 = [Y[2][j] - Y[0][j] for j in range(3)]
        g = [Y[2][j] - Y[1][j] for j in range(3)]
        a01, a02, a12 = _dot(e1, e1), _dot(e2, e2), _dot(g, g)
        p2, p1, q2 = a02, -((2 * a02) * c01), a12 - a01
        P0 = [a02 - a01, (2 * a01) * c02, -a01]
        Q1 = [-((2 * a12) * c01), (2 * a01) * c12]
        Q0 = [a12, F8(0.0), -a01]
        A = [p2 * Q0[k] - P0[k] * q2 for k in range(3)]
        B = [p2 * Q1[0] - p1 * q2, p2 * Q1[1]]
        C = [p1 * Q0[0] - P0[0] * Q1[0],
             p1 * Q0[1] - (P0[0] * Q1[1] + P0[1] * Q1[0]),
             p1 * Q0[2] - (P0[1] * Q1[1] + P0[2] * Q1[0]),
             -(P0[2] * Q1[1])]
        G = [A[0] * A[0] - B[0] * C[0],
             2 * (A[0] * A[1]) - (B[0] * C[1] + B[1] * C[0]),
             (2 * (A[0] * A[2]) + A[1] * A[1]) - (B[0] * C[2] + B[1] * C[1]),
             2 * (A[1] * A[2]) - (B[0] * C[3] + B[1] * C[2]),
             A[2] * A[2] - B[1] * C[3]]
        b, c, d, e = G[3] / G[4], G[2] / G[4], G[1] / G[4], G[0] / G[4]
        b2 = b * b
        p = c - 0.375 * b2
        q = (d - 0.5 * (b * c)) + 0.125 * (b2 * b)
        r = ((e - 0.25 * (b * d)) + 0.0625 * (b2 * c)) - 0.01171875 * (b2 * b2)
        k2, k1, k0 = p, 0.25 * (p * p) - r, -(0.125 * (q * q))
        lo = F8(0.0)
        m2, m1, m0 = (-k2 if k2 < 0 else k2), (-k1 if k1 < 0 else k1), (-k0 if k0 < 0 else k0)
        mx = m2 if m2 > m1 else m1
        hi = 1 + (mx if mx > m0 else m0)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            gm = ((mid + k2) * mid + k1) * mid + k0
            if gm > 0:
                hi = mid
            else:
                lo = mid
        m = hi
        s = np.sqrt(2 * m)
        hh, w = 0.5 * p + m, q / (2 * s)
        rt0, rt1 = np.sqrt(s * s - 4 * (hh + w)), np.sqrt(s * s - 4 * (hh - w))
        ys = [0.5 * (s + rt0), 0.5 * (s - rt0), 0.5 * (rt1 - s), 0.5 * (-s - rt1)]
        E1, E2, E3 = _frame(e1, e2, np.sqrt(a01))
        Rs, ts = [], []
        for y in ys:
            v = y - 0.25 * b
            u = -(((A[2] * v + A[1]) * v + A[0]) / (B[1] * v + B[0]))
            d0 = np.sqrt(a02 / ((1 + v * v) - (2 * v) * c02))
            d1, d2 = u * d0, v * d0
            for _ in range(NEWTON):
                r0 = ((d0 * d0 + d1 * d1) - (2 * (d0 * d1)) * c01) - a01
                r1 = ((d0 * d0 + d2 * d2) - (2 * (d0 * d2)) * c02) - a02
                r2 = ((d1 * d1 + d2 * d2) - (2 * (d1 * d2)) * c12) - a12
                j00, j01 = 2 * (d0 - d1 * c01), 2 * (d1 - d0 * c01)
                j10, j12 = 2 * (d0 - d2 * c02), 2 * (d2 - d0 * c02)
                j21, j22 = 2 * (d1 - d2 * c12), 2 * (d2 - d1 * c12)
                det = -(j00 * (j12 * j21) + j01 * (j10 * j22))
                x = r1 * j22 - j12 * r2
                n0 = -(r0 * (j12 * j21)) - j01 * x
                n1 = j00 * x - r0 * (j10 * j22)
                n2 = (r0 * (j10 * j21) - j00 * (r1 * j21)) - j01 * (j10 * r2)
                d0, d1, d2 = d0 - n0 / det, d1 - n1 / det, d2 - n2 / det
            X0 = [d0 * f[0][j] for j in range(3)]
            x1 = [d1 * f[1][j] - X0[j] for j in range(3)]
            x2 = [d2 * f[2][j] - X0[j] for j in range(3)]
            F1, F2, F3 = _frame(x1, x2, np.sqrt((x1[0] * x1[0] + x1[1] * x1[1]) + x1[2] * x1[2]))
            R = np.zeros((3, 3))
            t = np.zeros(3)
            for i in range(3):
                for j in range(3):
                    R[i, j] = (F1[i] * E1[j] + F2[i] * E2[j]) + F3[i] * E3[j]
                t[i] = X0[i] - ((R[i, 0] * Y[0][0] + R[i, 1] * Y[0][1]) + R[i, 2] * Y[0][2])
            if d0 > 0 and d1 > 0 and d2 > 0 and np.isfinite(R).all() and np.isfinite(t).all():
                Rs.append(R)
                ts.append(t)
    return np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3)


# ---- 3. a pair, and a batch ----------------------------------------------------------------------
def supporters(Y, nu, nv, R, t, K, inlier_px):
    """The final pass's inlier test per correspondence, its P2 > 0 and its e (squared pixels)."""
    fx, fy = K[0, 0], K[1, 1]
    P = pc._project(Y, R, t)
    ok = P[2] > 0
    with np.errstate(all="ignore"):
        a = 1.0 / P[2]
        ex, ey = fx * (P[0] * a - nu), fy * (P[1] * a - nv)
        e = ex * ex + ey * ey
        inl = ok & (e <= inlier_px * inlier_px)
    return inl, ok, e


def pnp_pair(Y, nu, nv, K, hyps=128, iters=10, huber_px=1.0, inlier_px=2.0, min_points=6, seed=0):
    """The PnP of one pair with n = len(Y) >= min_points correspondences.  Returns a dict with the
    struct's fields (R [3, 3]) and inl: the final pass's inlier flags [n]."""
    K = np.asarray(K, F8).reshape(3, 3)
    n = len(Y)
    out = dict(R=np.zeros((3, 3)), t=np.zeros(3), scale=0.0, rms=0.0, n_corr=n, n_best=0, n_used=0, n_inliers=0,
               sample=-1, solution=-1, iters=0, status=NO_MODEL, inl=np.zeros(n, bool))
    best = None
    for h in range(hyps):
        idx = sample(n, h, seed)
        if idx is None:
            continue
        idx = list(idx)
        Rs, ts = p3p(Y[idx], np.stack([nu[idx], nv[idx]], 1))
        for s in range(len(Rs)):
            count = int(supporters(Y, nu, nv, Rs[s], ts[s], K, inlier_px)[0].sum())
            if best is None or count > best[0]:  # ascending (h, s): a tie keeps the earlier one
                best = (count, h, s, Rs[s], ts[s])
    if best is None:
        return out
    out["n_best"], out["sample"], out["solution"] = best[0], best[1], best[2]
    if best[0] < min_points:
        return out
    sup = supporters(Y, nu, nv, best[3], best[4], K, inlier_px)[0]
    r = pc.refine(Y[sup], nu[sup], nv[sup], best[3], best[4], K, iters, huber_px, inlier_px)
    R, t = r["R"], r["t"]
    inl, ok, e = supporters(Y, nu, nv, R, t, K, inlier_px)
    n_in = int(inl.sum())
    total = pc.tree_sum(np.where(inl, e, 0.0)[:, None])[0]
    out.update(R=R, t=t, scale=np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]),
               rms=np.sqrt(total / F8(n_in)) if n_in else 0.0, n_used=int(ok.sum()), n_inliers=n_in,
               iters=r["iters"], status=r["status"], inl=inl)
    return out


def correspondences(lms, xy2, matches, recs, K, p):
    """Pair p's correspondences: (match indices i ascending, Y [n, 3], nu, nv)."""
    if p == 0 or len(lms[p - 1][0]) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros(0), np.zeros(0)
    pm, pxyz = lms[p - 1]
    first = {}  # trainIdx of pair p - 1 -> its smallest landmark ordinal
    for o, i in enumerate(pm):
        first.setdefault(int(matches[p - 1][1][i]), o)
    q = matches[p][0]
    hit = [(i, first[int(q[i])]) for i in range(len(q)) if int(q[i]) in first]
    idx = np.array([i for i, _ in hit], np.int64)
    ordn = np.array([o for _, o in hit], np.int64)
    Y = pc.points_in_first_camera(pxyz[ordn].reshape(-1, 3), recs[p - 1]["R"], recs[p - 1]["t"])
    nu, nv = pc.normalise(np.asarray(xy2[p], np.float32).reshape(-1, 2)[idx], K)
    return idx, Y, nu, nv


def reference(lms, xy2, matches, recs, K, hyps=128, iters=10, huber_px=1.0, inlier_px=2.0, min_points=6, seed=0):
    """lms, matches, recs as track_cases.reference takes them; xy2: per pair float32 [m, 2], every
    match's second-frame pixel.  Returns (pnp TRACK_PNP_DTYPE [P], masks: per pair uint8 [m], info:
    per pair the pnp_pair dict or None)."""
    K = np.asarray(K, F8).reshape(3, 3)
    P = len(lms)
    pnp = np.zeros(P, TRACK_PNP_DTYPE)
    masks, info = [], []
    for p in range(P):
        mask = np.zeros(len(matches[p][0]), np.uint8)
        idx, Y, nu, nv = correspondences(lms, xy2, matches, recs, K, p)
        pnp[p]["n_corr"] = len(idx)
        if p == 0 or len(idx) < min_points:
            pnp[p]["status"] = NONE
            masks.append(mask)
            info.append(None)
            continue
        r = pnp_pair(Y, nu, nv, K, hyps, iters, huber_px, inlier_px, min_points, seed)
        pnp[p]["R"], pnp[p]["t"] = r["R"].reshape(9), r["t"]
        for f in ("scale", "rms", "n_best", "n_used", "n_inliers", "sample", "solution", "iters", "status"):
            pnp[p][f] = r[f]
        mask[idx[r["inl"]]] = 1
        masks.append(mask)
        info.append(r)
    return pnp, masks, info


def pack(lms, xy2, matches, recs, cap, stride):
    """The hook's arrays (ops.test_track_pnp): track_pose_cases.pack with every match's pixel, xy2 [P, stride, 2]."""
    lxy = [np.asarray(xy2[p], np.float32).reshape(-1, 2)[lms[p][0]] for p in range(len(lms))]
    lm, count, mq, mt, m = pc.pack(lms, lxy, matches, recs, cap, stride)
    px = np.zeros((len(lms), stride, 2), np.float32)
    for p in range(len(lms)):
        px[p, :m[p]] = xy2[p]
    return lm, count, mq, mt, m, px


# ---- 4. seeded chains for the hook: sizes set exactly, noise-free truth ---------------------------
K_CHAIN = pc.K_CHAIN
FAILED = -5  # the status a failed pair's record gets (any non-zero value: only the landmark list matters)


def chain(spec, extras, kp_cap, seed, outliers=0.0, noise=0.0, behind=0, fail=(), identical=False):
    """track_cases.chain's index structure (spec = [(m, count, n_common), ...]) with the decoy
    matches (those that are no landmark) rewritten so that exactly extras[p] of pair p's hit a
    landmark of pair p - 1: unlinked raw matches that are correspondences all the same, n_corr[p] =
    n_common + extras[p].  Every other decoy hits none.

    Geometry.  Pair p has a true motion (R_p, s_p d_p), d_p a unit vector and s_p the baseline ratio;
    its record holds R_p and d_p.  A correspondence is built backwards from what the camera sees: a
    float32 pixel of frame p + 1, a depth of 3 to 9, the point X' behind that pixel, Y = R_p^T (X' -
    s_p d_p) in camera p, and the previous pair's landmark R_{p-1}^T (Y - d_{p-1}) that the kernels
    turn into Y again; so without noise the true pose reprojects to about 1e-13 px.  A share
    `outliers` of every pair's correspondences, the unlinked ones first, has its pixel displaced by 20
    to 200 px; `noise`: normal pixel noise on all; behind: that many correspondences per pair lie
    behind camera p + 1 (their depth negated); identical: every correspondence is one point at one
    pixel.  fail: pairs whose record is marked failed (their spec must have count 0).
    Returns dict(lms, xy2, matches, recs, truth: per pair None or (R, t, inlier match indices))."""
    lms, matches, recs = tc.chain(spec, kp_cap, seed)
    r = np.random.RandomState(seed + 104729)
    P = len(spec)
    K = K_CHAIN
    lms = [(a, b.copy()) for a, b in lms]
    matches = [(a.copy(), b) for a, b in matches]
    for p in range(P):
        q, t = matches[p]
        land = lms[p][0]
        m = len(q)
        is_land = np.zeros(m, bool)
        is_land[land] = True
        decoy = np.flatnonzero(~is_land)
        T_prev = np.unique(matches[p - 1][1][lms[p - 1][0]]) if p >= 1 else np.zeros(0, np.int64)
        free_hit = np.setdiff1d(T_prev, q[land])
        outside = np.setdiff1d(np.arange(kp_cap), np.union1d(T_prev, q[land]))
        e = extras[p] if p >= 1 else 0
        assert e <= min(len(decoy), len(free_hit)) and len(outside) >= len(decoy) - e, (p, e, len(decoy), len(free_hit))
        hit = r.choice(decoy, e, replace=False) if e else np.zeros(0, np.int64)
        if e:
            q[hit] = r.choice(free_hit, e, replace=False)
        rest = np.setdiff1d(decoy, hit)
        q[rest] = r.permutation(outside)[:len(rest)]
        assert len(np.unique(q)) == m
    motion = []
    for p in range(P):
        Rr = pc.small_rotation(r, 0.05)
        d = np.array([1.0, r.uniform(-0.3, 0.3), r.uniform(-0.3, 0.3)])
        d /= np.linalg.norm(d)
        s = r.uniform(0.5, 2.0)
        recs[p]["R"], recs[p]["t"] = Rr.reshape(9), d
        if p in fail:
            assert len(lms[p][0]) == 0
            recs[p]["status"] = FAILED
        motion.append((recs[p]["R"].reshape(3, 3).astype(F8), recs[p]["t"].astype(F8), s))
    xy2, truth = [], []
    for p in range(P):
        m = len(matches[p][0])
        px = np.stack([r.uniform(0, 640, m), r.uniform(0, 480, m)], 1).astype(np.float32)
        idx = correspondences(lms, [None] * p + [px], matches, recs, K, p)[0] if p >= 1 else np.zeros(0, np.int64)
        n = len(idx)
        if n == 0:
            xy2.append(px)
            truth.append(None)
            continue
        Rp, dp, sp = motion[p]
        Rq, dq, _ = motion[p - 1]
        tp = sp * dp
        first = {}
        for o, i in enumerate(lms[p - 1][0]):
            first.setdefault(int(matches[p - 1][1][i]), o)
        pix = np.stack([r.uniform(20, 620, n), r.uniform(20, 460, n)], 1).astype(np.float32)
        depth = r.uniform(3, 9, n)
        if identical:
            pix[:], depth[:] = pix[0], depth[0]
        back = r.choice(n, min(behind, n), replace=False) if behind else np.zeros(0, np.int64)
        depth[back] *= -1.0
        Xc = np.stack([(pix[:, 0].astype(F8) - K[0, 2]) / K[0, 0], (pix[:, 1].astype(F8) - K[1, 2]) / K[1, 1],
                       np.ones(n)], 1) * depth[:, None]
        Y = (Xc - tp) @ Rp  # R_p^T (X' - t_p), row by row
        Xa = (Y - dq) @ Rq
        for k, i in enumerate(idx):
            lms[p - 1][1][first[int(matches[p][0][i])]] = Xa[k]
        is_land = np.zeros(m, bool)
        is_land[lms[p][0]] = True
        n_out = int(round(outliers * n))
        order = np.concatenate([np.flatnonzero(~is_land[idx]), np.flatnonzero(is_land[idx])])  # the unlinked ones first
        bad = order[:n_out]
        shown = pix.astype(F8)
        if n_out:
            ang, mag = r.uniform(0, 2 * np.pi, n_out), r.uniform(20, 200, n_out)
            shown[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
        if noise:
            shown = shown + r.normal(0, noise, shown.shape)
        px[idx] = shown.astype(np.float32)
        good = np.ones(n, bool)
        good[bad] = False
        good[back] = False
        xy2.append(px)
        truth.append((Rp, tp, idx[good]))
    return dict(lms=lms, xy2=xy2, matches=matches, recs=recs, truth=truth)


# ---- 5. seeded triples for the solver's own tests -------------------------------------------------
# The generator's ranges: depths 2 to 10 and an image triangle of at least MIN_AREA square pixels, so
# that the three rays are far from collinear; test_track_pnp_host.py measures the share of triples
# whose kept solutions miss the true pose by more than 1e-9 with this restatement alone.
MIN_AREA = 2000.0


def triples(count, seed):
    """count seeded (Y [3, 3], nunv [3, 2], R, t): three points 2 to 10 deep in the second camera at
    pixels of a 640 x 480 image whose triangle has at least MIN_AREA px^2, and a seeded pose."""
    r = np.random.RandomState(seed)
    K = K_CHAIN
    out = []
    while len(out) < count:
        px = np.stack([r.uniform(0, 640, 3), r.uniform(0, 480, 3)], 1)
        a, b = px[1] - px[0], px[2] - px[0]
        if abs(a[0] * b[1] - a[1] * b[0]) / 2 < MIN_AREA:
            continue
        R = pc.small_rotation(r, 0.3)
        t = r.uniform(-1, 1, 3)
        nunv = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1]], 1)
        X = np.concatenate([nunv, np.ones((3, 1))], 1) * r.uniform(2, 10, (3, 1))
        Y = (X - t) @ R
        out.append((Y, nunv, R, t))
    return out


def pose_error(Rs, ts, R, t):
    """The smallest max-abs deviation of a kept solution from (R, t); inf with none kept."""
    if len(Rs) == 0:
        return np.inf
    return min(max(np.abs(Rs[s] - R).max(), np.abs(ts[s] - t).max()) for s in range(len(Rs)))
