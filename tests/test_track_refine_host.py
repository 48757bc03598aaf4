"""Track ids and refined landmarks without a GPU: the ABI's structs and the numpy dtypes agree, both
sides name the new entry points, and the numpy restatement the GPU tests compare against
(track_refine_cases) does what the header says: on a case small enough to write out, on ids
against two other ways of ranking the lists, as a float64 anchor of the formulas (true motions
and noiseless observations return the true point), on the accuracy it is for (closer to the truth
than the two-view point), and on the degenerate inputs."""
import os
import re
import types

import numpy as np
import pytest

import track_cases as tc
import track_pose_cases as pc
import track_refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dvo_stream_set_track_refine", "dvo_knn_stream_set_track_refine", "dvo_test_track_refine")
C_TYPES = {"int32_t": ("<i4", 4), "float": ("<f4", 4), "double": ("<f8", 8)}
K = pc.K_CHAIN


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


@pytest.mark.parametrize("struct, dtype, size", [("dvo_track_id", "TRACK_ID_DTYPE", 16),
                                                 ("dvo_landmark_refined", "LANDMARK_REFINED_DTYPE", 56)])
def test_struct_and_dtype_agree(struct, dtype, size):
    from droplet_visual_odometry_amd import _native
    dt = getattr(_native, dtype)
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        code, sz = C_TYPES[ctype]
        for name in (n.strip() for n in names.split(",")):
            off = (off + sz - 1) // sz * sz
            fields.append((name, code, off))
            off += sz
    assert off == dt.itemsize == size
    assert [f[0] for f in fields] == list(dt.names)
    for name, code, o in fields:
        assert dt.fields[name][0] == np.dtype(code) and dt.fields[name][1] == o, name
    h = _header()
    assert "sizeof(dvo_track_id) == 16 && sizeof(dvo_landmark_refined) == 56" in h
    for name, value in (("OK", 0), ("NONE", 1), ("DEGENERATE", 2)):
        assert re.search(r"#define DVO_TRACK_REFINE_%s %d\b" % (name, value), h)
        assert getattr(_native, "TRACK_REFINE_" + name) == getattr(rc, name) == value


def test_entry_points_declared_and_bound():
    from test_abi import declared_symbols
    from droplet_visual_odometry_amd import _native
    names = declared_symbols()
    for e in ENTRIES:
        assert e in names, e
        assert e in _native._SIGNATURES, e
    lib = _native.load_library()
    for e in ENTRIES:
        assert getattr(lib, e) is not None


def test_python_surface_and_binding_rules():
    import inspect
    import torch
    from droplet_visual_odometry_amd import ops, stream
    for cls in (stream.FrameStream, stream.KnnFrameStream):
        sig = inspect.signature(cls.bind_refine)
        got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
        assert got == dict(views=6, iters=5, huber_px=1.0, inlier_px=2.0, ids=True, refined=True)
    assert callable(ops.test_track_refine)
    for bad in ((0, 4), (2, 0)):
        with pytest.raises(ValueError):
            stream.RefinedLandmarks(*bad, "cpu")
    rf = stream.RefinedLandmarks(3, 5, "cpu")
    assert rf.refined.shape == (3, 5, 56) and rf.ids.shape == (3, 5, 16)
    assert rf.numpy(1, 9).shape == (5,) and rf.ids_numpy(2, 2).shape == (2,)
    # the wrapper's own checks: refine goes after tracks, with the bound Landmarks' cap and pairs
    calls = []
    dev = torch.device("cpu")
    fake = types.SimpleNamespace(h=None, device=dev, _after_torch=lambda: None, _lm_next=None, _tr_next=None,
                                 ctx=types.SimpleNamespace(check=lambda rc_: None))

    def setter(*a):
        calls.append(a)
        return 0

    with pytest.raises(ValueError):
        stream._bind_refine(fake, setter, rf, 6, 5, 1.0, 2.0, True, True)
    fake._lm_next = stream.Landmarks(3, 5, "cpu")
    with pytest.raises(ValueError):
        stream._bind_refine(fake, setter, rf, 6, 5, 1.0, 2.0, True, True)
    fake._tr_next = stream.Tracks(3, 5, "cpu")
    for wrong in (stream.RefinedLandmarks(3, 4, "cpu"), stream.RefinedLandmarks(2, 5, "cpu"), object()):
        with pytest.raises(ValueError):
            stream._bind_refine(fake, setter, wrong, 6, 5, 1.0, 2.0, True, True)
    assert not calls
    assert stream._bind_refine(fake, setter, rf, 4, 2, 0.5, 3.0, True, False) is rf
    assert calls[-1] == (None, None, rf.ids.data_ptr(), 4, 2, 0.5, 3.0)
    assert stream._bind_refine(fake, setter, rf, 4, 2, 0.5, 3.0, False, True) is rf
    assert calls[-1][1:3] == (rf.refined.data_ptr(), None)
    assert stream._bind_refine(fake, setter, None, 6, 5, 1.0, 2.0, True, True) is None
    assert calls[-1] == (None, None, None, 0, 0, 0.0, 0.0)
    assert stream._bind_refine(fake, setter, rf, 6, 5, 1.0, 2.0, False, False) is None  # neither output: a clear
    assert rc.defaults(0, -1, 0.0, -2.0) == (6, 5, 1.0, 2.0) and rc.defaults(8, 16, np.inf, 3.0) == (8, 16, np.inf, 3.0)


# ---- a case written out by hand ----------------------------------------------------------------
def _hand_case():
    """Three pairs of two landmarks.  Landmark 0 of every pair is one scene point (a chain of 3),
    landmark 1 of pair 2 links to landmark 1 of pair 1, which has no predecessor."""
    Rs = [pc.small_rotation(np.random.RandomState(s), 0.05) for s in (1, 2, 3)]
    ts = [np.array([0.30, 0.02, 0.05]), np.array([0.50, -0.04, 0.03]), np.array([0.40, 0.03, -0.06])]
    base = [np.linalg.norm(t) for t in ts]
    recs = np.zeros(3, pc.PAIR_RECORD_DTYPE)
    recs["n_models"] = 1
    for p in range(3):
        recs[p]["R"], recs[p]["t"] = Rs[p].reshape(9), ts[p] / base[p]
    Xa = np.array([0.4, -0.3, 5.0])     # in camera 0
    Xb = np.array([-0.7, 0.5, 6.5])     # in camera 1
    Xc0 = np.array([1.0, 1.0, 4.0])     # pair 0's second landmark, seen by pair 0 alone
    cams = [(np.eye(3), np.zeros(3))]
    for p in range(3):
        cams.append((Rs[p] @ cams[-1][0], Rs[p] @ cams[-1][1] + ts[p]))  # camera p + 1 from camera 0

    def px(Xw, j):  # a world (camera 0) point in camera j
        X = cams[j][0] @ Xw + cams[j][1]
        return X, np.float32([K[0, 0] * X[0] / X[2] + K[0, 2], K[1, 1] * X[1] / X[2] + K[1, 2]])

    Xb_w = Rs[0].T @ (Xb - ts[0])
    world = [[Xa, Xc0], [Xa, Xb_w], [Xa, Xb_w]]
    lms, xy1, xy2 = [], [], []
    for p in range(3):
        pts = [px(w, p) for w in world[p]]
        lms.append((np.arange(2, dtype=np.int32), np.stack([x / base[p] for x, _ in pts])))
        xy1.append(np.stack([q for _, q in pts]))
        xy2.append(np.stack([px(w, p + 1)[1] for w in world[p]]))
    # keypoints: pair p's landmark i has queryIdx 10 p + i and trainIdx 10 (p + 1) + i, but pair 0's
    # second landmark goes nowhere (trainIdx 19)
    matches = [(np.int32([0, 1]), np.int32([10, 19])), (np.int32([10, 11]), np.int32([20, 21])),
               (np.int32([20, 21]), np.int32([30, 31]))]
    return lms, xy1, xy2, matches, recs, world, base, cams


def test_restatement_written_out():
    lms, xy1, xy2, matches, recs, world, base, cams = _hand_case()
    links, scales, poses, refined, ids, info = rc.reference(lms, xy1, xy2, matches, recs, K, views=6, iters=6,
                                                            huber_px=np.inf)
    assert [list(l) for l in links] == [[-1, -1], [0, -1], [0, 1]]
    assert [i.tolist() for i in ids] == [[(0, 0, 0, 0), (0, 1, 0, 0)], [(0, 0, 1, 0), (1, 1, 0, 0)],
                                         [(0, 0, 2, 0), (1, 1, 1, 0)]]
    assert list(refined[0]["status"]) == [rc.NONE, rc.NONE] and list(refined[0]["views"]) == [2, 2]
    assert list(refined[1]["status"]) == [rc.OK, rc.NONE] and list(refined[1]["views"]) == [3, 2]
    assert list(refined[2]["status"]) == [rc.OK, rc.OK] and list(refined[2]["views"]) == [4, 3]
    for p in range(3):  # a NONE slot holds the landmark's own point and zeros
        for o in np.flatnonzero(refined[p]["status"] == rc.NONE):
            r = refined[p][o]
            assert (r["X"], r["Y"], r["Z"]) == tuple(lms[p][1][o]) and not (r["rms"] or r["n_used"] or r["iters"])
    # pair 2, landmark 0, by hand: the cameras of frames 3, 2 (its own), 1 and 0 relative to frame 2,
    # in units of baseline 2, from the records and the ratios, written as matrices
    rho = scales["ratio"]
    np.testing.assert_allclose(rho[1:], [base[1] / base[0], base[2] / base[1]], rtol=1e-12)  # XYZ is exact
    R = [recs[p]["R"].reshape(3, 3) for p in range(3)]
    d = [recs[p]["t"] for p in range(3)]
    A1, b1 = R[1].T, -R[1].T @ d[1] / rho[2]
    A2, b2 = R[0].T @ A1, R[0].T @ (b1 - d[0] / (rho[2] * rho[1]))
    view_cams = [(np.eye(3), np.zeros(3)), (R[2], d[2]), (A1, b1), (A2, b2)]
    obs = [xy1[2][0], xy2[2][0], xy1[1][0], xy1[0][0]]
    X = lms[2][1][0].copy()
    for _ in range(6):  # plain Gauss-Newton with numpy's solver
        J, r = [], []
        for (A, b), o in zip(view_cams, obs):
            P = A @ X + b
            nu, nv = (np.float64(o[0]) - K[0, 2]) / K[0, 0], (np.float64(o[1]) - K[1, 2]) / K[1, 1]
            J += [(A[0] - P[0] / P[2] * A[2]) / P[2], (A[1] - P[1] / P[2] * A[2]) / P[2]]
            r += [P[0] / P[2] - nu, P[1] / P[2] - nv]
        J, r = np.array(J), np.array(r)
        X = X + np.linalg.solve(J.T @ J, -J.T @ r)
    got = refined[2][0]
    np.testing.assert_allclose([got["X"], got["Y"], got["Z"]], X, rtol=1e-9)
    assert got["iters"] == 6 and got["n_used"] == 4 and got["n_inliers"] == 4 and got["rms"] < 0.01
    # and the window camera of frame 0 is where the scene puts it: camera 0 from camera 2, baseline-2 units
    C2 = cams[2]
    np.testing.assert_allclose(A2, C2[0].T, atol=1e-12)
    np.testing.assert_allclose(b2, -C2[0].T @ C2[1] / base[2], rtol=1e-5, atol=1e-7)
    win = rc.window(2, *rc.unit_motions(recs, scales), [2, 2, 2], 6)
    np.testing.assert_allclose(win[1][0], A2, atol=1e-15)
    np.testing.assert_allclose(win[1][1], b2, atol=1e-15)


# ---- ids ---------------------------------------------------------------------------------------
def _forward_ids(links):
    """Track ids by carrying each root forward, pair after pair."""
    out, prev = [], None
    for p, link in enumerate(links):
        cur = [(p, o, 0) if l < 0 else (prev[l][0], prev[l][1], prev[l][2] + 1) for o, l in enumerate(link)]
        out.append(cur)
        prev = cur
    return out


def _jumping_ids(links):
    """The kernel's list ranking: launch 0 turns a link into (age, ordinal), launch r joins every
    landmark with the state its ancestor had after launch r - 1; rounds from the pair count alone."""
    P = len(links)
    state = [[(1, int(l)) if l >= 0 else (0, o) for o, l in enumerate(link)] for link in links]
    rounds = 0
    while (1 << rounds) < P - 1:
        rounds += 1
    for _ in range(rounds):
        state = [[(a + state[p - a][o][0], state[p - a][o][1]) if a else (a, o) for a, o in row]
                 for p, row in enumerate(state)]
    return [[(p - a, o, a) for a, o in row] for p, row in enumerate(state)], rounds + 1


@pytest.mark.parametrize("pairs", (1, 2, 3, 4, 5, 8, 9, 16, 17, 33))
def test_ids_against_other_rankings(pairs):
    r0 = np.random.RandomState(100 + pairs)
    spec = [(60, 50, 0)] + [(60, 50, int(r0.randint(5, 30))) for _ in range(pairs - 1)]
    land, matches = rc.persistent_indices(spec, 256, seed=pairs, dups=3, max_age=None if pairs % 2 else max(pairs - 2, 1))
    lms = [(l, np.ones((len(l), 3))) for l in land]
    links, _ = tc.reference(lms, matches, np.zeros(pairs, pc.PAIR_RECORD_DTYPE))
    ids = rc.ids_reference(links)
    want = _forward_ids(links)
    jump, launches = _jumping_ids(links)
    assert launches <= 1 + int(np.ceil(np.log2(pairs))) if pairs > 1 else launches == 1
    for p in range(pairs):
        got = [(int(i["root_pair"]), int(i["root_ord"]), int(i["age"])) for i in ids[p]]
        assert got == want[p] == jump[p], p
        assert not ids[p]["reserved"].any()
    if pairs >= 3:
        assert max(int(i["age"].max()) for i in ids) >= min(pairs - 2, 8)


# ---- the float64 anchor of the formulas ----------------------------------------------------------
@pytest.mark.parametrize("views", (3, 6, 8))
@pytest.mark.parametrize("with_poses", (False, True))
def test_true_motions_return_the_true_point(views, with_poses):
    """True records, true ratios, noiseless observations, a start pushed off by up to 3 %: the true
    point to 1e-9 relative.  The observations are doubles (normalise64): rounding a pixel to
    float32 alone moves a point at these depths by 1e-6 of its depth, which would hide an error in
    the unit chain, a transpose or the view order three orders of magnitude larger than this bound
    admits.  With poses the records are turned by 0.05 rad and the true motions come in as poses."""
    from droplet_visual_odometry_amd._native import TRACK_POSE_DTYPE
    spec = [(120, 100, 0)] + [(120, 100, 80)] * 9
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 1024, seed=3, f64=True)
    links, scales = tc.reference(lms, matches, recs)
    scales = scales.copy()
    scales["ratio"][1:] = base[1:] / base[:-1]
    poses = None
    if with_poses:
        poses = np.zeros(len(lms), TRACK_POSE_DTYPE)
        poses["status"] = pc.OK
        poses["status"][[0, 4]] = pc.NONE  # these two fall back to the records, which stay true
        r = np.random.RandomState(9)
        for p in range(len(lms)):
            poses[p]["R"], poses[p]["scale"] = recs[p]["R"], scales[p]["ratio"]
            poses[p]["t"] = recs[p]["t"] * scales[p]["ratio"]
            if poses[p]["status"] == pc.OK:
                recs[p]["R"] = (pc.small_rotation(r, 0.05) @ recs[p]["R"].reshape(3, 3)).reshape(9)
                scales[p]["ratio"] *= 1.3
    r = np.random.RandomState(1)
    pushed = [(a, x * (1 + r.uniform(-0.03, 0.03, (len(x), 1)))) for a, x in lms]
    refined, info = rc.refine_reference(pushed, xy1, xy2, matches, links, recs, scales, K, views=views, iters=8,
                                        poses=poses, normalise=rc.normalise64)
    assert info["views"][views] >= 80 and not info["views"][views + 1:].any()
    worst, n = 0.0, 0
    for p in range(len(lms)):
        on = np.flatnonzero(refined[p]["status"] == rc.OK)
        assert len(on) == (refined[p]["views"] >= 3).sum()
        X = np.stack([refined[p]["X"], refined[p]["Y"], refined[p]["Z"]], 1)[on]
        if len(on):
            worst = max(worst, (np.linalg.norm(X - truth[p][on], axis=1) / np.linalg.norm(truth[p][on], axis=1)).max())
            n += len(on)
            assert (refined[p]["rms"][on] < 1e-6).all() and (refined[p]["n_inliers"][on] == refined[p]["views"][on]).all()
    print("views", views, "poses", with_poses, "landmarks", n, "worst relative distance", worst)
    assert n >= 700 and worst <= 1e-9


# ---- accuracy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("views", rc.ACC_VIEWS)
def test_refined_is_closer_than_the_two_view_point(views):
    """True records, DLT starts, 0.3 px of noise: the median distance to the truth over the
    landmarks with a full window is strictly below the raw median.  The other two legs (records
    turned by 0.01 rad, without and with the refined poses) are printed, not asserted."""
    n, raw_med, raw_p90, ref_med, ref_p90 = rc.accuracy(views, "true")
    print("true", views, n, raw_med, raw_p90, ref_med, ref_p90)
    assert n >= 300 and ref_med < raw_med
    np.testing.assert_allclose((n, raw_med, raw_p90, ref_med, ref_p90), rc.ACCURACY[("true", views)], rtol=2e-3)
    for leg in ("rot", "poses"):
        got = rc.accuracy(views, leg)
        print(leg, views, *got)
        np.testing.assert_allclose(got, rc.ACCURACY[(leg, views)], rtol=2e-3)
        assert ((leg, views) in rc.WORSE) == (got[3] >= got[1])


# ---- degenerate inputs -------------------------------------------------------------------------
def test_one_ray_is_degenerate_with_no_step_taken():
    lms, xy1, xy2, matches, recs = rc.one_ray(4, 3)
    *_, refined, ids, info = rc.reference(lms, xy1, xy2, matches, recs, K)
    assert (refined[0]["status"] == rc.NONE).all()
    for p in (1, 2):
        x = refined[p]
        assert (x["status"] == rc.DEGENERATE).all() and (x["iters"] == 0).all() and (x["views"] == p + 2).all()
        assert (x["X"] == 0).all() and (x["Y"] == 0).all() and (x["Z"] == 5.0).all()
        assert (x["n_used"] == p + 2).all() and (x["n_inliers"] == p + 2).all() and (x["rms"] == 0).all()


def test_a_view_behind_the_camera_contributes_nothing():
    spec = [(60, 50, 0)] + [(60, 50, 40)] * 3
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 256, seed=4, noise=0.3, behind=10)
    *_, refined, ids, info = rc.reference(lms, xy1, xy2, matches, recs, K)
    seen = 0
    for p in range(1, 4):
        x = refined[p]
        mirrored = (lms[p][1][:, 2] < 0) & (x["views"] >= 3)
        seen += int(mirrored.sum())
        assert (x["n_used"][mirrored] < x["views"][mirrored]).all()  # view 0 at the least sees it behind
        assert (x["n_used"][~mirrored & (x["views"] >= 3)] == x["views"][~mirrored & (x["views"] >= 3)]).all()
    assert seen >= 5


def test_huber_infinity_weights_every_view_one():
    spec = [(60, 50, 0)] + [(60, 50, 40)] * 3
    case = rc.scene_chain(spec, 256, seed=5, noise=0.3, outliers=0.2, dlt=True)
    *_, info = rc.reference(*case[:5], K)
    assert info["quad"] > 0 and info["lin"] > 0
    *_, ref_inf, _, info = rc.reference(*case[:5], K, huber_px=np.inf)
    assert info["lin"] == 0 and info["quad"] > 0
    assert all(np.isfinite(x["X"]).all() for x in ref_inf)
