"""Track bundle without a GPU: the ABI's struct and the numpy dtype agree, both sides name the new
entry points, bind_bundle and carry_scale(bundle=) follow their rules, and the numpy restatement
the GPU tests compare against (track_bundle_cases) does what the header says: its Schur step
against a plain dense Gauss-Newton step, as a float64 anchor of the formulas (noiseless
observations return the true cameras and points), on the accuracy it is for, on the guard and on
the degenerate inputs."""
import os
import re
import types

import numpy as np
import pytest

import track_bundle_cases as bc
import track_cases as tc
import track_pose_cases as pc
import track_refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dvo_stream_set_track_bundle", "dvo_knn_stream_set_track_bundle", "dvo_test_track_bundle")
C_TYPES = {"int32_t": ("<i4", 4), "float": ("<f4", 4), "double": ("<f8", 8)}
K = pc.K_CHAIN


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_struct_and_dtype_agree():
    from droplet_visual_odometry_amd import _native
    dt = _native.TRACK_BUNDLE_DTYPE
    body = re.search(r"typedef struct \{([^}]*)\} dvo_track_bundle;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        code, sz = C_TYPES[ctype]
        for name in (n.strip() for n in names.split(",")):
            dims = re.search(r"\[(\d+)\]", name)
            count = int(dims.group(1)) if dims else 1
            off = (off + sz - 1) // sz * sz
            fields.append((name.split("[")[0], code, off, count))
            off += sz * count
    assert off == dt.itemsize == 160
    assert [f[0] for f in fields] == list(dt.names)
    for name, code, o, count in fields:
        assert dt.fields[name][0].base == np.dtype(code) and dt.fields[name][1] == o, name
        assert dt.fields[name][0].shape == ((count,) if count > 1 else ()), name
    h = _header()
    assert "sizeof(dvo_track_bundle) == 160" in h
    for name, value in (("OK", 0), ("NONE", 1), ("DEGENERATE", 2), ("NOT_IMPROVED", 3)):
        assert re.search(r"#define DVO_TRACK_BUNDLE_%s %d\b" % (name, value), h)
        assert getattr(_native, "TRACK_BUNDLE_" + name) == getattr(bc, name) == value
    assert float(re.search(r"#define DVO_TRACK_BUNDLE_LAMBDA (\S+)", h).group(1)) == bc.LAMBDA


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
        sig = inspect.signature(cls.bind_bundle)
        got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
        assert got == dict(views=6, iters=5, lam=0.0, huber_px=1.0, inlier_px=2.0, min_points=8, pairs=True, points=True)
    assert callable(ops.test_track_bundle)
    for bad in ((0, 4), (2, 0)):
        with pytest.raises(ValueError):
            stream.TrackBundle(*bad, "cpu")
    bd = stream.TrackBundle(3, 5, "cpu")
    assert bd.bundle.shape == (3, 160) and bd.points.shape == (3, 5, 56)
    assert bd.numpy().shape == (3,) and bd.numpy().dtype.names[:3] == ("R", "t", "ratio")
    assert bd.points_numpy(1, 9).shape == (5,) and bd.points_numpy(2, 2).shape == (2,)
    # the wrapper's own checks: the bundle goes after tracks, with the bound Landmarks' cap and pairs
    calls = []
    dev = torch.device("cpu")
    fake = types.SimpleNamespace(h=None, device=dev, _after_torch=lambda: None, _lm_next=None, _tr_next=None,
                                 ctx=types.SimpleNamespace(check=lambda rc_: None))

    def setter(*a):
        calls.append(a)
        return 0

    args = (6, 5, 0.0, 1.0, 2.0, 8, True, True)
    with pytest.raises(ValueError):
        stream._bind_bundle(fake, setter, bd, *args)
    fake._lm_next = stream.Landmarks(3, 5, "cpu")
    with pytest.raises(ValueError):
        stream._bind_bundle(fake, setter, bd, *args)
    fake._tr_next = stream.Tracks(3, 5, "cpu")
    for wrong in (stream.TrackBundle(3, 4, "cpu"), stream.TrackBundle(2, 5, "cpu"), object()):
        with pytest.raises(ValueError):
            stream._bind_bundle(fake, setter, wrong, *args)
    assert not calls
    assert stream._bind_bundle(fake, setter, bd, 4, 2, 1e-3, 0.5, 3.0, 9, True, False) is bd
    assert calls[-1] == (None, bd.bundle.data_ptr(), None, 4, 2, 1e-3, 0.5, 3.0, 9)
    assert stream._bind_bundle(fake, setter, bd, 4, 2, 1e-3, 0.5, 3.0, 9, False, True) is bd
    assert calls[-1][1:3] == (None, bd.points.data_ptr())
    assert stream._bind_bundle(fake, setter, None, *args) is None
    assert calls[-1] == (None, None, None, 0, 0, 0.0, 0.0, 0.0, 0)
    assert stream._bind_bundle(fake, setter, bd, 6, 5, 0.0, 1.0, 2.0, 8, False, False) is None  # neither output: a clear
    assert bc.defaults(0, -1, 0.0, 0.0, -2.0, 0) == (6, 5, bc.LAMBDA, 1.0, 2.0, 8)
    assert bc.defaults(8, 16, 1e-2, np.inf, 3.0, 6) == (8, 16, 1e-2, np.inf, 3.0, 6)


def _scales(ratio, n_common):
    from droplet_visual_odometry_amd._native import TRACK_SCALE_DTYPE
    s = np.zeros(len(ratio), TRACK_SCALE_DTYPE)
    s["ratio"], s["n_common"] = ratio, n_common
    return s


def test_carry_scale_with_bundle():
    from droplet_visual_odometry_amd._native import TRACK_BUNDLE_DTYPE, TRACK_POSE_DTYPE
    from droplet_visual_odometry_amd.stream import carry_scale
    nan = np.nan
    s = _scales([0.0, 2.0, 0.5, 0.0, 3.0, 1.5, 4.0], [-1, 5, 1, 0, 7, 2, 3])
    po = np.zeros(7, TRACK_POSE_DTYPE)
    po["scale"] = [0.0, 2.25, 0.5, 0.0, 3.5, 9.0, 4.5]
    po["status"] = [1, 0, 1, 1, 0, 2, 0]
    bd = np.zeros(7, TRACK_BUNDLE_DTYPE)
    bd["ratio"] = [0.0, 2.125, 0.625, 0.0, 0.0, 1.75, 4.25]
    bd["status"] = [0, 0, 3, 1, 0, 0, 2]
    anchor = [2.0, nan, nan, 7.0, nan, nan, nan]
    # OK with a ratio > 0 takes the bundle's; NOT_IMPROVED (2), a two-camera fit's 0.0 (4) and
    # DEGENERATE (6) fall back to the pose's scale or the median ratio
    out = carry_scale(anchor, s, po, bd)
    np.testing.assert_array_equal(out, [2.0, 2.0 * 2.125, 2.0 * 2.125 * 0.5, 7.0, 7.0 * 3.5, 7.0 * 3.5 * 1.75,
                                        7.0 * 3.5 * 1.75 * 4.5])
    out = carry_scale(anchor, s, bundle=bd)
    np.testing.assert_array_equal(out, [2.0, 2.0 * 2.125, 2.0 * 2.125 * 0.5, 7.0, 7.0 * 3.0, 7.0 * 3.0 * 1.75,
                                        7.0 * 3.0 * 1.75 * 4.0])
    # the chain still breaks where no point is shared, whatever the bundle says
    bd2 = bd.copy()
    bd2["status"][3], bd2["ratio"][3] = 0, 1.5
    assert np.isnan(carry_scale([1.0, nan, nan, nan, nan, nan, nan], s, po, bd2)[3:]).all()
    # bundle=None: today's results to the bit, on the cases of test_tracks_host.py and test_track_poses_host.py
    for a in ([nan, nan, 0.8, nan, nan, 0.25, nan], anchor):
        assert carry_scale(a, s, None, None).tobytes() == carry_scale(a, s).tobytes()
        assert carry_scale(a, s, po, None).tobytes() == carry_scale(a, s, po).tobytes()
    np.testing.assert_array_equal(carry_scale([nan, nan, 0.8, nan, nan, 0.25, nan], s), [nan, nan, 0.8, nan, nan, 0.25, 1.0])
    np.testing.assert_array_equal(carry_scale(anchor, s), [2.0, 4.0, 2.0, 7.0, 21.0, 31.5, 126.0])
    np.testing.assert_array_equal(carry_scale(anchor, s, po), [2.0, 2.0 * 2.25, 2.0 * 2.25 * 0.5, 7.0, 7.0 * 3.5,
                                                               7.0 * 3.5 * 1.5, 7.0 * 3.5 * 1.5 * 4.5])
    with pytest.raises(ValueError):
        carry_scale(anchor, s, po, bd[:3])


# ---- the Schur step against the unreduced normal equations --------------------------------------
# max |difference| / max |step| between track_bundle_cases.step and dense_step (numpy's solver on
# the full system with the same damping) over the three pairs of the scene below, measured here:
# (cameras, points).  The system's condition grows as 1 / lambda along the free scale, and so does
# the difference; the assertion is at 4 x the recorded figure.
DENSE_DEV = {1e-6: (3.06e-11, 3.28e-11), 1e-2: (3.15e-14, 5.58e-14)}


@pytest.mark.parametrize("lam", sorted(DENSE_DEV))
def test_schur_step_equals_dense_gauss_newton(lam):
    spec = [(60, 50, 0)] + [(60, 50, 40)] * 2
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 256, seed=7, noise=0.3, rot_sigma=0.003, dlt=True)
    links, scales = tc.reference(lms, matches, recs)
    R, d, rho = rc.unit_motions(recs, scales)
    counts = [len(a[0]) for a in lms]
    kh = 1.0 / ((K[0, 0] + K[1, 1]) / 2)
    worst = [0.0, 0.0]
    for p in range(3):
        win = rc.window(p, R, d, rho, counts, 6)
        cams = [(np.eye(3), np.zeros(3)), (R[p], d[p])] + win
        assert len(cams) == p + 2
        nu, nv, nviews = bc.gather(p, lms, xy1, xy2, links, win, K, pc.normalise)
        X = np.asarray(lms[p][1], np.float64)
        new, Xn, good, _ = bc.step(cams, X, nu, nv, nviews, kh, lam)
        assert good.all()
        Vd, g, W, Ut, ht, _ = bc.linearise(cams, X, nu, nv, nviews, kh, lam)
        S, rr, *_ = bc.reduced_system(Vd, g, W, Ut, ht, nviews, len(cams), lam)
        dc = bc.ldl_solve(S, rr)
        dd, dx = bc.dense_step(cams, X, nu, nv, nviews, kh, lam)
        worst[0] = max(worst[0], np.abs(dc - dd).max() / np.abs(dd).max())
        worst[1] = max(worst[1], np.abs((Xn - X) - dx).max() / np.abs(dx).max())
        for c in range(1, len(cams)):  # and the cameras moved by that step
            A, b = pc.cayley_update(cams[c][0], cams[c][1], dc[6 * (c - 1):6 * c])
            assert np.array_equal(A, new[c][0]) and np.array_equal(b, new[c][1])
    print("lambda", lam, "cameras %.3g points %.3g" % tuple(worst))
    assert worst[0] <= 4 * DENSE_DEV[lam][0] and worst[1] <= 4 * DENSE_DEV[lam][1]


# ---- the float64 anchor of the formulas ----------------------------------------------------------
@pytest.mark.parametrize("views", (2, 3, 6, 8))
def test_noiseless_observations_return_the_truth(views):
    """True motions turned by 0.002 rad, noiseless double observations (normalise64), points pushed
    off by up to 3 %, 16 steps at the default damping: the true points and the true motion of the
    pair come back.  The assertion is at 4 x the largest deviation recorded in
    track_bundle_cases.ANCHOR_DEV."""
    spec = [(120, 100, 0)] + [(120, 100, 80)] * 9
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 1024, seed=3, rot_sigma=0.002, push=0.03, f64=True)
    links, scales = tc.reference(lms, matches, recs)
    true = rc.scene_chain(spec, 1024, seed=3, f64=True)[4]  # the records before they were turned
    bundle, points, info = bc.bundle_reference(lms, xy1, xy2, matches, links, recs, scales, K, views=views, iters=16,
                                               normalise=rc.normalise64)
    assert (bundle["status"] == bc.OK).all() and (bundle["iters"] == 16).all()
    assert list(bundle["n_cams"]) == [min(views, p + 2) for p in range(10)]
    worst = cam = ratio = 0.0
    for p in range(10):
        X = np.stack([points[p][f] for f in "XYZ"], 1)
        worst = max(worst, (np.linalg.norm(X - truth[p], axis=1) / np.linalg.norm(truth[p], axis=1)).max())
        cam = max(cam, np.abs(bundle[p]["R"] - true[p]["R"]).max(), np.abs(bundle[p]["t"] - true[p]["t"]).max())
        if bundle[p]["n_cams"] >= 3:
            ratio = max(ratio, abs(bundle[p]["ratio"] / (base[p] / base[p - 1]) - 1))
        assert (points[p]["status"] == rc.OK).all() and (points[p]["n_inliers"] == points[p]["views"]).all()
    print("views", views, "worst relative distance %.3e camera %.3e ratio %.3e" % (worst, cam, ratio))
    bound = 4 * max(bc.ANCHOR_DEV.values())
    assert worst <= bound and cam <= bound and ratio <= bound
    assert (bundle["rms"] < 1e-9).all() and (bundle["cost"] < 1e-24).all()


# ---- accuracy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("views", rc.ACC_VIEWS)
def test_bundled_is_closer_than_raw_and_refined(views):
    """track_refine_cases.ACC_SPEC with 0.3 px of noise.  Leg "true": the bundled points' median
    distance to the truth is strictly below the raw median.  Leg "rot" (records turned by 0.01 rad):
    strictly below both the raw and the refined median wherever WORSE does not list the size, and 8
    views may not be listed."""
    n, raw, ref, bun, p90, status = bc.bundle_accuracy(views, "true")
    print("true", views, n, raw, ref, bun, p90, status)
    assert n >= 300 and bun < raw
    np.testing.assert_allclose((n, raw, ref, bun, p90), bc.ACCURACY[("true", views)], rtol=2e-3)
    n, raw, ref, bun, p90, status = bc.bundle_accuracy(views, "rot")
    print("rot", views, n, raw, ref, bun, p90, status)
    np.testing.assert_allclose((n, raw, ref, bun, p90), bc.ACCURACY[("rot", views)], rtol=2e-3)
    assert (("rot", views) in bc.WORSE) == (not (bun < raw and bun < ref))
    assert ("rot", 8) not in bc.WORSE
    assert raw == rc.ACCURACY[("rot", views)][1] or abs(raw / rc.ACCURACY[("rot", views)][1] - 1) < 2e-3


def test_lambda_sweep_is_behind_the_default():
    got = {lam: bc.bundle_accuracy(6, "rot", lam)[3] for lam in (1e-6, 1e-4, 1e-2)}
    print("lambda sweep", got)
    for lam, med in got.items():
        np.testing.assert_allclose(med, bc.LAMBDA_SWEEP[lam][0], rtol=2e-3)
    assert min(got, key=got.get) == bc.LAMBDA


# ---- the guard ---------------------------------------------------------------------------------
def diverging_case():
    """Records turned by 0.4 rad and points pushed off by up to 60 %, fitted with no Huber weight:
    plain Gauss-Newton steps from there raise the cost of some pairs."""
    return rc.scene_chain([(120, 100, 0)] + [(120, 100, 80)] * 3, 400, seed=41, noise=0.3, rot_sigma=0.4, push=0.6)


def test_a_worse_fit_is_not_handed_out():
    lms, xy1, xy2, matches, recs, truth, base = diverging_case()
    links, scales, poses, bundle, points, info = bc.reference(lms, xy1, xy2, matches, recs, K, huber_px=np.inf)
    where = np.flatnonzero(bundle["status"] == bc.NOT_IMPROVED)
    assert len(where) >= 1
    R, d, rho = rc.unit_motions(recs, scales)
    for p in where:  # the start values, byte for byte
        b, x = bundle[p], points[p]
        assert not b["cost"] <= b["cost0"] and b["iters"] == 5
        assert b["R"].tobytes() == R[p].tobytes() and b["t"].tobytes() == d[p].tobytes()
        assert b["ratio"] == (rho[p] if b["n_cams"] >= 3 else 0.0) and b["rms"] == b["rms0"]
        assert np.stack([x["X"], x["Y"], x["Z"]], 1).tobytes() == np.ascontiguousarray(lms[p][1]).tobytes()
        assert (x["status"] == rc.NONE).all() and (x["iters"] == 0).all()
    for p in np.flatnonzero(bundle["status"] == bc.OK):
        assert bundle[p]["cost"] <= bundle[p]["cost0"]
        assert abs(np.linalg.norm(bundle[p]["t"]) - 1) < 1e-15


# ---- degenerate inputs -------------------------------------------------------------------------
def test_one_ray_is_degenerate_with_no_step_taken():
    lms, xy1, xy2, matches, recs = rc.one_ray(8, 3)
    *_, bundle, points, info = bc.reference(lms, xy1, xy2, matches, recs, K)
    assert list(bundle["status"]) == [bc.DEGENERATE] * 3 and list(bundle["iters"]) == [0] * 3
    assert list(bundle["n_cams"]) == [2, 3, 4]
    for p in range(3):
        assert bundle[p]["R"].tobytes() == recs[p]["R"].tobytes() and bundle[p]["t"].tobytes() == recs[p]["t"].tobytes()
        x = points[p]
        assert (x["X"] == 0).all() and (x["Z"] == 5.0).all() and (x["status"] == rc.NONE).all()
        assert (x["n_used"] == p + 2).all() and (x["rms"] == 0).all()


def test_every_view_behind_its_camera():
    """Every landmark mirrored through its camera: no view is used, every V is zero, no landmark
    contributes, the reduced system is zero and its first pivot is not > 0."""
    spec = [(60, 50, 0)] + [(60, 50, 40)] * 2
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 256, seed=4, noise=0.3, behind=50)
    *_, bundle, points, info = bc.reference(lms, xy1, xy2, matches, recs, K)
    assert list(bundle["status"]) == [bc.DEGENERATE] * 3 and not bundle["iters"].any()
    assert not bundle["cost0"].any() and not bundle["n_inliers"].any() and not bundle["rms"].any()
    assert all((x["n_used"][x["views"] == 2] == 0).all() for x in points)


def test_a_window_camera_no_landmark_sees():
    """The window's length comes from the unit motions, not from the chains: where every track ends
    after two links, the cameras further back are seen by no landmark, their blocks of S are zero
    and the pair ends DEGENERATE on its start values.  A caller with short tracks binds fewer views."""
    spec = [(120, 100, 0)] + [(120, 100, 30)] * 6
    case = rc.scene_chain(spec, 400, seed=33, noise=0.3, rot_sigma=0.003, dlt=True, max_age=2)
    *_, bundle, points, info = bc.reference(*case[:5], K, views=6)
    assert list(bundle["status"]) == [bc.OK] * 3 + [bc.DEGENERATE] * 4 and not bundle["iters"][3:].any()
    for p in range(3, 7):
        assert points[p]["views"].max() < bundle[p]["n_cams"]
        assert bundle[p]["R"].tobytes() == case[4][p]["R"].tobytes()
        assert points[p]["X"].tobytes() == np.ascontiguousarray(case[0][p][1][:, 0]).tobytes()
    *_, bundle, points, info = bc.reference(*case[:5], K, views=3)
    assert list(bundle["status"]) == [bc.OK] * 7 and (bundle["iters"] == 5).all()


def test_identical_points():
    """Every landmark of a pair the same point at the same pixels: the cameras' system has rank
    below 6 (Y W^T cancels U), and the pair ends DEGENERATE or keeps a fit that is no worse."""
    n = 8
    recs = np.zeros(2, pc.PAIR_RECORD_DTYPE)
    recs["R"] = np.eye(3).reshape(9)
    recs["n_models"] = 1
    recs["t"] = [1.0, 0.0, 0.0]
    idx = np.arange(n, dtype=np.int32)
    X = np.tile([[0.1, 0.2, 5.0]], (n, 1))
    px1 = np.tile(np.float32([[K[0, 0] * 0.1 / 5 + K[0, 2], K[1, 1] * 0.2 / 5 + K[1, 2]]]), (n, 1))
    px2 = np.tile(np.float32([[K[0, 0] * 1.1 / 5 + K[0, 2], K[1, 1] * 0.2 / 5 + K[1, 2]]]), (n, 1))
    lms = [(idx, X), (idx, X)]
    *_, bundle, points, info = bc.reference(lms, [px1, px1], [px2, px2], [(idx, idx + 100), (idx + 200, idx + 300)], recs, K)
    for p in range(2):
        assert bundle[p]["status"] in (bc.OK, bc.DEGENERATE, bc.NOT_IMPROVED) and bundle[p]["n_cams"] == 2
        assert bundle[p]["status"] != bc.OK or bundle[p]["cost"] <= bundle[p]["cost0"]
        assert np.isfinite(points[p]["X"]).all()


def test_fewer_than_min_points():
    spec = [(60, 50, 0), (60, 7, 5), (60, 8, 5), (60, 0, 0)]
    lms, xy1, xy2, matches, recs, truth, base = rc.scene_chain(spec, 256, seed=6, noise=0.3)
    *_, bundle, points, info = bc.reference(lms, xy1, xy2, matches, recs, K)
    assert list(bundle["status"] == bc.NONE) == [False, True, False, True]
    for p in (1, 3):
        b = bundle[p]
        assert b["R"].tobytes() == recs[p]["R"].tobytes() and b["t"].tobytes() == recs[p]["t"].tobytes()
        assert not any(b[f] for f in ("ratio", "cost0", "cost", "rms0", "rms", "n_points", "n_obs", "n_inliers", "n_cams",
                                      "iters"))
        assert (points[p]["views"] == 2).all() and (points[p]["status"] == rc.NONE).all()
        assert np.stack([points[p][f] for f in "XYZ"], 1).tobytes() == np.ascontiguousarray(lms[p][1], np.float64).tobytes()
    *_, bundle, _, _ = bc.reference(lms, xy1, xy2, matches, recs, K, min_points=6)
    assert list(bundle["status"] == bc.NONE) == [False, False, False, True]
