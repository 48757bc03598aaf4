"""Track poses without a GPU: the ABI's struct and the numpy dtype agree, both sides name the new
entry points, carry_scale takes the refined scale where there is one, the numpy restatement the
GPU tests compare against (track_pose_cases) does what the header says on a case small enough to
write out, keeps the header's sum order, reports the degenerate inputs, and on the three-view scene
through the CPU oracle the refined scale is closer to the true baseline ratio than the ratio."""
import os
import re

import numpy as np
import pytest

import track_cases as tc
import track_pose_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dvo_stream_set_track_poses", "dvo_knn_stream_set_track_poses", "dvo_test_track_poses")
C_TYPES = {"int32_t": ("<i4", 4), "float": ("<f4", 4), "double": ("<f8", 8)}


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_struct_and_dtype_agree():
    from droplet_visual_odometry_amd import _native
    dt = _native.TRACK_POSE_DTYPE
    body = re.search(r"typedef struct \{([^}]*)\} dvo_track_pose;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        code, size = C_TYPES[ctype]
        for name in (n.strip() for n in names.split(",")):
            count = 1
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            if arr:
                name, count = arr.group(1), int(arr.group(2))
            off = (off + size - 1) // size * size
            fields.append((name, code, off, count))
            off += size * count
    assert (off + 7) // 8 * 8 == dt.itemsize == 128
    assert [f[0] for f in fields] == list(dt.names)
    for name, code, o, count in fields:
        assert dt.fields[name][0].base == np.dtype(code), name
        assert dt.fields[name][0].shape == (() if count == 1 else (count,)), name
        assert dt.fields[name][1] == o, name
    h = _header()
    for name, value in (("OK", 0), ("NONE", 1), ("DEGENERATE", 2)):
        assert re.search(r"#define DVO_TRACK_POSE_%s %d\b" % (name, value), h)
        assert getattr(_native, "TRACK_POSE_" + name) == getattr(pc, name) == value


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


def test_python_surface():
    import inspect
    from droplet_visual_odometry_amd import ops, stream
    for cls in (stream.FrameStream, stream.KnnFrameStream):
        sig = inspect.signature(cls.bind_track_poses)
        got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
        assert got == dict(iters=10, huber_px=1.0, inlier_px=2.0, min_points=6)
    assert callable(stream.TrackPoses) and callable(ops.test_track_poses)
    assert "poses" in inspect.signature(stream.carry_scale).parameters


def _scales(ratio, n_common):
    from droplet_visual_odometry_amd._native import TRACK_SCALE_DTYPE
    s = np.zeros(len(ratio), TRACK_SCALE_DTYPE)
    s["ratio"], s["n_common"] = ratio, n_common
    return s


def test_carry_scale_with_poses():
    from droplet_visual_odometry_amd._native import TRACK_POSE_DTYPE
    from droplet_visual_odometry_amd.stream import carry_scale
    nan = np.nan
    s = _scales([0.0, 2.0, 0.5, 0.0, 3.0, 1.5, 4.0], [-1, 5, 1, 0, 7, 2, 3])
    po = np.zeros(7, TRACK_POSE_DTYPE)
    po["scale"] = [0.0, 2.25, 0.5, 0.0, 3.5, 9.0, 4.5]
    po["status"] = [1, 0, 1, 1, 0, 2, 0]
    anchor = [2.0, nan, nan, 7.0, nan, nan, nan]
    # status 0 takes the refined scale; NONE (pair 2) and DEGENERATE (pair 5) fall back to the ratio
    out = carry_scale(anchor, s, po)
    np.testing.assert_array_equal(out, [2.0, 2.0 * 2.25, 2.0 * 2.25 * 0.5, 7.0, 7.0 * 3.5, 7.0 * 3.5 * 1.5,
                                        7.0 * 3.5 * 1.5 * 4.5])
    # the chain still breaks where no point is shared, whatever the pose says
    po2 = po.copy()
    po2["status"][3] = 0
    assert np.isnan(carry_scale([1.0, nan, nan, nan, nan, nan, nan], s, po2)[3:]).all()
    # without poses: the old results to the bit
    old = carry_scale(anchor, s)
    np.testing.assert_array_equal(old, [2.0, 2.0 * 2.0, 2.0 * 2.0 * 0.5, 7.0, 7.0 * 3.0, 7.0 * 3.0 * 1.5,
                                        7.0 * 3.0 * 1.5 * 4.0])
    assert carry_scale(anchor, s, None).tobytes() == old.tobytes()
    with pytest.raises(ValueError):
        carry_scale(anchor, s, po[:3])


def test_restatement_written_out():
    """Identity pose, three points seen exactly where they project: every residual is 0, so g is 0,
    d is 0, the Cayley map is the identity and every step returns the start pose; rms is 0."""
    K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
    Y = np.array([[1.0, 0.5, 4.0], [-1.0, 1.0, 2.0], [0.5, -0.25, 8.0]])
    nu, nv = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]  # exact quotients, as P0 * (1 / P2) gives them here
    for k in range(3):
        assert nu[k] == Y[k, 0] * (1.0 / Y[k, 2]) and nv[k] == Y[k, 1] * (1.0 / Y[k, 2])
    r = pc.refine(Y, nu, nv, np.eye(3), np.zeros(3), K, iters=10)
    assert r["status"] == pc.OK and r["iters"] == 10
    np.testing.assert_array_equal(r["R"], np.eye(3))
    np.testing.assert_array_equal(r["t"], np.zeros(3))
    assert r["rms"] == 0.0 and r["scale"] == 0.0 and r["n_used"] == r["n_inliers"] == 3
    assert r["quad"] == 30 and r["lin"] == 0
    # the sums of that step by hand: H's diagonal entry of the z translation is sum of b^2 + c^2
    S, _, _ = pc.step_sums(Y, nu, nv, np.eye(3), np.zeros(3), 1.0 / 500.0)
    a = 1.0 / Y[:, 2]
    b, c = -(nu * a), -(nv * a)
    assert S[20] == ((b * b + c * c)[0] + (b * b + c * c)[1]) + (b * b + c * c)[2]
    assert (S[21:] == 0).all()
    # one point moved by a pixel: the fit leaves the identity and pulls the residual down
    nu2 = nu.copy()
    nu2[0] += 1.0 / 500.0
    r2 = pc.refine(Y, nu2, nv, np.eye(3), np.zeros(3), K, iters=10)
    assert r2["status"] == pc.OK and not np.array_equal(r2["R"], np.eye(3)) and r2["rms"] < 1e-6
    assert np.abs(r2["R"] @ r2["R"].T - np.eye(3)).max() < 1e-14  # the Cayley map keeps R a rotation


def test_sum_order():
    """The stated order is not the only one: np.sum differs in the last bit for some seeded input,
    and tree_sum is the header's: lane sums, the halving tree inside 64 lanes, then four groups."""
    r = np.random.RandomState(5)
    T = r.normal(size=(1000, 27)) * 10.0 ** r.uniform(-3, 3, (1000, 1))
    got = pc.tree_sum(T)
    other = T.sum(0)
    assert np.allclose(got, other, rtol=1e-9, atol=1e-9) and (got != other).any()
    q = 11
    lanes = np.zeros(256)
    for k in range(1000):  # ascending k per lane
        lanes[k % 256] = lanes[k % 256] + T[k, q]
    groups = []
    for g0 in range(0, 256, 64):
        v = lanes[g0:g0 + 64].copy()
        for s in (32, 16, 8, 4, 2, 1):
            for lane in range(s):
                v[lane] = v[lane] + v[lane + s]
        groups.append(v[0])
    assert got[q] == ((groups[0] + groups[1]) + groups[2]) + groups[3]
    alone = np.array([pc.tree_sum(T[:, [j]])[0] for j in range(27)])
    assert (alone == got).all()  # a column alone sums as it does beside the others


def test_degenerate_inputs():
    # eight identical points seen at one pixel: rank 2, DEGENERATE with no step taken, the start pose kept
    lms, xy2, matches, recs = pc.identical_points(8)
    _, sc, po, _ = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN)
    assert sc[1]["n_common"] == 8 and sc[1]["ratio"] == 1.0
    assert po[1]["status"] == pc.DEGENERATE and po[1]["iters"] == 0
    np.testing.assert_array_equal(po[1]["R"], np.eye(3).reshape(9))
    np.testing.assert_array_equal(po[1]["t"], [1.0, 0.0, 0.0])
    assert po[1]["scale"] == 1.0 and po[1]["n_used"] == 8
    # n < min_points: NONE with the start values; pair 0: NONE and all zero
    lms, xy2, matches, recs, _ = pc.chain([(40, 30, 0), (40, 30, 5), (40, 30, 6), (40, 30, 0)], 200, seed=3)
    _, sc, po, info = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN)
    assert list(po["status"]) == [pc.NONE, pc.NONE, pc.OK, pc.NONE] and list(po["iters"]) == [0, 0, 10, 0]
    assert not po[0]["R"].any() and po[0]["scale"] == 0 and not po[3]["R"].any() and not po[3]["t"].any()
    np.testing.assert_array_equal(po[1]["R"], recs[1]["R"])
    np.testing.assert_array_equal(po[1]["t"], sc[1]["ratio"] * recs[1]["t"])
    assert po[1]["scale"] > 0 and po[1]["rms"] == 0 and po[1]["n_used"] == 0 and info[1] is None
    _, _, po3, _ = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN, min_points=3)
    assert list(po3["status"]) == [pc.NONE, pc.OK, pc.OK, pc.NONE]


def test_chain_is_consistent():
    """The generator's chains: sizes as asked.  With true records and exact pixels the refined
    scale is the ratio of the true baselines (float32 pixels round by 3e-5 px at most).  Turning
    pair p - 1's R and t moves Y rigidly, so a pose that explains every point still exists (its
    translation is another one: no bound on the scale then) and the steps find it from pair p's
    turned record: the rms falls to the pixels' rounding."""
    spec = [(300, 200, 0), (300, 260, 63), (280, 0, 0), (300, 262, 0), (300, 256, 255)]
    for sigma in (0.0, 0.01):
        lms, xy2, matches, recs, base = pc.chain(spec, kp_cap=900, seed=5, rot_sigma=sigma)
        _, sc, po, info = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN)
        assert list(sc["n_common"]) == [-1, 63, 0, 0, 255]
        assert list(po["status"]) == [pc.NONE, pc.OK, pc.NONE, pc.NONE, pc.OK]
        for p in (1, 4):
            true = base[p] / base[p - 1]
            print("sigma", sigma, "pair", p, "ratio dev %.3e" % (sc[p]["ratio"] / true - 1),
                  "scale dev %.3e" % (po[p]["scale"] / true - 1), "rms %.3e" % po[p]["rms"])
            assert po[p]["rms"] < 1e-3
            assert po[p]["n_used"] == po[p]["n_inliers"] == sc[p]["n_common"]
            if sigma == 0:
                assert abs(po[p]["scale"] / true - 1) < 1e-5
            else:  # the steps had work to do
                assert np.abs(info[p]["R"].reshape(9) - recs[p]["R"]).max() > 1e-3
    # gross outliers take the linear Huber branch and are not inliers at the end
    lms, xy2, matches, recs, base = pc.chain([(300, 280, 0), (300, 280, 200)], 900, seed=6, noise=0.3, outliers=0.2)
    _, sc, po, info = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN)
    assert info[1]["quad"] > 0 and info[1]["lin"] > 0 and 100 < po[1]["n_inliers"] < 190
    assert abs(po[1]["scale"] / (base[1] / base[0]) - 1) < 0.05


def test_scene_scale_beats_the_ratio(oracle_mod):
    """The three-view scene through the CPU oracle: with 0.3 px of noise the refined scale is closer
    to the true baseline ratio than the median ratio at every size; without noise it stays within 4x
    the largest deviation recorded in track_pose_cases.NOISELESS_DEV; six points share three: NONE."""
    true = tc.T_B / tc.T_A
    for m in pc.NOISY_SIZES:
        sc, po, _ = pc.scene_reference(oracle_mod, m, 0.3)
        ratio_dev, dev = sc[1]["ratio"] / true - 1, po[1]["scale"] / true - 1
        print("noise 0.3 m", m, "n", sc[1]["n_common"], "ratio dev %.3e scale dev %.3e" % (ratio_dev, dev),
              "inliers", po[1]["n_inliers"], "rms %.3f" % po[1]["rms"])
        assert po[1]["status"] == pc.OK and po[1]["iters"] == 10
        assert abs(dev) < abs(ratio_dev), (m, dev, ratio_dev)
    for m in pc.SCENE_SIZES:
        sc, po, _ = pc.scene_reference(oracle_mod, m)
        dev = po[1]["scale"] / true - 1
        print("noiseless m", m, "n", sc[1]["n_common"], "ratio dev %.3e scale dev %.3e" % (sc[1]["ratio"] / true - 1, dev),
              "rms %.3e" % po[1]["rms"])
        assert po[1]["status"] == pc.OK and po[0]["status"] == pc.NONE
        assert abs(dev) <= pc.SCENE_BOUND, (m, dev)
    sc, po, _ = pc.scene_reference(oracle_mod, 6)
    assert sc[1]["n_common"] == 3 and po[1]["status"] == pc.NONE and po[1]["iters"] == 0
