"""Track PnP on the host: the sample generator and the P3P solver the kernel compiles
(dvo_track_pnp_samples_host, dvo_p3p_host: csrc/p3p.h) against the numpy restatement of the header
(track_pnp_cases.py), the solver's own properties on seeded triples, the restatement end to end on a
noise-free chain with gross outliers, and carry_scale's pnp argument.  No GPU."""
import numpy as np
import pytest

import track_pnp_cases as pn
from droplet_visual_odometry_amd import ops
from droplet_visual_odometry_amd._native import TRACK_PNP_DTYPE, TRACK_POSE_DTYPE, TRACK_SCALE_DTYPE, DVOError
from droplet_visual_odometry_amd.stream import carry_scale

N_TRIPLES = 1000


@pytest.fixture(scope="module")
def solved():
    """The seeded triples with the restatement's and the library's solutions, computed once."""
    out = []
    for Y, nunv, R, t in pn.triples(N_TRIPLES, 1):
        out.append((Y, nunv, R, t, pn.p3p(Y, nunv), ops.p3p(Y, nunv)))
    return out


@pytest.mark.parametrize("n", [3, 4, 5, 64, 1000])
@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_samples_equal_the_restatement(n, seed):
    got = ops.track_pnp_samples(n, 512, seed)
    assert np.array_equal(got, pn.samples(n, 512, seed))
    for hyps in (1, 63, 128):  # a shorter run is a prefix: sample h depends on n, h and the seed only
        assert np.array_equal(ops.track_pnp_samples(n, hyps, seed), got[:hyps])
    void = got[:, 0] < 0
    assert (got[void] == -1).all()
    ok = got[~void]
    assert ((ok >= 0) & (ok < n)).all()
    assert (ok[:, 0] != ok[:, 1]).all() and (ok[:, 0] != ok[:, 2]).all() and (ok[:, 1] != ok[:, 2]).all()
    if n == 3:
        assert void.any() and not void.all()  # 8 draws of 3 values miss one of them about one time in nine
    if n >= 64:
        assert not void.any()


def test_default_seed_is_the_e_ransacs():
    assert np.array_equal(ops.track_pnp_samples(64, 32, 0), ops.track_pnp_samples(64, 32, 2 ** 64 - 1))
    assert not np.array_equal(ops.track_pnp_samples(64, 32, 0), ops.track_pnp_samples(64, 32, 1))


def test_samples_einval():
    for n, hyps in ((0, 1), (-1, 1), (4, 0), (4, 513)):
        with pytest.raises(DVOError):
            ops.track_pnp_samples(n, hyps)


def test_p3p_host_equals_the_restatement(solved):
    for Y, nunv, R, t, (Rs, ts), (Rh, th) in solved:
        assert Rs.shape == Rh.shape and Rs.tobytes() == Rh.tobytes() and ts.tobytes() == th.tobytes()


def test_p3p_solutions_are_poses_of_the_three_points(solved):
    """Every kept solution has an orthonormal R of determinant 1, puts its three points in front of
    the camera and reprojects them onto their rays: 1e-9 in normalised coordinates, the project's
    noise-free tolerance (the depths come out of Newton steps on exactly these three equations)."""
    kept = 0
    for Y, nunv, R, t, _, (Rh, th) in solved:
        assert 0 <= len(Rh) <= 4
        for s in range(len(Rh)):
            kept += 1
            assert np.abs(Rh[s] @ Rh[s].T - np.eye(3)).max() <= 1e-12
            assert abs(np.linalg.det(Rh[s]) - 1) <= 1e-12
            X = Y @ Rh[s].T + th[s]
            assert (X[:, 2] > 0).all()
            assert np.abs(X[:, :2] / X[:, 2:] - nunv).max() <= 1e-9
    assert kept >= N_TRIPLES


def test_true_pose_is_among_the_solutions(solved):
    """At most 1 % of the 1000 seeded triples (depths 2 to 10, an image triangle of at least 2000
    px^2: track_pnp_cases.triples) may have no kept solution within 1e-9 of the true pose.
    Measured with the restatement alone: 0 of 1000 (0.0 %); the library's solutions are the same bits."""
    miss = sum(not pn.pose_error(Rs, ts, R, t) <= 1e-9 for Y, nunv, R, t, (Rs, ts), _ in solved)
    print(f"triples without the true pose within 1e-9: {miss} of {N_TRIPLES}")
    assert miss <= N_TRIPLES // 100


def test_p3p_degenerate_inputs_keep_nothing():
    Y = np.tile([[0.1, 0.2, 5.0]], (3, 1))
    nunv = np.tile([[0.02, 0.04]], (3, 1))
    for Rs, ts in (pn.p3p(Y, nunv), ops.p3p(Y, nunv)):
        assert len(Rs) == 0 and len(ts) == 0


@pytest.fixture(scope="module")
def outlier_chain():
    """Three pairs, 120 correspondences each in pairs 1 and 2, half of them gross outliers, noise-free."""
    c = pn.chain([(200, 130, 0), (200, 130, 60), (200, 130, 60)], [0, 60, 60], 2000, 11, outliers=0.5)
    return c, pn.reference(c["lms"], c["xy2"], c["matches"], c["recs"], pn.K_CHAIN)


def test_restatement_end_to_end(outlier_chain):
    """Noise-free inliers with 50 % outliers displaced by at least 20 px, 128 hypotheses: the chance
    that no sample is clean is (1 - 0.5^3)^128, about 4e-8.  The final inlier mask is the truth set
    exactly and R, t are the truth within 1e-9."""
    c, (pnp, masks, info) = outlier_chain
    assert pnp["status"].tolist() == [pn.NONE, pn.OK, pn.OK]
    assert pnp["n_corr"].tolist() == [0, 120, 120]
    assert not masks[0].any()
    for p in (1, 2):
        R, t, good = c["truth"][p]
        want = np.zeros(len(masks[p]), np.uint8)
        want[good] = 1
        assert len(good) == 60 and np.array_equal(masks[p], want)
        assert pnp["n_inliers"][p] == 60 and pnp["n_best"][p] == 60 and pnp["iters"][p] == 10
        assert np.abs(pnp["R"][p].reshape(3, 3) - R).max() <= 1e-9
        assert np.abs(pnp["t"][p] - t).max() <= 1e-9
        assert abs(pnp["scale"][p] - np.linalg.norm(t)) <= 1e-9
        assert pnp["rms"][p] <= 1e-9


def test_outliers_are_displaced(outlier_chain):
    c, _ = outlier_chain
    K = pn.K_CHAIN
    for p in (1, 2):
        R, t, good = c["truth"][p]
        idx, Y, nu, nv = pn.correspondences(c["lms"], c["xy2"], c["matches"], c["recs"], K, p)
        X = Y @ R.T + t
        px = np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], 1)
        err = np.linalg.norm(px - c["xy2"][p][idx].astype(np.float64), axis=1)
        is_good = np.isin(idx, good)
        assert err[is_good].max() <= 1e-3 and err[~is_good].min() >= 20 - 1e-3  # float32 pixels


def test_failed_pair_in_the_restatement():
    """A chain whose middle pair failed (no landmarks, record marked): PnP gives it the true pose from
    pair 0's landmarks, and the pair after it has no correspondences."""
    c = pn.chain([(150, 90, 0), (150, 0, 0), (150, 90, 0)], [0, 70, 0], 1500, 12, fail=(1,))
    pnp, masks, _ = pn.reference(c["lms"], c["xy2"], c["matches"], c["recs"], pn.K_CHAIN)
    assert pnp["status"].tolist() == [pn.NONE, pn.OK, pn.NONE] and pnp["n_corr"].tolist() == [0, 70, 0]
    R, t, good = c["truth"][1]
    assert np.abs(pnp["R"][1].reshape(3, 3) - R).max() <= 1e-9 and np.abs(pnp["t"][1] - t).max() <= 1e-9
    assert masks[1].sum() == 70 and not masks[2].any()


def test_carry_scale_bridges_a_failed_pair():
    anchor = np.array([2.0, np.nan, np.nan, np.nan, np.nan])
    scales = np.zeros(5, TRACK_SCALE_DTYPE)
    scales["n_common"] = [-1, 40, 0, 0, 30]
    scales["ratio"] = [0, 1.5, 0, 0, 3.0]
    pnp = np.zeros(5, TRACK_PNP_DTYPE)
    pnp["status"] = [pn.NONE, pn.OK, pn.OK, pn.NO_MODEL, pn.OK]
    pnp["scale"] = [0, 9.0, 0.5, 7.0, 9.0]
    base = carry_scale(anchor, scales)
    assert np.array_equal(base, carry_scale(anchor, scales, pnp=None), equal_nan=True)
    assert base[:2].tolist() == [2.0, 3.0] and np.isnan(base[2:]).all()
    out = carry_scale(anchor, scales, pnp=pnp)
    # pair 1 keeps the ratio (the existing rule set it), pair 2 is bridged, pair 3 has no model, pair 4 has no predecessor
    assert out[:3].tolist() == [2.0, 3.0, 1.5] and np.isnan(out[3:]).all()
    poses = np.zeros(5, TRACK_POSE_DTYPE)
    poses["status"] = 1
    assert np.array_equal(carry_scale(anchor, scales, poses=poses, pnp=pnp), out, equal_nan=True)
    with pytest.raises(ValueError):
        carry_scale(anchor, scales, pnp=pnp[:4])
