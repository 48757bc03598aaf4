"""The fixtures of test_gpu_geometry_params.py and test_gpu_stream_status.py reach the
regimes they are named for, on the CPU oracle alone: without this a GPU case could
pass while exercising nothing (an adaptive stop that never happens, a tie that is
not one, a five-match pair that has six)."""
import numpy as np
import pytest

import geom_cases as G


@pytest.fixture(scope="module")
def grid(oracle_mod):
    out = {}
    for cam, th, pr in G.param_grid():
        K = G.CAMERAS[cam]
        p1, p2 = G.correspondences(400, K)
        out[cam, th, pr] = oracle_mod.find_essential(p1, p2, K, pr, th, 1000)
    return out


def test_grid_has_adaptive_and_capped_cases(grid):
    for cam in G.CAMERAS:
        iters = [it for (c, th, pr), (E, mask, it) in grid.items() if c == cam and E is not None]
        assert 1000 in iters                      # the max_iters cap
        assert any(it < 32 for it in iters)        # stops inside the first round
        assert any(32 <= it < 1000 for it in iters)  # stops adaptively in a later round
        inl = {int(mask.sum()) for (c, th, pr), (E, mask, it) in grid.items() if c == cam and E is not None}
        assert len(inl) >= 8 and min(inl) < 10 and max(inl) > 250


def test_grid_has_the_zero_threshold_case(grid):
    for cam, K in G.CAMERAS.items():
        assert G.score_threshold_f32(G.T_ZERO_THRESHOLD, K) < G.FLT_MIN
        E, mask, it = grid[cam, G.T_ZERO_THRESHOLD, 0.999]
        assert E is None and it == 1000            # no model: DVO_ENOMODEL
        assert all(G.score_threshold_f32(th, K) >= G.FLT_MIN for th in G.THRESHOLDS)


def test_size_and_round_cases_find_models(oracle_mod):
    for m in G.M_SIZES:
        p1, p2 = G.correspondences(m, G.K_SKEW)
        its = []
        for mi in G.MAX_ITERS:
            E, mask, it = oracle_mod.find_essential(p1, p2, G.K_SKEW, 0.999, 1.0, mi)
            assert E is not None and E.shape == (3, 3) and it <= mi
            its.append(it)
        if m >= 64:  # the loop is still running at every round boundary
            assert its[:4] == [1, 31, 32, 33] and its[4] > 33


def _pick(oracle_mod, E, R, t):
    dec = G.decompositions(oracle_mod, E)
    hit = [i for i, (Rc, tc) in enumerate(dec) if np.allclose(Rc, R, atol=1e-9) and np.allclose(tc, t.ravel(), atol=1e-9)]
    assert len(hit) == 1
    return hit[0]


def test_pose_scenes_reach_every_pick_and_tie(oracle_mod):
    K = G.K_SKEW
    dec = G.decompositions(oracle_mod, G.POSE_E)
    for a in range(4):
        for b in range(a + 1, 4):  # four distinct (R, +-t) combinations
            assert not (np.allclose(dec[a][0], dec[b][0]) and np.allclose(dec[a][1], dec[b][1]))
    picks, zero_ties, max_ties = set(), 0, 0
    for name, (E, parts, want) in G.POSE_SCENES.items():
        p1, p2 = G.pose_scene(oracle_mod, E, parts)
        for d in G.DIST_THRESHOLDS:
            cnt = G.pose_counts(oracle_mod, E, p1, p2, K, d)
            good, R, t, mo = oracle_mod.recover_pose(E, p1, p2, K, d)
            pick = _pick(oracle_mod, E, R, t)
            assert good == max(cnt) == cnt[pick] == int(np.count_nonzero(mo))
            assert pick == cnt.index(max(cnt))     # the >= chain: the lowest index among the maxima
            if d == 50.0:
                assert pick == want
                picks.add(pick)
                if name.startswith("tie"):
                    assert sorted(cnt)[-1] == sorted(cnt)[-2] > 0
                    max_ties += 1
            if max(cnt) == 0:
                assert pick == 0
                zero_ties += 1
    assert picks == {0, 1, 2, 3}
    assert zero_ties >= 4 and max_ties == 4


def test_axis_scene_has_exact_zero_translation_components(oracle_mod):
    """R = I, t = (0, 0, 1): recoverPose's t has exact zeros, so pose_count_kernel cannot
    mirror decomposition c into c + 2 and triangulates it on its own."""
    t = G.decompositions(oracle_mod, G.AXIS_E)[0][1]
    assert np.count_nonzero(t == 0.0) == 2 and abs(t[2]) == 1.0
    t = G.decompositions(oracle_mod, G.POSE_E)[0][1]
    assert np.count_nonzero(t == 0.0) == 0


def test_pose_masks_change_the_result(oracle_mod):
    E, parts, _ = G.POSE_SCENES["pick0"]  # one decomposition holds every point: a mask cannot move the pick
    p1, p2 = G.pose_scene(oracle_mod, E, parts)
    rmask = G.ransac_mask(oracle_mod, p1, p2, G.K_SKEW)
    masks = G.pose_masks(len(p1), rmask)
    base = oracle_mod.recover_pose(E, p1, p2, G.K_SKEW, 50.0)
    assert set(np.unique(base[3])) <= {0, 255} and base[0] == 200
    for name, mk in masks.items():
        if mk is None:
            continue
        good, R, t, mo = oracle_mod.recover_pose(E, p1, p2, G.K_SKEW, 50.0, mk)
        # cv::recoverPose: bitwise_and(mask, mask1, mask1), good = countNonZero(mask1)
        np.testing.assert_array_equal(mo, base[3] & mk)
        assert good == np.count_nonzero(mo)
        assert 0 < np.count_nonzero(mk) < len(mk)
    assert set(np.unique(oracle_mod.recover_pose(E, p1, p2, G.K_SKEW, 50.0, masks["ransac01"])[3])) == {0, 1}


def test_triangulation_cases(oracle_mod):
    for kind in G.TRI_KINDS:
        P1, P2, x1, x2 = G.triangulation_case(kind, 257)
        X = oracle_mod.triangulate(P1, P2, x1, x2)
        assert X.shape == (4, 257) and np.all(np.isfinite(X))
        np.testing.assert_allclose(np.linalg.norm(X, axis=0), 1.0, rtol=1e-9)
        assert (kind == "same") == np.array_equal(P1, P2)
        if kind == "integer":
            np.testing.assert_array_equal(x1, np.round(x1))
        if kind == "canonical":
            np.testing.assert_array_equal(P1[:, :3], G.K_SKEW)
            np.testing.assert_array_equal(P1[:, 3], 0)


def test_mixed_batch_reaches_every_pair_kind(oracle_mod):
    refs = G.mixed_reference(oracle_mod)
    assert len(refs) == len(G.MIXED_KINDS) == 5
    normal, few, five, model, blank = refs
    assert len(normal["q"]) > 50 and normal["E"].shape == (3, 3) and normal["good"] > 0
    assert 1 <= len(few["q"]) <= 4 and few["E"] is None
    assert len(five["q"]) == 5 and five["E"].shape[0] > 3 and five["E"].shape[0] % 3 == 0 and five["R"] is None
    assert len(model["q"]) >= 6 and model["E"].shape == (3, 3) and model["R"] is not None
    assert len(blank["kp_cur"]) == 0 and len(blank["kp_prev"]) > 0 and blank["E"] is None
    assert [G.pair_successful(r) for r in refs] == [True, False, False, True, False]
