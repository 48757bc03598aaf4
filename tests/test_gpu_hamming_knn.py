"""BFMatcher(NORM_HAMMING).knnMatch on the device (dvo_bf_knn_hamming, cv.BFMatcher.knnMatch) and
the batched ratio stage of the ORB stream (dvo_test_hamming_ratio_batch) against the numpy
restatement of hamming_knn_cases: every index and distance equal.  The restatement is pinned to the
oracle's BFMatcher.match in tests/test_hamming_knn_host.py."""
import numpy as np
import pytest

import hamming_knn_cases as hk

pytestmark = pytest.mark.gpu


def _check(gpu_ctx, q, t, tsplit=0, what=""):
    from droplet_visual_odometry_amd import ops
    wi, wd = hk.knn(q, t, 2)
    for k in (1, 2):
        gi, gd = ops.bf_knn_hamming(q, t, k, tsplit=tsplit, ctx=gpu_ctx)
        assert gi.shape == (len(q), k) and gd.shape == (len(q), k)
        np.testing.assert_array_equal(gi, wi[:, :k], err_msg=f"{what} nq={len(q)} nt={len(t)} k={k} tsplit={tsplit}")
        np.testing.assert_array_equal(gd, wd[:, :k], err_msg=f"{what} nq={len(q)} nt={len(t)} k={k} tsplit={tsplit}")


@pytest.mark.parametrize("kind", ["random", "pool4", "same"])
@pytest.mark.parametrize("nt", hk.NT)
def test_knn_shapes(gpu_ctx, kind, nt):
    from droplet_visual_odometry_amd import ops
    rng = np.random.default_rng(100 + nt)
    for nq in hk.NQ:
        q, t = hk.content(kind, rng, nq, nt)
        _check(gpu_ctx, q, t, what=kind)
        if kind == "same" and nt >= 2:
            gi, gd = ops.bf_knn_hamming(q, t, 2, ctx=gpu_ctx)
            assert np.all(gi == [0, 1]) and np.all(gd == 0)


@pytest.mark.parametrize("kind", ["random", "pool4", "same"])
@pytest.mark.parametrize("nq,nt", [(200, 512), (300, 1100), (1, 256), (257, 320)])
def test_knn_split_trains(gpu_ctx, kind, nq, nt):
    """Sizes at which the per-call path splits the trains (one or two query blocks, 4 or more
    stages): the library's choice and every forced split give the same rows."""
    rng = np.random.default_rng(7)
    q, t = hk.content(kind, rng, nq, nt)
    for tsplit in (0, 1, 2, 3, 4, 8, 16):
        _check(gpu_ctx, q, t, tsplit, kind)


def test_knn_planted(gpu_ctx):
    rng = np.random.default_rng(12)
    for q, t, name in hk.planted_cases(rng):
        for tsplit in (0, 1, 2, 4, 8):
            _check(gpu_ctx, q, t, tsplit, name)


def test_knn_empty_and_limits(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    rng = np.random.default_rng(3)
    q = hk.random_rows(rng, 5)
    gi, gd = ops.bf_knn_hamming(q, q[:0], 2, ctx=gpu_ctx)
    assert np.all(gi == -1) and np.all(gd == hk.FLT_MAX) and gi.shape == (5, 2)
    gi, gd = ops.bf_knn_hamming(q[:0], q, 2, ctx=gpu_ctx)
    assert gi.shape == (0, 2)
    with pytest.raises(DVOError):
        ops.bf_knn_hamming(q, q, 3, ctx=gpu_ctx)
    with pytest.raises(DVOError):
        ops.bf_knn_hamming(np.zeros((8193, 32), np.uint8), q, 2, ctx=gpu_ctx)


def test_cv_knn_match(gpu_ctx):
    from droplet_visual_odometry_amd import cv
    rng = np.random.default_rng(5)
    for nq, nt in ((65, 1), (65, 2), (257, 129), (300, 1100)):
        q, t = hk.content("pool4" if nt == 129 else "random", rng, nq, nt)
        wi, wd = hk.knn(q, t, 2)
        for k in (1, 2):
            rows = cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q, t, k)
            assert len(rows) == nq
            for i, row in enumerate(rows):
                n = min(k, nt)
                assert [(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in row] == \
                    [(i, int(wi[i, s]), 0, float(wd[i, s])) for s in range(n)]
    # crossCheck with k = 1: the cross-checked matches, one row per query
    q, t = hk.content("random", rng, 65, 70)
    bf = cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True)
    rows = bf.knnMatch(q, t, 1)
    flat = [(m.queryIdx, m.trainIdx, m.distance) for r in rows for m in r]
    assert flat == [(m.queryIdx, m.trainIdx, m.distance) for m in bf.match(q, t)]
    assert len(rows) == 65 and 0 < len(flat) < 65
    assert len(bf.knnMatch(q, t, 1, compactResult=True)) == len(flat)


@pytest.mark.parametrize("ratio", [0.75, 1.0])
@pytest.mark.parametrize("case", range(len(hk.RATIO_BATCHES)))
def test_ratio_batch(gpu_ctx, case, ratio):
    """The stream's ratio-mode match stage at crafted counts: top-2 words, kept matches, point
    quads, counts and pair statuses.  The keep-and-drop condition of these cases is asserted on the
    CPU first (and in test_hamming_knn_host.py)."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT
    counts, cap = hk.RATIO_BATCHES[case]
    rng = np.random.default_rng(21)
    desc = hk.ratio_frames(rng, counts, cap)
    kps = hk.keypoints(rng, len(counts), cap)
    P = len(counts) - 1
    want = []
    for p in range(P):
        nq, nt = counts[p], counts[p + 1]
        m = hk.ratio_matches(desc[p, :nq], desc[p + 1, :nt], ratio) if nt >= 2 else []
        if nq >= 32 and nt >= 32:
            assert len(m) >= 8 and nq - len(m) >= 8, (p, len(m))
        want.append(m)
    out = ops.test_hamming_ratio_batch(desc, kps, counts, ratio, ctx=gpu_ctx)
    for p in range(P):
        nq, nt = counts[p], counts[p + 1]
        assert out["status"][p] == (DVO_ENOFEAT if nq == 0 or nt < 2 else 0), p
        wi, wd = hk.knn(desc[p, :nq], desc[p + 1, :nt], 2)
        words = np.where(wi < 0, -1, (np.where(wi < 0, 0, wd).astype(np.int64) << 16) | wi).astype(np.int32)
        np.testing.assert_array_equal(out["top2"][p, :nq], words, err_msg=f"pair {p}")
        m = want[p]
        assert out["nmatch"][p] == len(m), p
        got = out["matches"][p, :len(m)]
        assert [(int(g["queryIdx"]), int(g["trainIdx"]), float(g["distance"])) for g in got] == m, p
        assert np.all(got["imgIdx"] == 0)
        pts = np.array([[kps[p, a]["x"], kps[p, a]["y"], kps[p + 1, b]["x"], kps[p + 1, b]["y"]] for a, b, _ in m],
                       np.float32).reshape(-1, 4)
        np.testing.assert_array_equal(out["pts"][p, :len(m)], pts, err_msg=f"pair {p}")
    if case == 0:
        # [70, 0, 1, 2, 128]: no train, no query, then a second neighbour exists for every query
        assert list(out["status"]) == [DVO_ENOFEAT, DVO_ENOFEAT, 0, 0]
        assert np.all(out["top2"][0, :70] == -1) and out["nmatch"][0] == 0 and out["nmatch"][1] == 0
        assert np.all(out["top2"][2, 0] >= 0) and np.all(out["top2"][3, :2] >= 0)


def test_ratio_batch_one_train(gpu_ctx):
    """A train frame of one descriptor: the nearest is train 0, the second -1 (never a padded
    column), nothing is kept, and the pair is DVO_ENOFEAT."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT
    rng = np.random.default_rng(9)
    counts, cap = [70, 1, 70], 128
    desc = hk.ratio_frames(rng, counts, cap)
    out = ops.test_hamming_ratio_batch(desc, hk.keypoints(rng, 3, cap), counts, 1.0, ctx=gpu_ctx)
    d = hk.hamming(desc[0, :70], desc[1, :1])[:, 0]
    np.testing.assert_array_equal(out["top2"][0, :70, 0], d << 16)
    assert np.all(out["top2"][0, :70, 1] == -1)
    assert out["nmatch"][0] == 0 and out["status"][0] == DVO_ENOFEAT
    assert out["status"][1] == 0 and np.all(out["top2"][1, :1] >= 0)
