"""BFMatcher(NORM_HAMMING).knnMatch and the ORB stream's ratio test: what holds without a GPU.
The ABI declares and binds the new entry points, the cv2-shaped shim answers empty sets and
refuses what OpenCV refuses before any device call, and the numpy restatement the GPU tests
compare against (hamming_knn_cases) agrees with the oracle's BFMatcher.match on every case."""
import os
import re

import numpy as np
import pytest

import hamming_knn_cases as hk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_native_binds():
    from droplet_visual_odometry_amd import _native
    text = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name in ("dvo_bf_knn_hamming", "dvo_stream_set_ratio_test", "dvo_test_hamming_ratio_batch",
                 "dvo_test_bf_knn_hamming"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _native._SIGNATURES, name
    args, res = _native._SIGNATURES["dvo_stream_set_ratio_test"]
    assert len(args) == 2 and args[1] is _native.ctypes.c_double
    assert len(_native._SIGNATURES["dvo_bf_knn_hamming"][0]) == 8


def test_knn_match_empty_sets_need_no_gpu():
    from droplet_visual_odometry_amd import cv
    bf = cv.BFMatcher(cv.NORM_HAMMING)
    q = np.zeros((3, 32), np.uint8)
    none = np.zeros((0, 32), np.uint8)
    assert bf.knnMatch(q, none, 2) == [[], [], []]
    assert bf.knnMatch(none, q, 2) == []
    assert bf.knnMatch(none, none, 2) == []
    assert bf.knnMatch(q, none, 2, compactResult=True) == []
    assert bf.knnMatch(q, none, 1) == [[], [], []]


def test_knn_match_refuses():
    from droplet_visual_odometry_amd import cv
    q = np.zeros((3, 32), np.uint8)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).knnMatch(q, q, 2)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q, q, 3)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q, q, 0)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q.astype(np.float32), q, 2)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(np.zeros((3, 16), np.uint8), q, 2)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(None, q, 2)
    with pytest.raises(cv.error):
        cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q, q, 2, mask=np.ones((3, 3), np.uint8))


def _pin(oracle_mod, q, t):
    idx, dist = hk.knn(q, t, 2)
    oq, ot, od = oracle_mod.bf_match(q, t, 0)
    np.testing.assert_array_equal(oq, np.arange(len(q)))
    np.testing.assert_array_equal(idx[:, 0], ot)
    np.testing.assert_array_equal(dist[:, 0], od)
    # the second column on its own terms: the best of the trains left when the first is taken out
    if len(t) >= 2:
        for i in range(0, len(q), max(1, len(q) // 16)):
            rest = np.delete(np.arange(len(t)), idx[i, 0])
            _, t2, d2 = oracle_mod.bf_match(q[i:i + 1], t[rest], 0)
            assert rest[t2[0]] == idx[i, 1] and d2[0] == dist[i, 1]
    else:
        assert np.all(idx[:, 1] == -1) and np.all(dist[:, 1] == hk.FLT_MAX)


@pytest.mark.parametrize("kind", ["random", "pool4", "same"])
def test_restatement_equals_oracle_shapes(oracle_mod, kind):
    rng = np.random.default_rng(11)
    for nt in hk.NT:
        for nq in hk.NQ:
            _pin(oracle_mod, *hk.content(kind, rng, nq, nt))
    _pin(oracle_mod, *hk.content(kind, rng, 300, 1100))
    _pin(oracle_mod, *hk.content(kind, rng, 200, 512))


def test_restatement_equals_oracle_planted(oracle_mod):
    rng = np.random.default_rng(12)
    for q, t, _ in hk.planted_cases(rng):
        _pin(oracle_mod, q, t)
        idx, dist = hk.knn(q, t, 2)
        assert np.all(dist[:60] <= 5)  # the planted rows are the two nearest


def test_ratio_frames_keep_and_drop():
    """The condition of the batched ratio test's cases, on the CPU: every pair with at least 32
    queries and 32 trains keeps at least 8 matches and drops at least 8, at both ratios."""
    for counts, cap in hk.RATIO_BATCHES:
        desc = hk.ratio_frames(np.random.default_rng(21), counts, cap)
        for ratio in (0.75, 1.0):
            for p in range(len(counts) - 1):
                nq, nt = counts[p], counts[p + 1]
                if nq < 32 or nt < 32:
                    continue
                kept = len(hk.ratio_matches(desc[p, :nq], desc[p + 1, :nt], ratio))
                assert kept >= 8 and nq - kept >= 8, (counts, p, ratio, kept)
