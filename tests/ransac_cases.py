"""Point sets shared by the RANSAC tests: the degenerate sets of
test_gpu_edge.py::test_degenerate_correspondences and the per-hypothesis sets of
test_gpu_ransac_hypotheses.py (test_oracle_kats.py checks on the CPU oracle what the GPU
tests rely on).  Plain functions, numpy only."""
import os
import re

import numpy as np

from geom_cases import _px, _rot, correspondences

K_VGA = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
N_HYP = 600

DEGENERATE = ("identical", "repeated", "collinear", "integer", "pure_rotation")


def degenerate_sets():
    rng = np.random.default_rng(7)
    K = K_VGA.copy()
    X = np.c_[rng.uniform(-1, 1, (30, 2)), rng.uniform(3, 6, 30)]
    p1 = X[:, :2] / X[:, 2:] * 500 + [320, 240]
    X2 = X - [0.3, 0.1, 0.0]
    p2 = X2[:, :2] / X2[:, 2:] * 500 + [320, 240]
    line = np.c_[np.linspace(100, 500, 30), np.linspace(50, 400, 30)]
    return {
        "identical": (p1, p1.copy(), K),                      # no motion: every skew E fits
        "repeated": (np.repeat(p1[:8], 4, 0), np.repeat(p2[:8], 4, 0), K),  # 8 distinct pairs, 4 copies each
        "collinear": (line, line + [3.0, 0.0], K),            # all points on one line in both views
        "integer": (np.round(p1), np.round(p2), K),           # pixel-quantised, as ORB keypoints at level 0
        "pure_rotation": (p1, (p1 - [320, 240]) @ np.array([[0.99, -0.14], [0.14, 0.99]]) + [320, 240], K),
    }


def score_chunk():
    """DVO_SCORE_CHUNK, the points per LDS chunk of the score kernel, from the source."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "droplet_visual_odometry_amd", "csrc", "geometry.hip")
    return int(re.search(r"^#define DVO_SCORE_CHUNK (\d+)", open(src).read(), flags=re.M).group(1))


def over_chunk_m():
    """A point count above the score chunk that is no multiple of 64 (a partial last wave pass)."""
    return score_chunk() + 77


def undecided_tail_set():
    """score chunk + 3 correspondences, the last three of them inliers of the motion, for a camera
    whose focal length is tiny: every normalised coordinate is > 1e6, outside the score's
    single-precision range, so every (model, point) test is left to f64 -- listed for the block's
    deferred pass while the list has room, inline after.  A model whose first chunk was all
    deferred has counted nothing yet when the last chunk (3 points, fewer than the bail bound of
    4) starts: only the deferred-test term of the early exit keeps it being scored."""
    m = score_chunk() + 3
    K = K_VGA.copy()
    rng = np.random.default_rng(4)
    X = np.c_[rng.uniform(-1.5, 1.5, (m, 2)), rng.uniform(3, 8, m)]
    p1 = _px(X, K) + rng.normal(0, 0.5, (m, 2))
    p2 = _px(X @ _rot([0.2, 1.0, 0.1], 0.06).T + [0.4, 0.05, 0.1], K) + rng.normal(0, 0.5, (m, 2))
    bad = rng.permutation(m - 3)[: m // 10]
    p2[bad] = rng.uniform([0, 0], [640, 480], (len(bad), 2))
    K[0, 0] = K[1, 1] = 1e-4
    return p1, p2, K


HYPOTHESIS_SETS = DEGENERATE + ("realistic50", "sparse25", "over_chunk", "undecided_tail")
# the sets whose models must almost all have more than 4 inliers (the counts compared exactly)
CAPPED_SETS = ("realistic50", "sparse25", "repeated", "collinear", "integer", "pure_rotation", "over_chunk",
               "undecided_tail")

_CACHE = {}


def hypothesis_sets():
    """name -> (p1, p2, K), float64 and contiguous; built once."""
    if not _CACHE:
        for name, (p1, p2, K) in degenerate_sets().items():
            _CACHE[name] = (p1, p2, K)
        K = K_VGA.copy()
        _CACHE["realistic50"] = (*correspondences(200, K, seed=1, outliers=0.5, noise=0.5), K)
        # a quarter inliers: 0.25^5 per hypothesis keeps niters at the cap of 600
        _CACHE["sparse25"] = (*correspondences(200, K, seed=2, outliers=0.75, noise=0.5), K)
        assert over_chunk_m() % 64 != 0
        _CACHE["over_chunk"] = (*correspondences(over_chunk_m(), K, seed=3, outliers=0.5, noise=0.5), K)
        _CACHE["undecided_tail"] = undecided_tail_set()
        for name, (p1, p2, K) in list(_CACHE.items()):
            _CACHE[name] = (np.ascontiguousarray(p1, np.float64), np.ascontiguousarray(p2, np.float64), K)
    return _CACHE


_ORACLE = {}


def oracle_hypotheses(oracle_mod, name, threshold=1.0):
    """oracle.ransac_hypotheses of a set (N_HYP hypotheses), computed once; treat as read-only."""
    if name not in _ORACLE:
        p1, p2, K = hypothesis_sets()[name]
        ref = oracle_mod.ransac_hypotheses(p1, p2, K, threshold, N_HYP)
        for v in ref.values():
            v.setflags(write=False)
        _ORACLE[name] = ref
    return _ORACLE[name]
