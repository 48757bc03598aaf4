"""The k-NN modes' one-call pair path (D8) without a GPU: the new entry points are
declared, exported and bound, and the drop-in keeps the operator-by-operator path
whenever the stock operators are not in use (no library call is made to decide)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_knn_pair_create", "dvo_knn_pair_destroy", "dvo_knn_pair_run", "dvo_knn_pair_get_matches",
       "dvo_knn_pair_get_features", "dvo_test_ratio_gather"]


def test_new_symbols_declared_exported_bound():
    from droplet_visual_odometry_amd import _native, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    lib = _native.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in _native._SIGNATURES and getattr(lib, name).argtypes is not None, name
    for macro in ("DVO_DETECT_SIFT 0", "DVO_DETECT_SURF 1", "DVO_MATCH_BF_L1 0", "DVO_MATCH_FLANN 1"):
        assert "#define " + macro in hdr


def test_config_struct_matches_header_layout():
    """dvo_knn_pair_config as a C compiler lays it out: 4 int32, double, 2 int32, double,
    9 doubles, 2 doubles, int32 (+ padding), double."""
    from droplet_visual_odometry_amd._native import KnnPairConfig
    f = KnnPairConfig
    assert (f.width.offset, f.height.offset, f.detector.offset, f.matcher.offset) == (0, 4, 8, 12)
    assert (f.hessian_threshold.offset, f.trees.offset, f.checks.offset, f.ratio.offset) == (16, 24, 28, 32)
    assert (f.K.offset, f.prob.offset, f.threshold.offset, f.max_iters.offset, f.dist_thresh.offset) == \
        (40, 112, 120, 128, 136)
    assert ctypes.sizeof(f) == 144


def test_null_handles_are_refused():
    from droplet_visual_odometry_amd import _native
    lib = _native.load_library()
    n = ctypes.c_int()
    assert lib.dvo_knn_pair_create(None, None, None) == _native.DVO_EINVAL
    assert lib.dvo_knn_pair_run(None, None, None, 0, 0, None, None) == _native.DVO_EINVAL
    assert lib.dvo_knn_pair_get_matches(None, None, 0, ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_knn_pair_get_features(None, 0, None, None, 0, ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_test_ratio_gather(None, None, None, 0, None, 0, None, 0, 0.75, 0, None, None, None, None) == \
        _native.DVO_EINVAL
    lib.dvo_knn_pair_destroy(None)


def _v3():
    sys.path.insert(0, os.path.join(ROOT, "droplet_visual_odometry_amd", "dropin"))
    try:
        import visual_odometry_v3 as v3
    finally:
        sys.path.pop(0)
    return v3


def _vo(v3, tmp_path, mode, cls=None):
    y = tmp_path / "cal.yaml"
    y.write_text("camera_matrix:\n  rows: 3\n  cols: 3\n  data: [500.0, 0.0, 320.0, 0.0, 500.0, 240.0, 0.0, 0.0, 1.0]\n"
                 "distortion_coefficients:\n  rows: 1\n  cols: 5\n  data: [0.0, 0.0, 0.0, 0.0, 0.0]\n")
    return (cls or v3.VisualOdometry)(mode=mode, calibration_file_path=str(y), controlled=True, real_marker_length=0.1)


class _Engine:
    """Stands in for ops.KnnPairStream: records how it was made and called."""
    made = []

    def __init__(self, w, h, K, **kw):
        self.kw = dict(kw, w=w, h=h)
        self.calls = []
        _Engine.made.append(self)

    def pair(self, prev, cur, reuse_prev=False, rng_state=None):
        from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
        self.calls.append((prev is None, reuse_prev, rng_state))
        rec = np.zeros(1, PAIR_RECORD_DTYPE)[0]
        rec["n_models"] = 1
        rec["E"][:] = np.arange(9)
        rec["status"] = self.status
        return rec, 12345

    status = 0


@pytest.fixture
def stub_engine(monkeypatch):
    from droplet_visual_odometry_amd import ops
    _Engine.made = []
    _Engine.status = 0
    monkeypatch.setattr(ops, "KnnPairStream", _Engine)
    return _Engine


IMG = np.zeros((48, 64), np.uint8)
IMG2 = np.ones((48, 64), np.uint8)


@pytest.mark.parametrize("mode,detector,matcher", [("knn_sift", "sift", "bf"), ("surf", "surf", "bf"),
                                                   ("flann", "sift", "flann")])
def test_dropin_takes_the_fused_call_with_stock_operators(tmp_path, stub_engine, mode, detector, matcher):
    from droplet_visual_odometry_amd import cv
    v3 = _v3()
    vo = _vo(v3, tmp_path, mode)
    cv.setRNGSeed(7)
    E, R, t = vo._fused_pair(IMG, IMG2)
    assert len(stub_engine.made) == 1
    eng = stub_engine.made[0]
    assert (eng.kw["detector"], eng.kw["matcher"], eng.kw["w"], eng.kw["h"]) == (detector, matcher, 64, 48)
    assert eng.kw["hessian_threshold"] == 400.0
    assert eng.calls == [(False, False, 7)]
    np.testing.assert_array_equal(E, np.arange(9.0).reshape(3, 3))
    # the state the call leaves is committed in flann mode only
    assert cv._the_rng() == (12345 if mode == "flann" else 7)
    vo._fused_pair(IMG2, IMG)  # the last current frame comes back: reused, same engine
    assert len(stub_engine.made) == 1 and eng.calls[-1][:2] == (True, True)
    # a failing pair: nothing is committed, nothing is reused next
    stub_engine.status = -3
    cv.setRNGSeed(9)
    assert vo._fused_pair(IMG, IMG2) is None
    assert cv._the_rng() == 9
    stub_engine.status = 0
    vo._fused_pair(IMG2, IMG)
    assert eng.calls[-1][:2] == (False, False)


def test_dropin_keeps_the_operator_path(tmp_path, stub_engine, monkeypatch):
    from droplet_visual_odometry_amd import cv
    v3 = _v3()

    class MyMatcher(cv.BFMatcher):
        pass

    vo = _vo(v3, tmp_path, "knn_sift")
    vo.bf = MyMatcher(normType=cv.NORM_L1, crossCheck=False)
    assert vo._fused_pair(IMG, IMG2) is None

    vo = _vo(v3, tmp_path, "knn_sift")
    vo.bf = cv.BFMatcher(normType=cv.NORM_L2, crossCheck=False)
    assert vo._fused_pair(IMG, IMG2) is None

    class Overridden(v3.VisualOdometry):
        def get_matches_between_two_frames(self, *a, **k):
            return super().get_matches_between_two_frames(*a, **k)

    for mode in ("knn_sift", "surf", "flann"):
        assert _vo(v3, tmp_path, mode, Overridden)._fused_pair(IMG, IMG2) is None

    assert _vo(v3, tmp_path, "sift")._fused_pair(IMG, IMG2) is None  # bf.match, no neighbour list: v3:201

    class MySift(cv.SIFT):
        pass

    vo = _vo(v3, tmp_path, "knn_sift")
    vo.feature_detector = MySift()
    assert vo._fused_pair(IMG, IMG2) is None

    vo = _vo(v3, tmp_path, "surf")
    assert vo._fused_pair(IMG, IMG2.astype(np.float32)) is None
    assert vo._fused_pair(IMG, np.zeros((48, 65), np.uint8)) is None
    assert vo._fused_pair(np.zeros((48, 64, 3), np.uint8), np.zeros((48, 64, 3), np.uint8)) is None

    monkeypatch.setattr(cv, "OPENCV_SEMANTICS", "3.2")
    assert _vo(v3, tmp_path, "flann")._fused_pair(IMG, IMG2) is None
    assert _vo(v3, tmp_path, "knn_sift")._fused_pair(IMG, IMG2) is not None  # only flann depends on it
    assert len(stub_engine.made) == 1
