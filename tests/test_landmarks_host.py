"""Landmarks without a GPU: the ABI's struct and the numpy dtype agree, both sides name the new
entry points, and the expectation the GPU tests compare against (landmark_cases.expected) keeps
exactly what OpenCV's recoverPose keeps when it is handed findEssentialMat's mask."""
import os
import re

import numpy as np
import pytest

import landmark_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dvo_stream_set_landmarks", "dvo_knn_stream_set_landmarks", "dvo_test_landmarks")
C_TYPES = {"int32_t": ("<i4", 4), "float": ("<f4", 4), "double": ("<f8", 8)}


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_struct_and_dtype_agree():
    """dvo_landmark's fields, laid out by C's rules for these naturally aligned types, are
    LANDMARK_DTYPE's names, types and offsets; 48 bytes."""
    from droplet_visual_odometry_amd._native import LANDMARK_DTYPE
    body = re.search(r"typedef struct \{([^}]*)\} dvo_landmark;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        code, size = C_TYPES[ctype]
        for name in (n.strip() for n in names.split(",")):
            off = (off + size - 1) // size * size
            fields.append((name, code, off))
            off += size
    size = (off + 7) // 8 * 8
    assert size == LANDMARK_DTYPE.itemsize == 48
    assert [f[0] for f in fields] == list(LANDMARK_DTYPE.names)
    for name, code, o in fields:
        assert LANDMARK_DTYPE.fields[name][0] == np.dtype(code), name
        assert LANDMARK_DTYPE.fields[name][1] == o, name
    assert "48 bytes" in _header()


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
    from droplet_visual_odometry_amd import stream
    for cls in (stream.FrameStream, stream.KnnFrameStream):
        assert callable(getattr(cls, "bind_landmarks"))
    assert callable(stream.Landmarks)


@pytest.mark.parametrize("m", (6, 64, 256, 257))
def test_expected_keeps_what_recover_pose_keeps_with_the_mask(oracle_mod, m):
    p1, p2, K = lc.case(m)
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    E, mask, _ = oracle_mod.find_essential(p1, p2, K)
    assert E.shape == (3, 3)
    _, _, _, out = oracle_mod.recover_pose(E, p1, p2, K, mask=mask)
    want = lc.expected(oracle_mod, p1, p2, K)
    np.testing.assert_array_equal(want["match"], np.flatnonzero(out != 0))
    assert want["count"] == len(want["match"]) == len(want["xyz"]) > 0
    assert np.isfinite(want["xyz"]).all() and (want["xyz"][:, 2] > 0).all() and (want["xyz"][:, 2] < 50).all()


def test_case_conditions(oracle_mod):
    """What the GPU test's sizes are chosen for: five matches give several models (no landmarks),
    every other size one model with landmarks, and each filter alone drops points."""
    only_pose = only_inlier = 0
    for m in lc.SIZES:
        p1, p2, K = lc.case(m)
        p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
        E, _, _ = oracle_mod.find_essential(p1, p2, K)
        w = lc.expected(oracle_mod, p1, p2, K)
        if m == 5:
            assert E.shape[0] > 3 and w["count"] == 0
            continue
        assert E.shape[0] == 3 and 0 < w["count"] < m, m
        only_pose += w["only_pose"]
        only_inlier += w["only_inlier"]
    assert only_pose > 0 and only_inlier > 0
