"""SIFT_create(nfeatures) (dvo_sift_detect_and_compute_n and the nfeatures setters) without a GPU:
the new entry points are declared, exported and bound, cv.SIFT_create takes nfeatures, bad values
are refused, dvo_sift_retain_bytes is the header's formula, and the inputs of the GPU tests
(sift_nfeatures_cases.py) really cut, tie and permute on the CPU oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sift_nfeatures_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_sift_detect_and_compute_n", "dvo_sift_retain_bytes", "dvo_sift_batch_set_nfeatures",
       "dvo_knn_pair_set_nfeatures", "dvo_knn_stream_set_nfeatures"]


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


def test_header_comments_cite_the_reference_lines():
    """Each new entry point's comment names v3:100 (SIFT_create) and v3:373 (detectAndCompute)."""
    hdr = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name in NEW:
        at = hdr.index(name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "100" in comment and "373" in comment, name


def test_cv_sift_create_takes_nfeatures():
    from droplet_visual_odometry_amd import cv
    for make in (cv.SIFT_create, cv.xfeatures2d.SIFT_create, cv.SIFT):
        d = make(nfeatures=7)
        assert d.getNFeatures() == 7 and d.descriptorSize() == 128
        assert make().getNFeatures() == 0
        assert make(7).getNFeatures() == 7  # the first constructor argument
    for bad in (dict(nOctaveLayers=4), dict(contrastThreshold=0.03), dict(edgeThreshold=12), dict(sigma=1.2)):
        with pytest.raises(cv.error):
            cv.SIFT_create(nfeatures=7, **bad)


def test_negative_nfeatures_is_refused():
    from droplet_visual_odometry_amd import _native, cv, ops
    for bad in (-1, 2.5):
        with pytest.raises(cv.error):
            cv.SIFT_create(nfeatures=bad)
        with pytest.raises(_native.DVOError) as e:
            ops._check_nfeatures(bad)
        assert e.value.code == _native.DVO_EINVAL
    assert ops._check_nfeatures(0) == 0 and ops._check_nfeatures(300) == 300


def test_null_handles_are_refused():
    from droplet_visual_odometry_amd import _native
    lib = _native.load_library()
    n = ctypes.c_int()
    assert lib.dvo_sift_detect_and_compute_n(None, None, 8, 8, 8, 4, None, None, 0, ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_sift_batch_set_nfeatures(None, 4) == _native.DVO_EINVAL
    assert lib.dvo_knn_pair_set_nfeatures(None, 4) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_set_nfeatures(None, 4) == _native.DVO_EINVAL


def test_retain_bytes():
    """Per frame: a keypoint list, the responses and their positions at the list capacity of 65536,
    and two position arrays of 65537; 0 for a group the batch would reject."""
    from droplet_visual_odometry_amd import _native, ops
    lib = _native.load_library()
    frame = 65536 * (_native.KEYPOINT_DTYPE.itemsize + 4 + 4) + 2 * 65537 * 4
    assert frame == 2883592
    for g in (1, 2, 16, 64):
        assert lib.dvo_sift_retain_bytes(g) == g * frame
        assert ops.SiftBatch.retain_bytes(g) == g * frame
    for g in (0, -1, 65):
        assert lib.dvo_sift_retain_bytes(g) == 0


def _kept(oracle_mod, name, n):
    k, _ = sc.full(oracle_mod, name)
    p = sc.perm(oracle_mod, name, n)
    assert sorted(set(p.tolist())) == sorted(p.tolist()) and len(p) <= len(k)  # a selection of the list
    if n < len(k):  # retainBest runs (also where a tie at the bottom then keeps the whole list)
        # what retainBest promises: everything at or above the boundary response, nothing below
        b = np.sort(k["response"])[::-1][n - 1]
        assert sorted(p.tolist()) == np.flatnonzero(k["response"] >= b).tolist()
        assert not np.array_equal(p, np.arange(len(p))), "the cut is not a permutation of the list"
    return len(p)


@pytest.mark.parametrize("name,n,kept", sc.CUTS)
def test_detector_cases_cut_tie_and_permute(oracle_mod, name, n, kept):
    assert len(sc.full(oracle_mod, name)[0]) == sc.FULL[name]
    assert _kept(oracle_mod, name, n) == kept
    assert n <= kept <= sc.FULL[name] and n < sc.FULL[name]
    # at and above the list's length nothing is cut
    full = sc.FULL[name]
    assert _kept(oracle_mod, name, full) == full and _kept(oracle_mod, name, full + 1) == full


def test_group_frames_cut(oracle_mod):
    kept = tuple(_kept(oracle_mod, name, sc.GROUP_N) for name in sc.GROUP_FRAMES)
    assert kept == sc.GROUP_KEPT
    full = [len(sc.full(oracle_mod, name)[0]) for name in sc.GROUP_FRAMES]
    assert full[:3] == [107, 42, 469]
    assert sum(c > 40 for c in full) >= 3 and max(kept) <= 40  # feat_cap 40: below full counts, above every kept one
    assert sum(k == 16 for k in kept) == 1 and sum(k > 16 for k in kept) == 4  # feat_cap 16: complete and not


def test_synthetic_frames_cut(oracle_mod):
    names = [("synth", i) for i in range(4)]
    assert tuple(len(sc.full(oracle_mod, nm)[0]) for nm in names) == sc.SYNTH_FULL
    for n, want in sc.SYNTH_KEPT.items():
        assert tuple(_kept(oracle_mod, nm, n) for nm in names) == want
    assert sc.SYNTH_FULL[3] > 1024  # more keypoints than a workgroup has lanes
    assert min(sc.SYNTH_FULL) > 304  # feat_cap 304 is below every full count


def test_dropin_keys_the_fused_engine_on_nfeatures(tmp_path, monkeypatch):
    """D8: a detector replaced by SIFT_create(nfeatures = N) stays on the one-call path, with an
    engine made for N; the default detector asks for nfeatures 0."""
    from test_knn_pair_host import IMG, IMG2, _Engine, _v3, _vo
    from droplet_visual_odometry_amd import cv, ops
    _Engine.made, _Engine.status = [], 0
    monkeypatch.setattr(ops, "KnnPairStream", _Engine)
    v3 = _v3()
    for mode in ("knn_sift", "flann"):
        _Engine.made = []
        vo = _vo(v3, tmp_path, mode)
        assert vo._fused_pair(IMG, IMG2) is not None
        assert [e.kw["nfeatures"] for e in _Engine.made] == [0]
        vo.feature_detector = cv.SIFT_create(nfeatures=300)
        assert vo._fused_pair(IMG, IMG2) is not None
        assert [e.kw["nfeatures"] for e in _Engine.made] == [0, 300]
        assert _Engine.made[-1].calls[-1][:2] == (False, False)  # a new engine detects both frames
        assert vo._fused_pair(IMG2, IMG) is not None  # the same detector: the same engine, the cache serves
        assert len(_Engine.made) == 2 and _Engine.made[-1].calls[-1][:2] == (True, True)
    _Engine.made = []
    vo = _vo(v3, tmp_path, "surf")
    assert vo._fused_pair(IMG, IMG2) is not None and _Engine.made[0].kw["nfeatures"] == 0
