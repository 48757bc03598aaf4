"""csrc/sift.hip and csrc/surf.hip in the branches the textured and synthetic frames never enter: on every
case of detector_cases.py (test_detector_census.py asserts, with the oracle's counters, which branches those
are: singular refinement systems, det <= 0, duplicates, orientation peak wrap, windows cut by the border,
the descriptor radius clamp, saturation at 255, exact ties in both sort orders, SURF's clamped window
samples and all three INTER_AREA paths, ...) the per-call operators, the group detectors over the cases
of a size as one stack, and the k-NN pair stream equal the oracle bit for bit; and SURF's keypoint list
overflows as documented (DVO_ECAP, the frame marked, its neighbours untouched).

SIFT's own lists (65536 keypoints, 2^18 candidates) cannot be overflowed by a frame small enough for a
test; that is left out."""
import numpy as np
import pytest

import detector_cases as dc
from sift_batch_frames import CONSTANT
from test_gpu_sift import _check as _check_sift
from test_gpu_surf import _check as _check_surf

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in dc.cases()]
_ORA = {}


def _ora_sift(oracle_mod, name, img):
    if ("sift", name) not in _ORA:
        _ORA[("sift", name)] = oracle_mod.sift_detect_and_compute(img)
    return _ORA[("sift", name)]


def _ora_surf(oracle_mod, name, img, thr):
    if ("surf", name, thr) not in _ORA:
        _ORA[("surf", name, thr)] = oracle_mod.surf_detect_and_compute(img, thr)
    return _ORA[("surf", name, thr)]


def _same(got, want):
    assert len(got) == len(want)
    for (kg, dg), (kw, dw) in zip(got, want):
        assert len(kg) == len(kw)
        np.testing.assert_array_equal(kg.view(np.uint8), kw.view(np.uint8))
        np.testing.assert_array_equal(dg.view(np.uint32), dw.view(np.uint32))


def _stack(w, h):
    """The cases of a size with the constant frame of the group detectors' tests in the middle: 7, 11 and 7
    frames, no multiple of the group of 3.  (names, frames); the constant frame's name is None."""
    cs = dc.by_size(w, h)
    mid = len(cs) // 2
    names = [c.name for c in cs[:mid]] + [None] + [c.name for c in cs[mid:]]
    frames = np.stack([c.img for c in cs[:mid]] + [np.full((h, w), 90, np.uint8)] + [c.img for c in cs[mid:]])
    assert len(frames) % 3 != 0 and 0 < mid < len(frames) - 1
    return names, frames


@pytest.mark.parametrize("name", NAMES)
def test_per_call_operators_equal_oracle(gpu_ctx, oracle_mod, name):
    c = next(c for c in dc.cases() if c.name == name)
    assert _check_sift(gpu_ctx, oracle_mod, c.img) >= c.min_sift
    _check_surf(gpu_ctx, oracle_mod, c.img, 400.0)
    assert _check_surf(gpu_ctx, oracle_mod, c.img, c.surf_thr) >= c.min_surf


@pytest.mark.parametrize("wh", dc.SIZES)
def test_sift_group_stack_equals_oracle(gpu_ctx, oracle_mod, wh):
    from droplet_visual_odometry_amd import ops
    w, h = wh
    names, frames = _stack(w, h)
    blank = (np.zeros(0, oracle_mod.KEYPOINT_DTYPE), np.zeros((0, 128), np.float32))
    ora = [blank if n is None else _ora_sift(oracle_mod, n, f) for n, f in zip(names, frames)]
    sb = ops.SiftBatch(w, h, 3, ctx=gpu_ctx)
    got = sb.detect(frames)
    sb.close()
    assert len(got[names.index(None)][0]) == 0  # the constant frame, between two frames with keypoints
    _same(got, ora)


@pytest.mark.parametrize("wh", dc.SIZES)
def test_surf_group_stack_equals_oracle(gpu_ctx, oracle_mod, wh):
    """At 400 and at the lowest threshold the size's cases name (0: every other threshold's keypoints are
    among them), on one handle."""
    from droplet_visual_odometry_amd import ops
    w, h = wh
    names, frames = _stack(w, h)
    low = min(c.surf_thr for c in dc.by_size(w, h))
    blank = (np.zeros(0, oracle_mod.KEYPOINT_DTYPE), np.zeros((0, 64), np.float32))
    sb = ops.SurfBatch(w, h, 3, ctx=gpu_ctx)
    for thr in (400.0, low):
        ora = [blank if n is None else _ora_surf(oracle_mod, n, f, thr) for n, f in zip(names, frames)]
        assert sum(len(k) for k, _ in ora) >= 4
        got = sb.detect(frames, thr)
        assert len(got[names.index(None)][0]) == 0
        _same(got, ora)
    sb.close()


@pytest.mark.parametrize("detector", ["sift", "surf"])
def test_knn_pair_stream_on_exact_ties(gpu_ctx, oracle_mod, detector):
    """The tiled noise against itself shifted by one tile: most queries have two train descriptors at
    exactly the same distance (0), which the ratio test must drop as the oracle chain does
    (test_gpu_knn_pair.py::test_knn_pair_stream_equals_oracle_chain).  SIFT keeps fewer than 5 matches:
    the record says DVO_EFEWPTS; SURF keeps enough for findEssentialMat."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EFEWPTS
    a, b = dc.tiled(), dc.tiled(dc.TILE)
    K = np.array([[150.0, 0, 88.0], [0, 150.0, 80.0], [0, 0, 1]])
    if detector == "sift":
        (k1, d1), (k2, d2) = _ora_sift(oracle_mod, "tiled", a), _ora_sift(oracle_mod, "tiled_shifted", b)
    else:
        (k1, d1), (k2, d2) = _ora_surf(oracle_mod, "tiled", a, 400.0), _ora_surf(oracle_mod, "tiled_shifted", b, 400.0)
    idx, dist = oracle_mod.bf_knn_float(d1, d2, 2, 0)
    assert int((dist[:, 0] == dist[:, 1]).sum()) >= 20  # the ties are there
    keep = [q for q in range(len(d1)) if float(dist[q, 0]) < 0.75 * float(dist[q, 1])]
    ks = ops.KnnPairStream(176, 160, K, detector=detector, matcher="bf", ctx=gpu_ctx)
    rec, _ = ks.pair(a, b)
    m = ks.matches()
    feats = [ks.features(0), ks.features(1)]
    ks.close()
    _same(feats, [(k1, d1), (k2, d2)])
    assert (rec["n_kp_prev"], rec["n_kp_cur"], rec["n_matches"]) == (len(k1), len(k2), len(keep))
    np.testing.assert_array_equal(m["queryIdx"], keep)
    np.testing.assert_array_equal(m["trainIdx"], idx[keep, 0])
    np.testing.assert_array_equal(m["distance"].view(np.uint32), dist[keep, 0].astype(np.float32).view(np.uint32))
    if len(keep) < 5:
        assert rec["status"] == DVO_EFEWPTS and rec["n_models"] == 0 and not np.any(rec["E"])
        return
    p1 = np.stack([k1["x"][keep], k1["y"][keep]], 1).astype(np.float64)
    p2 = np.stack([k2["x"][idx[keep, 0]], k2["y"][idx[keep, 0]]], 1).astype(np.float64)
    E, _, _ = oracle_mod.find_essential(p1, p2, K)
    assert E is not None and E.shape == (3, 3)
    assert rec["status"] == 0 and rec["n_models"] == 1
    np.testing.assert_array_equal(rec["E"].reshape(3, 3), E)


def test_surf_list_overflow(gpu_ctx, oracle_mod):
    """Uniform noise at 512 x 512, threshold 0: more keypoints than the device list holds
    (kp_cap = max(4096, w h / 64) = 4096).  The per-call operator raises DVO_ECAP; in a group stack
    between two ordinary frames only that frame is flagged (2: list overflow), the neighbours equal the
    oracle, and nothing is written past a frame's features nor behind the last slot."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ECAP, KEYPOINT_DTYPE, DVOError
    w = h = 512
    kp_cap = max(4096, w * h // 64)
    over = dc.overflow_noise()
    first, last = dc.overflow_neighbours()
    n_over = len(oracle_mod.surf_detect_and_compute(over, 0.0)[0])
    print("oracle keypoints of the overflowing frame:", n_over)
    assert n_over > kp_cap
    with pytest.raises(DVOError) as e:
        ops.surf_detect_and_compute(over, 0.0, ctx=gpu_ctx)
    assert e.value.code == DVO_ECAP
    ora = [oracle_mod.surf_detect_and_compute(f, 0.0) for f in (first, last)]
    counts = [len(k) for k, _ in ora]
    cap = 3800
    assert 4 <= counts[0] < cap and 4 <= counts[1] < cap < kp_cap, counts
    kps = torch.full((4, cap, KEYPOINT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    desc = torch.full((4, cap, 64), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((4, 2), -3, dtype=torch.int32, device="cuda")
    sb = ops.SurfBatch(w, h, 3, ctx=gpu_ctx)
    assert sb.list_cap == kp_cap
    frames = np.stack([first, over, last])
    sb.detect_device(frames, cap, 0.0, out=(kps, desc, cnt))
    torch.cuda.synchronize()
    kps, desc, cnt = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    assert cnt[1, 1] == 2 and cap < cnt[1, 0] <= kp_cap  # flagged; the count is of the list's part that was kept
    for slot, (ko, do) in ((0, ora[0]), (2, ora[1])):
        n = len(ko)
        assert cnt[slot, 0] == n and cnt[slot, 1] == 0
        np.testing.assert_array_equal(kps[slot, :n].reshape(-1), ko.view(np.uint8))
        np.testing.assert_array_equal(desc[slot, :n].view(np.uint32), do.view(np.uint32))
        assert (kps[slot, n:] == 0xAB).all() and (desc[slot, n:] == -7.0).all()
    assert (kps[3] == 0xAB).all() and (desc[3] == -7.0).all() and (cnt[3] == -3).all()  # behind the last slot
    with pytest.raises(DVOError) as e:
        sb.detect(frames, 0.0)
    assert e.value.code == DVO_ECAP
    _same(sb.detect(frames[[0, 2]], 0.0), ora)  # the handle works on
    sb.close()
