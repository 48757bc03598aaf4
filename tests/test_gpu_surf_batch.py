"""The group SURF detector (dvo_surf_batch_detect / ops.SurfBatch): SURF_create(hessianThreshold)
.detectAndCompute (visual_odometry_v3.py:104, :373) of a stack of device-resident frames, one launch
per stage over a group of frames.  Every frame's keypoints and descriptors must equal the oracle's
(oracle/surf.cpp) and the single-frame detector's (ops.surf_detect_and_compute) bit for bit, whatever
the group, the threshold of the call, the row pitch and the frame stride; a frame over feat_cap is
marked and touches nothing of its neighbours."""
import numpy as np
import pytest

from conftest import synth_frames
from sift_batch_frames import CONSTANT, stack

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(oracle_mod, gpu_ctx, w, h, thr=100.0):
    """Once per size and threshold: the stack, the oracle's features and the single-frame detector's."""
    if (w, h, thr) not in _REF:
        from droplet_visual_odometry_amd import ops
        frames = stack(w, h)
        _REF[(w, h, thr)] = (frames, [oracle_mod.surf_detect_and_compute(f, thr) for f in frames],
                             [ops.surf_detect_and_compute(f, thr, ctx=gpu_ctx) for f in frames])
    return _REF[(w, h, thr)]


def _same(got, want):
    assert len(got) == len(want)
    for (kg, dg), (kw, dw) in zip(got, want):
        assert len(kg) == len(kw)
        np.testing.assert_array_equal(kg.view(np.uint8), kw.view(np.uint8))
        np.testing.assert_array_equal(dg.view(np.uint32), dw.view(np.uint32))


@pytest.mark.parametrize("wh", [(161, 97), (97, 61)])
def test_stack_equals_oracle_and_single_frame_detector(gpu_ctx, oracle_mod, wh):
    from droplet_visual_odometry_amd import ops
    w, h = wh
    frames, ora, single = _ref(oracle_mod, gpu_ctx, w, h)
    for f, (k, _) in enumerate(ora):  # the condition on the frames: no empty result can pass
        assert len(k) == 0 if f == CONSTANT else len(k) >= 40, (f, len(k))
    sb = ops.SurfBatch(w, h, 5, ctx=gpu_ctx)
    got = sb.detect(frames, 100.0)
    sb.close()
    assert len(got[CONSTANT][0]) == 0  # between two textured neighbours
    _same(got, ora)
    _same(got, single)


@pytest.mark.parametrize("wh", [(8, 8), (40, 30)])
def test_small_frames(gpu_ctx, oracle_mod, wh):
    """8 x 8: no layer fits, every list is empty.  40 x 30: empty frames beside lists of 1 and 3.
    Group 3 over 5 frames (chunks of 3 and 2)."""
    from droplet_visual_odometry_amd import ops
    w, h = wh
    frames, ora, single = _ref(oracle_mod, gpu_ctx, w, h)
    counts = [len(k) for k, _ in ora]
    assert max(counts) == 0 if wh == (8, 8) else (0 in counts and 0 < max(counts) <= 8), counts
    sb = ops.SurfBatch(w, h, 3, ctx=gpu_ctx)
    got = sb.detect(frames, 100.0)
    sb.close()
    _same(got, ora)
    _same(got, single)


@pytest.mark.parametrize("group", [1, 2, 5, 8])
def test_features_do_not_depend_on_the_group(gpu_ctx, oracle_mod, group):
    """Group 1, 2 (5 is no multiple), 5 and 8 (above the frame count)."""
    from droplet_visual_odometry_amd import ops
    frames, ora, single = _ref(oracle_mod, gpu_ctx, 161, 97)
    sb = ops.SurfBatch(161, 97, group, ctx=gpu_ctx)
    _same(sb.detect(frames, 100.0), ora)
    got = sb.detect(frames, 100.0)  # and again on the same handle: the counters are cleared per call
    sb.close()
    _same(got, ora)
    _same(got, single)


def test_threshold_belongs_to_the_call(gpu_ctx, oracle_mod):
    """One handle, thresholds 100, 400, 100 in turn: each call equals the oracle at its threshold."""
    from droplet_visual_odometry_amd import ops
    frames, ora100, single100 = _ref(oracle_mod, gpu_ctx, 161, 97, 100.0)
    _, ora400, single400 = _ref(oracle_mod, gpu_ctx, 161, 97, 400.0)
    n100, n400 = [len(k) for k, _ in ora100], [len(k) for k, _ in ora400]
    assert all(0 < b < a for f, (a, b) in enumerate(zip(n100, n400)) if f != CONSTANT), (n100, n400)
    sb = ops.SurfBatch(161, 97, 2, ctx=gpu_ctx)
    for thr, ora, single in ((100.0, ora100, single100), (400.0, ora400, single400), (100.0, ora100, single100)):
        got = sb.detect(frames, thr)
        _same(got, ora)
        _same(got, single)
    sb.close()


def test_row_pitch_and_frame_stride(gpu_ctx, oracle_mod):
    """A sliced tensor: row pitch 192 > w, frame stride (h + 3) rows > pitch * h."""
    import torch
    from droplet_visual_odometry_amd import ops
    w, h = 161, 97
    frames, ora, single = _ref(oracle_mod, gpu_ctx, w, h)
    slab = torch.full((5, h + 3, 192), 255, dtype=torch.uint8, device="cuda")
    view = slab[:, 2:2 + h, 7:7 + w]
    view.copy_(torch.from_numpy(frames).cuda())
    assert view.stride(1) == 192 and view.stride(0) == (h + 3) * 192
    sb = ops.SurfBatch(w, h, 2, ctx=gpu_ctx)
    got = sb.detect(view, 100.0)
    sb.close()
    _same(got, ora)
    _same(got, single)


@pytest.mark.parametrize("large_first", ["1", "0"])
def test_all_four_octaves(gpu_ctx, oracle_mod, monkeypatch, large_first):
    """640 x 480 scene frames at threshold 400: keypoints in every octave of every frame, so the large
    descriptor windows of octave 3 run; group 2 over 3 frames ends with a chunk of one frame.  With
    describe's large-window queue (the default: octaves 2 and 3 first, by ticket, whichever frame the
    wave is of) and with DVO_SURF_LARGE_FIRST=0 (read when the handle is made), the plain stride."""
    from droplet_visual_odometry_amd import ops
    if "octaves" not in _REF:
        frames, _ = synth_frames(640, 480, range(3))
        frames = np.stack(frames)
        _REF["octaves"] = (frames, [oracle_mod.surf_detect_and_compute(f, 400.0) for f in frames],
                           [ops.surf_detect_and_compute(f, 400.0, ctx=gpu_ctx) for f in frames])
    frames, ora, single = _REF["octaves"]
    for k, _ in ora:
        assert all((k["octave"] == o).sum() >= 1 for o in range(4)), np.bincount(k["octave"], minlength=4)
    monkeypatch.setenv("DVO_SURF_LARGE_FIRST", large_first)
    sb = ops.SurfBatch(640, 480, 2, ctx=gpu_ctx)
    got = sb.detect(frames, 400.0)
    sb.close()
    _same(got, ora)
    _same(got, single)


@pytest.mark.parametrize("order", [(1, 0, 2, 3, 4), (1, 2, 3, 4, 0)])
def test_capacity(gpu_ctx, oracle_mod, order):
    """feat_cap below frame 0's count (214) and above the others': frame 0, in the middle of a group
    or last in the stack, reports its true count; its slot holds its first feat_cap features, the
    other frames equal the oracle, and nothing is written past a frame's features: not in its slot,
    not in the next frame's, not behind the last slot."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_ECAP, KEYPOINT_DTYPE, DVOError
    w, h = 161, 97
    frames, ora, single = _ref(oracle_mod, gpu_ctx, w, h)
    counts = [len(k) for k, _ in ora]
    cap = counts[0] - 2
    assert all(c < cap for c in counts[1:]) and cap > 40
    n = len(order)
    kps = torch.full((n + 1, cap, KEYPOINT_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda")
    desc = torch.full((n + 1, cap, 64), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n + 1, 2), -3, dtype=torch.int32, device="cuda")
    sb = ops.SurfBatch(w, h, 3, ctx=gpu_ctx)
    sb.detect_device(frames[list(order)], cap, 100.0, out=(kps, desc, cnt))
    torch.cuda.synchronize()
    kps, desc, cnt = kps.cpu().numpy(), desc.cpu().numpy(), cnt.cpu().numpy()
    for slot, f in enumerate(order):
        assert cnt[slot, 0] == counts[f] and cnt[slot, 1] == 0  # the true count, over feat_cap for frame 0
        kept = min(counts[f], cap)
        for want in (ora, single):
            np.testing.assert_array_equal(kps[slot, :kept].reshape(-1), want[f][0][:kept].view(np.uint8))
            np.testing.assert_array_equal(desc[slot, :kept].view(np.uint32), want[f][1][:kept].view(np.uint32))
        assert (kps[slot, kept:] == 0xAB).all() and (desc[slot, kept:] == -7.0).all()
    assert (kps[n] == 0xAB).all() and (desc[n] == -7.0).all() and (cnt[n] == -3).all()  # behind the last slot
    with pytest.raises(DVOError) as e:
        sb.detect(frames[list(order)], 100.0, feat_cap=cap)
    assert e.value.code == DVO_ECAP
    sb.close()


def test_bad_arguments(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    for args in ((0, 8, 1), (8, 0, 1), (4096, 8, 1), (8, 4096, 1), (8, 8, 0), (8, 8, 65)):
        with pytest.raises(DVOError) as e:
            ops.SurfBatch(*args, ctx=gpu_ctx)
        assert e.value.code == DVO_EINVAL
    sb = ops.SurfBatch(8, 8, 2, ctx=gpu_ctx)
    lib, d = gpu_ctx.lib, torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    # n_frames < 1, feat_cap outside 1..surf_kp_cap(8, 8) = 4096, a threshold that is not >= 0
    for frames, cap, thr in ((d[:0], 16, 100.0), (d, 0, 100.0), (d, 4097, 100.0), (d, 16, -1.0), (d, 16, float("nan"))):
        with pytest.raises(DVOError) as e:
            sb.detect_device(frames, cap, thr)
        assert e.value.code == DVO_EINVAL
    # stride < w, null buffers, a null handle
    k, ds, c = sb.detect_device(d, 16, 100.0)
    args = [sb.h, d.data_ptr(), 2, 64, 8, 100.0, 16, k.data_ptr(), ds.data_ptr(), c.data_ptr()]
    for i, bad in ((4, 7), (1, None), (7, None), (8, None), (9, None), (0, None)):
        a = list(args)
        a[i] = bad
        assert lib.dvo_surf_batch_detect(*a) == DVO_EINVAL, i
    assert lib.dvo_surf_batch_detect(*args) == 0
    torch.cuda.synchronize()
    sb.close()
