"""The mono input layouts the ORB path's ABI accepts: row pitch, base offset and frame stride of
dvo_stream_process / dvo_stream_submit, and the stride arguments of dvo_orb_detect_and_compute and
dvo_stream_pair.  Every other ORB stream test passes contiguous frames, and at the widths tested that are a
multiple of 16 the input pitch, the width and level 0's pitch are one number, so a kernel that used the wrong
one for level 0 would pass; process_frames' realign branch (a pointer, frame stride or pitch that is no
multiple of 4) is otherwise entered only by odd widths in the pyramid and FAST tests and never on submit,
where the slab is reused while earlier batches are in flight.

Each layout is a torch.as_strided view of a noise-filled buffer and must give the records (every field), the
features of every frame and the matches of every pair that the contiguous frames give; frame features are
also compared with oracle.detect_and_compute."""
import ctypes

import numpy as np
import pytest

from conftest import synth_frames

pytestmark = pytest.mark.gpu

W, H, NF, N = 320, 240, 300, 4


def _run(gpu_ctx, K, view, w):
    """One FrameStream.process of a [n, H, w] device view: (records, [features], [matches])."""
    from droplet_visual_odometry_amd.stream import FrameStream
    n = view.shape[0]
    fs = FrameStream(w, H, K, nfeatures=NF, max_frames=n, ctx=gpu_ctx)
    try:
        rec = fs.process(view)
        fs.sync()
        return (FrameStream.records_numpy(rec, n - 1), [fs.features(i) for i in range(n)],
                [fs.matches(p) for p in range(n - 1)])
    finally:
        fs.close()


def _view(frames, pitch, fstride, off, seed):
    """The frames as a strided device view of a noise-filled buffer (noise in every pad, before the base and
    in a tail after the last frame)."""
    import torch
    n, h, w = frames.shape
    host = np.random.default_rng(seed).integers(0, 256, off + n * fstride + 256, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(host[off:], (n, h, w), (fstride, pitch, 1))[...] = frames
    return torch.as_strided(torch.from_numpy(host).cuda(), (n, h, w), (fstride, pitch, 1), off)


def _same(got, want, label):
    rec, feats, matches = got
    rec_w, feats_w, matches_w = want
    assert rec.tobytes() == rec_w.tobytes(), label
    for i, ((k, d), (kw, dw)) in enumerate(zip(feats, feats_w)):
        assert k.tobytes() == kw.tobytes(), (label, "keypoints of frame", i)
        np.testing.assert_array_equal(d, dw, err_msg=f"{label}: descriptors of frame {i}")
    for p, (m, mw) in enumerate(zip(matches, matches_w)):
        assert m.tobytes() == mw.tobytes(), (label, "matches of pair", p)


@pytest.fixture(scope="module")
def ref(gpu_ctx, oracle_mod):
    """The contiguous 320-wide and 318-wide streams (computed once), their frame features checked against
    the oracle: frame 0 at 320, every frame at 318 (the contiguous 318-wide stream is itself realigned)."""
    import torch
    frames, K = synth_frames(W, H, range(N))
    crop = np.ascontiguousarray(frames[:, :, :318])
    out = {"frames": frames, "crop": crop, "K": K}
    for key, fr, which in ((320, frames, (0,)), (318, crop, range(N))):
        out[key] = _run(gpu_ctx, K, torch.from_numpy(fr).cuda(), fr.shape[2])
        assert np.all(out[key][0]["status"] == 0) and np.all(out[key][0]["n_matches"] > 20)
        for i in which:
            ko, do = oracle_mod.detect_and_compute(fr[i], NF)
            kg, dg = out[key][1][i]
            assert kg.tobytes() == ko.tobytes(), (key, i)
            np.testing.assert_array_equal(dg, do)
    return out


LAYOUTS = [  # (id, width, row pitch, frame stride, base offset)
    ("pitch324", 320, 324, 240 * 324 + 8, 0),        # aligned: the direct path with in_pitch != w != L[0].pitch
    ("pitch352", 320, 352, 240 * 352 + 8, 0),
    ("pitch321", 320, 321, 240 * 321, 0),            # realign
    ("base1", 320, 320, 240 * 320, 1),               # realign
    ("fstride+1", 320, 320, 240 * 320 + 1, 0),       # realign
    ("crop318-pitch320", 318, 320, 240 * 320, 0),    # the direct path at w mod 4 = 2
    ("crop318-pitch318", 318, 318, 240 * 318, 0),    # realign
]


@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_process_layout(gpu_ctx, ref, layout):
    name, w, pitch, fstride, off = layout
    frames = ref["frames"] if w == 320 else ref["crop"]
    direct = (pitch | fstride | off) & 3 == 0
    assert direct == (name in ("pitch324", "pitch352", "crop318-pitch320"))
    view = _view(frames, pitch, fstride, off, seed=pitch + off)
    assert view.data_ptr() % 4 == off
    _same(_run(gpu_ctx, ref["K"], view, w), ref[w], name)


def test_submit_realigned_batches(gpu_ctx, ref):
    """Three submit calls of realigned batches (pitch 321) and a drain equal the process calls of the
    contiguous batches: the realign copy of a batch lands in the slab while the batches before it are still
    in flight."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    frames, K = ref["frames"], ref["K"]
    orders = [[0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]]  # distinct batches
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=N, ctx=gpu_ctx)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=N, ctx=gpu_ctx)
    try:
        want = []
        for o in orders:
            r = a.process(torch.from_numpy(frames[o]).cuda())
            a.sync()
            want.append(FrameStream.records_numpy(r, N - 1))
        assert want[0].tobytes() == ref[320][0].tobytes()
        assert len({w.tobytes() for w in want}) == len(orders)
        views = [_view(frames[o], 321, 240 * 321, 0, seed=7 + i) for i, o in enumerate(orders)]
        recs = [b.new_records(N - 1) for _ in orders]
        torch.cuda.synchronize()
        retired = []
        for v, r in zip(views, recs):
            retired += b.submit(v, r)
        retired += b.drain()
        b.sync()
        assert [r.data_ptr() for r, _ in retired] == [r.data_ptr() for r in recs]
        for i, r in enumerate(recs):
            assert FrameStream.records_numpy(r, N - 1).tobytes() == want[i].tobytes(), i
    finally:
        a.close()
        b.close()


def test_detect_and_compute_row_strided(gpu_ctx, ref):
    """ops.detect_and_compute on a row-strided numpy view (the wrapper copies it), and the ABI's own stride
    argument (dvo_orb_detect_and_compute with stride w + 3 on the view's memory)."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import KEYPOINT_DTYPE, orb_params, ptr
    frame = ref["frames"][0]
    kw, dw = ref[320][1][0]
    wide = np.random.default_rng(5).integers(0, 256, (H, W + 3), dtype=np.uint8)
    wide[:, :W] = frame
    view = wide[:, :W]
    assert not view.flags.c_contiguous
    k, d = ops.detect_and_compute(view, NF, ctx=gpu_ctx)
    assert k.tobytes() == kw.tobytes()
    np.testing.assert_array_equal(d, dw)
    prm = orb_params(nfeatures=NF)
    cap = NF + 512
    kps, desc, n = np.zeros(cap, KEYPOINT_DTYPE), np.zeros((cap, 32), np.uint8), ctypes.c_int()
    gpu_ctx.check(gpu_ctx.lib.dvo_orb_detect_and_compute(gpu_ctx.h, ctypes.byref(prm), ptr(view), W, H, view.strides[0],
                                                         ptr(kps), ptr(desc), cap, ctypes.byref(n)))
    assert kps[:n.value].tobytes() == kw.tobytes()
    np.testing.assert_array_equal(desc[:n.value], dw)


def test_pair_row_strided(gpu_ctx, ref):
    """ops.PairStream.pair takes row-strided host images by copying them (np.ascontiguousarray) and always
    passes stride = width; the ABI's stride argument is exercised by calling dvo_stream_pair on the views'
    memory with stride w + 3.  Both records equal the contiguous pair's."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE, ptr
    frames, K = ref["frames"], ref["K"]
    wide = np.random.default_rng(6).integers(0, 256, (2, H, W + 3), dtype=np.uint8)
    wide[:, :, :W] = frames[:2]
    prev, cur = wide[0, :, :W], wide[1, :, :W]
    ps = ops.PairStream(W, H, K, nfeatures=NF, ctx=gpu_ctx)
    try:
        want = ps.pair(frames[0], frames[1])
        assert want["status"] == 0 and want["n_matches"] > 20
        assert ps.pair(prev, cur).tobytes() == want.tobytes()
        rec = np.zeros(1, PAIR_RECORD_DTYPE)
        gpu_ctx.check(gpu_ctx.lib.dvo_stream_pair(ps.h, ptr(prev), ptr(cur), prev.strides[0], 0, ptr(rec)))
        assert rec[0].tobytes() == want.tobytes()
    finally:
        ps.close()
