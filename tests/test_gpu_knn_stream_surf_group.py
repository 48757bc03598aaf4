"""stream.KnnFrameStream(detector="surf", surf_group=G): the batched k-NN stream with SURF detection
(visual_odometry_v3.py:104, :373) through the group detector (dvo_knn_stream_set_surf_group), G
frames per launch straight into the stream's frame slots.  Features, records (every field,
n_hypotheses too) and match lists must equal the same stream's with the frame-by-frame detection
(surf_group=0), for every G and however the frames are split into calls."""
import numpy as np
import pytest

from conftest import synth_frames

pytestmark = pytest.mark.gpu

W, H, NF = 640, 480, 5
_REF = {}


def _stream(K, ctx, cap, detector="surf", **kw):
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    return KnnFrameStream(W, H, K, NF, detector=detector, feat_cap=cap, ctx=ctx, **kw)


def _run(st, frames):
    import torch
    rec = st.process(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    st.sync()
    return st.records_numpy(rec, len(frames) - 1)


def _same(a, b):
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    assert len(a) == len(b)
    for name in PAIR_RECORD_DTYPE.names:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def _ref(ctx):
    """Once: the 5 frames, the single-frame detector's features, and the records and match lists of
    the stream with surf_group=0."""
    if not _REF:
        from droplet_visual_odometry_amd import ops
        frames, K = synth_frames(W, H, range(NF))
        feats = [ops.surf_detect_and_compute(f, 400.0, ctx=ctx) for f in frames]
        cap = max(len(k) for k, _ in feats) + 37  # above every count, no multiple of a tile
        st = _stream(K, ctx, cap)
        assert st.surf_group == 0
        recs = _run(st, frames)
        matches = [st.matches(p) for p in range(NF - 1)]
        st.close()
        _REF.update(frames=frames, K=K, feats=feats, cap=cap, recs=recs, matches=matches)
    return _REF


@pytest.mark.parametrize("group", [1, 3, 8])
def test_group_detection_changes_nothing(gpu_ctx, group):
    r = _ref(gpu_ctx)
    assert (r["recs"]["status"] == 0).all() and (r["recs"]["n_matches"] >= 5).all()  # the frames do match
    st = _stream(r["K"], gpu_ctx, r["cap"], surf_group=group)
    assert st.surf_group == group
    recs = _run(st, r["frames"])
    for f in range(NF):
        k, d = st.features(f)
        assert len(k) == len(r["feats"][f][0]) >= 40
        np.testing.assert_array_equal(k.view(np.uint8), r["feats"][f][0].view(np.uint8))
        np.testing.assert_array_equal(d.view(np.uint32), r["feats"][f][1].view(np.uint32))
    _same(recs, r["recs"])  # every field, n_hypotheses too
    for p in range(NF - 1):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), r["matches"][p].view(np.uint8))
    # two calls, the third frame in both
    a = _run(st, r["frames"][0:3])
    b = _run(st, r["frames"][2:5])
    _same(np.concatenate([a, b]), r["recs"])
    st.close()


def test_setter_switches_on_a_live_stream(gpu_ctx):
    r = _ref(gpu_ctx)
    st = _stream(r["K"], gpu_ctx, r["cap"])
    st.set_surf_group(2)
    assert st.surf_group == 2
    _same(_run(st, r["frames"]), r["recs"])
    st.set_surf_group(0)
    assert st.surf_group == 0
    _same(_run(st, r["frames"]), r["recs"])
    st.close()


def test_sift_stream_rejects_the_setter_and_bad_groups(gpu_ctx):
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    r = _ref(gpu_ctx)
    st = _stream(r["K"], gpu_ctx, 4096, detector="sift")
    with pytest.raises(DVOError) as e:
        st.set_surf_group(2)
    assert e.value.code == DVO_EINVAL
    st.close()
    with pytest.raises(DVOError) as e:
        _stream(r["K"], gpu_ctx, 4096, detector="sift", surf_group=2)
    assert e.value.code == DVO_EINVAL
    st = _stream(r["K"], gpu_ctx, r["cap"])
    for bad in (-1, 65):
        with pytest.raises(DVOError) as e:
            st.set_surf_group(bad)
        assert e.value.code == DVO_EINVAL
    assert st.surf_group == 0
    st.close()
