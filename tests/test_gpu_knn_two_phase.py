"""KnnFrameStream.detect + finish (dvo_knn_stream_detect / dvo_knn_stream_finish): the two phases of
process, for SIFT and SURF with BFMatcher and FLANN.  Together they must give process's records,
match lists and final theRNG state byte for byte; the draws word is the plan's own count; and the
FLANN hand-off (shard_draws) on one GPU gives the records of a stream whose state was first moved
past the draws of the ranks below, and leaves the state past those of the ranks above."""
import numpy as np
import pytest

from conftest import synth_frames

pytestmark = pytest.mark.gpu

W, H, NF = 640, 480, 5
SEED = 0xFFFFFFFF
TREES, CHECKS = 5, 50
COMBOS = [(d, m) for d in ("sift", "surf") for m in ("bf", "flann")]
_COUNTS, _REF = {}, {}


def _stream(detector, matcher, K, ctx, cap, max_frames=NF, **kw):
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    return KnnFrameStream(W, H, K, max_frames, detector=detector, feat_cap=cap, ctx=ctx, matcher=matcher, **kw)


def feature_counts(detector, frames, K, ctx):
    """The detector's count per frame (a BF stream with room for every frame's features)."""
    st = _stream(detector, "bf", K, ctx, 4096, max_frames=len(frames))
    rec = st.process(_dev(frames))
    st.sync()
    rec = st.records_numpy(rec, len(frames) - 1)
    st.close()
    counts = [int(rec["n_kp_prev"][0])] + [int(c) for c in rec["n_kp_cur"]]
    assert 0 < max(counts) <= 4096
    return counts


def _dev(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def _same(a, b):
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    assert len(a) == len(b)
    for name in PAIR_RECORD_DTYPE.names:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert a.tobytes() == b.tobytes()


def _process(st, frames):
    rec = st.process(_dev(frames))
    st.sync()
    return st.records_numpy(rec, len(frames) - 1)


def _ref(detector, matcher, ctx):
    """Once per combination: process's records, match lists, final state and the frames' features."""
    key = detector, matcher
    if key not in _REF:
        frames, K = synth_frames(W, H, range(NF))
        if detector not in _COUNTS:
            _COUNTS[detector] = feature_counts(detector, frames, K, ctx)
        counts = _COUNTS[detector]
        cap = max(counts) + 37  # above every count, no multiple of a tile
        st = _stream(detector, matcher, K, ctx, cap)
        rec = _process(st, frames)
        assert (rec["status"] == 0).all() and (rec["n_matches"] >= 5).all()  # the frames do match
        _REF[key] = dict(frames=frames, K=K, counts=counts, cap=cap, rec=rec,
                         matches=[st.matches(p) for p in range(NF - 1)],
                         state=st.rng_state if matcher == "flann" else None)
        st.close()
    return _REF[key]


def _two_phase(st, frames, draws=None, **kw):
    st.detect(_dev(frames), draws=draws)
    rec = st.finish(**kw)
    st.sync()
    return st.records_numpy(rec, len(frames) - 1)


@pytest.mark.parametrize("detector,matcher", COMBOS)
def test_detect_then_finish_equals_process(gpu_ctx, detector, matcher):
    import torch
    r = _ref(detector, matcher, gpu_ctx)
    st = _stream(detector, matcher, r["K"], gpu_ctx, r["cap"])
    big = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    st.detect(_dev(r["frames"]), draws=big[1:2])  # a view into a larger tensor
    for f in (0, NF - 1):  # features() works between the phases
        kps, desc = st.features(f)
        assert len(kps) == r["counts"][f] and desc.shape == (r["counts"][f], st.dim)
    rec = st.finish()
    st.sync()
    _same(st.records_numpy(rec, NF - 1), r["rec"])  # every field, n_hypotheses too
    for p in range(NF - 1):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), r["matches"][p].view(np.uint8))
    want = sum(TREES * (2 * n - 1) for n in r["counts"][1:]) if matcher == "flann" else 0  # every pair builds
    assert big.cpu().tolist() == [-1, want, -1]
    if matcher == "flann":
        assert st.rng_state == r["state"] != SEED
    st.close()


@pytest.mark.parametrize("detector,matcher", COMBOS)
def test_finish_with_nothing_pending(gpu_ctx, detector, matcher):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    r = _ref(detector, matcher, gpu_ctx)
    st = _stream(detector, matcher, r["K"], gpu_ctx, r["cap"])
    junk = torch.full((NF * 256,), 0xAB, dtype=torch.uint8, device="cuda")
    for after_a_call in (False, True):
        if after_a_call:
            _same(_process(st, r["frames"]), r["rec"])
        with pytest.raises(DVOError) as e:
            st.finish(junk)
        assert e.value.code == DVO_EINVAL
        st.sync()
        assert (junk.cpu().numpy() == 0xAB).all()  # nothing was written
    np.testing.assert_array_equal(st.matches(0).view(np.uint8), r["matches"][0].view(np.uint8))
    if matcher == "flann":
        assert st.rng_state == r["state"]
    st.close()


@pytest.mark.parametrize("detector,matcher", COMBOS)
def test_setter_between_the_phases_drops_the_detection(gpu_ctx, detector, matcher):
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    r = _ref(detector, matcher, gpu_ctx)
    st = _stream(detector, matcher, r["K"], gpu_ctx, r["cap"])
    d = _dev(r["frames"])
    group = st.set_detect_group if detector == "sift" else st.set_surf_group
    flann = (lambda: st.set_flann(TREES, CHECKS)) if matcher == "flann" else (lambda: st.set_flann(0))
    for setter in (lambda: group(2), lambda: group(0), flann):
        st.detect(d)
        setter()
        with pytest.raises(DVOError) as e:
            st.finish()
        assert e.value.code == DVO_EINVAL
    if matcher == "flann":
        assert st.rng_state == SEED  # no plan ran
    st.detect(d)
    if matcher == "flann":
        st.rng_state = 0x1234567  # allowed between the phases, ordered before the plan
        st.rng_state = SEED
    rec = st.finish()
    st.sync()
    _same(st.records_numpy(rec, NF - 1), r["rec"])
    if matcher == "flann":
        assert st.rng_state == r["state"]
    st.close()


@pytest.mark.parametrize("detector,matcher", COMBOS)
def test_second_detect_replaces_the_first(gpu_ctx, detector, matcher):
    r = _ref(detector, matcher, gpu_ctx)
    st = _stream(detector, matcher, r["K"], gpu_ctx, r["cap"])
    st.detect(_dev(r["frames"][::-1][:3]))
    _same(_two_phase(st, r["frames"]), r["rec"])
    if matcher == "flann":
        assert st.rng_state == r["state"]
    st.close()


def _made_up_draws(ops):
    """Draw counts a and b of imagined ranks below and above, as synthetic train sizes, with the
    host plan that advances a state by them."""
    below, above = [50, 100, 57], [9, 31]  # 5 (2 * 100 - 1) + 5 (2 * 57 - 1) = 1560 draws; 5 (2 * 31 - 1) = 305
    return 1560, 305, (lambda s: ops.flann_rng_plan_host(below, 200, TREES, s)[1]), \
        (lambda s: ops.flann_rng_plan_host(above, 200, TREES, s)[1])


@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_flann_hand_off_on_one_gpu(gpu_ctx, oracle_mod, detector):
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    r = _ref(detector, "flann", gpu_ctx)
    a, b, jump_a, jump_b = _made_up_draws(ops)
    state_a = jump_a(SEED)
    assert state_a == oracle_mod.flann_rng_after(SEED, [100, 57], TREES)
    st = _stream(detector, "flann", r["K"], gpu_ctx, r["cap"], rng_state=state_a)
    want = _process(st, r["frames"])
    want_matches = [st.matches(p) for p in range(NF - 1)]
    want_state = jump_b(st.rng_state)
    assert want.tobytes() != r["rec"].tobytes()  # another state, other forests
    st.rng_state = SEED
    x = 2 ** 62 + 99  # junk: entry [rank] is not read
    shard = torch.tensor([a, x, b], dtype=torch.int64, device="cuda")
    d = _dev(r["frames"])
    st.detect(d)
    for rank in (-1, 3):
        with pytest.raises(DVOError) as e:
            st.finish(shard_draws=shard, rank=rank)
        assert e.value.code == DVO_EINVAL
    rec = st.finish(shard_draws=shard, rank=1)  # the refused calls left the detection pending
    st.sync()
    _same(st.records_numpy(rec, NF - 1), want)
    for p in range(NF - 1):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), want_matches[p].view(np.uint8))
    assert st.rng_state == want_state
    # rank 0 of 1 with an array: nothing before, nothing after
    st.rng_state = SEED
    _same(_two_phase(st, r["frames"], shard_draws=shard[1:2], rank=0), r["rec"])
    assert st.rng_state == r["state"]
    # a single pending frame has no pair and plans nothing, with or without the array
    st.rng_state = SEED
    st.detect(d[:1])
    st.finish(shard_draws=shard, rank=1)
    assert st.rng_state == SEED
    st.close()


@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_bf_stream_ignores_the_array(gpu_ctx, detector):
    import torch
    r = _ref(detector, "bf", gpu_ctx)
    st = _stream(detector, "bf", r["K"], gpu_ctx, r["cap"])
    shard = torch.tensor([1560, 2 ** 62 + 99, 305], dtype=torch.int64, device="cuda")
    _same(_two_phase(st, r["frames"], shard_draws=shard, rank=1), r["rec"])
    st.close()
