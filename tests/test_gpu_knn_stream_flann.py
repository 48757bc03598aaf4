"""stream.KnnFrameStream(matcher="flann"): the batched k-NN stream with every pair's kd-forest
built and searched on the device (dvo_knn_stream_set_flann).  Its records must equal
ops.KnnPairStream(matcher="flann").pair's chained through the returned theRNG state (n_hypotheses
aside), the oracle chain's, and must not depend on how the frames are split into calls; the
state skips pairs that build no forest."""
import numpy as np
import pytest

from conftest import synth_frames

pytestmark = pytest.mark.gpu

W, H, NF = 640, 480, 5
DETECTORS = ("sift", "surf")
SEED = 0xFFFFFFFF
_REF = {}


def _pair_chain(detector, frames, K, ctx, pairs, state=SEED):
    """(records, match lists, state) of the FLANN pair path over the (a, b) frame pairs, the state chained."""
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    ks = ops.KnnPairStream(frames.shape[2], frames.shape[1], K, detector=detector, matcher="flann", ctx=ctx)
    recs, matches = np.zeros(len(pairs), PAIR_RECORD_DTYPE), []
    for i, (a, b) in enumerate(pairs):
        recs[i], state = ks.pair(frames[a], frames[b], rng_state=state)
        matches.append(ks.matches())
    ks.close()
    return recs, matches, state


def _stream(detector, K, ctx, max_frames=NF, **kw):
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    kw.setdefault("matcher", "flann")
    return KnnFrameStream(W, H, K, max_frames, detector=detector, ctx=ctx, **kw)


def _run(st, frames):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    rec = st.process(d)
    st.sync()
    return st.records_numpy(rec, len(frames) - 1)


def _same(a, b, skip=()):
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    assert len(a) == len(b)
    for name in PAIR_RECORD_DTYPE.names:
        if name not in skip:
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def _ref(detector, ctx):
    """Once per detector: the pair path's chained records, match lists and final state of the 4
    consecutive pairs, and the stream's own one-call records, match lists and final state."""
    if detector not in _REF:
        frames, K = synth_frames(W, H, range(NF))
        recs, matches, state = _pair_chain(detector, frames, K, ctx, [(p, p + 1) for p in range(NF - 1)])
        counts = [int(recs["n_kp_prev"][0])] + [int(c) for c in recs["n_kp_cur"]]
        cap = max(counts) + 37  # above every count, no multiple of a tile
        st = _stream(detector, K, ctx, feat_cap=cap)
        own = _run(st, frames)
        own_matches = [st.matches(p) for p in range(NF - 1)]
        own_state = st.rng_state
        st.close()
        _REF[detector] = dict(frames=frames, K=K, counts=counts, recs=recs, matches=matches, state=state, cap=cap,
                              own=own, own_matches=own_matches, own_state=own_state)
    return _REF[detector]


@pytest.mark.parametrize("detector", DETECTORS)
def test_records_equal_the_chained_pair_path(gpu_ctx, detector):
    r = _ref(detector, gpu_ctx)
    assert (r["recs"]["status"] == 0).all() and (r["recs"]["n_matches"] >= 5).all()  # the frames do match
    _same(r["own"], r["recs"], skip=("n_hypotheses",))
    for p in range(NF - 1):
        np.testing.assert_array_equal(r["own_matches"][p].view(np.uint8), r["matches"][p].view(np.uint8))
    assert r["own_state"] == r["state"] != SEED


@pytest.mark.parametrize("detector", DETECTORS)
def test_first_record_equals_the_oracle_chain(gpu_ctx, oracle_mod, detector):
    from test_gpu_knn_pair import _oracle_features  # the oracle's detections, computed once per session
    r = _ref(detector, gpu_ctx)
    k1, d1 = _oracle_features(oracle_mod, detector, 0)
    k2, d2 = _oracle_features(oracle_mod, detector, 1)
    idx, dist, _ = oracle_mod.flann_knn(d1, d2, 2, trees=5, checks=50, rng_state=oracle_mod.THE_RNG_SEED)
    dist = np.sqrt(dist.astype(np.float32))
    keep = [q for q in range(len(d1)) if float(dist[q, 0]) < 0.75 * float(dist[q, 1])]
    p1 = np.stack([k1["x"][keep], k1["y"][keep]], 1).astype(np.float64)
    p2 = np.stack([k2["x"][idx[keep, 0]], k2["y"][idx[keep, 0]]], 1).astype(np.float64)
    E, _, _ = oracle_mod.find_essential(p1, p2, r["K"])
    rec = r["own"][0]
    assert rec["status"] == 0 and rec["n_models"] == 1
    np.testing.assert_array_equal(rec["E"].reshape(3, 3), E)
    assert (rec["n_kp_prev"], rec["n_kp_cur"], rec["n_matches"]) == (len(k1), len(k2), len(keep))
    m = r["own_matches"][0]
    np.testing.assert_array_equal(m["queryIdx"], keep)
    np.testing.assert_array_equal(m["trainIdx"], idx[keep, 0])
    np.testing.assert_array_equal(m["distance"].view(np.uint32), dist[keep, 0].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("detector", DETECTORS)
def test_records_do_not_depend_on_the_split(gpu_ctx, detector):
    r = _ref(detector, gpu_ctx)
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"])
    a = _run(st, r["frames"][0:3])
    b = _run(st, r["frames"][2:5])  # starts from the state the first call left
    _same(np.concatenate([a, b]), r["own"])  # every field, n_hypotheses too
    assert st.rng_state == r["own_state"]
    st.rng_state = SEED
    _same(_run(st, r["frames"]), r["own"])
    assert st.rng_state == r["own_state"]
    st.close()


@pytest.mark.parametrize("detector", DETECTORS)
def test_blank_frame_in_the_middle(gpu_ctx, detector):
    """Pairs 1 and 2 build no forest: pair 3 starts from the state pair 0 left."""
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT
    r = _ref(detector, gpu_ctx)
    frames = r["frames"].copy()
    frames[2] = 0
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"])
    rec = _run(st, frames)
    got_matches = [st.matches(p) for p in range(NF - 1)]
    got_state = st.rng_state
    st.close()
    assert (rec["status"][1:3] == DVO_ENOFEAT).all()
    assert (rec["n_kp_prev"][1], rec["n_kp_cur"][1]) == (r["counts"][1], 0)
    assert (rec["n_kp_prev"][2], rec["n_kp_cur"][2]) == (0, r["counts"][3])
    for name in ("R", "t", "E", "n_matches", "n_inliers", "n_good", "ransac_iters", "n_models", "n_hypotheses"):
        assert not np.any(rec[name][1:3]), name
    assert len(got_matches[1]) == 0 and len(got_matches[2]) == 0
    want, matches, state = _pair_chain(detector, frames, r["K"], gpu_ctx, [(0, 1), (3, 4)])
    _same(rec[[0, 3]], want, skip=("n_hypotheses",))
    np.testing.assert_array_equal(got_matches[0].view(np.uint8), matches[0].view(np.uint8))
    np.testing.assert_array_equal(got_matches[3].view(np.uint8), matches[1].view(np.uint8))
    assert got_state == state


@pytest.mark.parametrize("detector", DETECTORS)
def test_capacity(gpu_ctx, detector):
    from droplet_visual_odometry_amd._native import DVO_ECAP
    r = _ref(detector, gpu_ctx)
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=max(min(r["counts"]) - 1, 2))
    rec = _run(st, r["frames"])  # the call itself succeeds
    assert (rec["status"] == DVO_ECAP).all()
    assert not np.any(rec["n_matches"])
    assert st.rng_state == SEED  # no forest, no draw
    st.close()
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=max(r["counts"]))
    _same(_run(st, r["frames"]), r["own"])
    assert st.rng_state == r["own_state"]
    st.close()


@pytest.mark.parametrize("detector", DETECTORS)
def test_group_detection_gives_the_same_records(gpu_ctx, detector):
    r = _ref(detector, gpu_ctx)
    kw = dict(detect_group=2) if detector == "sift" else dict(surf_group=2)
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"], **kw)
    _same(_run(st, r["frames"]), r["own"])
    for p in range(NF - 1):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), r["own_matches"][p].view(np.uint8))
    assert st.rng_state == r["own_state"]
    st.close()


@pytest.mark.parametrize("detector", DETECTORS)
def test_setter_returns_to_bfmatcher(gpu_ctx, detector):
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    r = _ref(detector, gpu_ctx)
    bf = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"], matcher="bf")
    want = _run(bf, r["frames"])
    for call in (lambda: bf.rng_state, lambda: setattr(bf, "rng_state", 1)):
        with pytest.raises(DVOError) as e:
            call()
        assert e.value.code == DVO_EINVAL
    bf.close()
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"])
    assert st.matcher == "flann" and st.rng_state == SEED
    for trees, checks in ((65, 50), (-1, 50), (5, 0)):
        with pytest.raises(DVOError) as e:
            st.set_flann(trees, checks)
        assert e.value.code == DVO_EINVAL
    _same(_run(st, r["frames"]), r["own"])  # the refused calls changed nothing
    st.set_flann(0)
    assert st.matcher == "bf"
    _same(_run(st, r["frames"]), want)
    st.set_flann(5, 50)  # and back: a fresh thread's state again
    assert st.rng_state == SEED
    _same(_run(st, r["frames"]), r["own"])
    st.close()


@pytest.mark.parametrize("detector", DETECTORS)
def test_incoming_state(gpu_ctx, detector):
    r = _ref(detector, gpu_ctx)
    want, matches, state = _pair_chain(detector, r["frames"], r["K"], gpu_ctx, [(p, p + 1) for p in range(NF - 1)],
                                       state=0x1234567)
    st = _stream(detector, r["K"], gpu_ctx, feat_cap=r["cap"], rng_state=0x1234567)
    rec = _run(st, r["frames"])
    _same(rec, want, skip=("n_hypotheses",))
    for p in range(NF - 1):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), matches[p].view(np.uint8))
    assert st.rng_state == state != r["own_state"]
    st.close()
