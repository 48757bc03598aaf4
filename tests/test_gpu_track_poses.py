"""Track poses on the device (dvo_stream_set_track_poses, stream.TrackPoses): each pair's pose
refined on the previous pair's landmarks.  Every comparison is exact: status and counts equal, and
R, t, scale, rms bit-identical to the numpy restatement of the header's contract
(track_pose_cases.reference); links and scales are checked as test_gpu_tracks.py checks them."""
import numpy as np
import pytest

import track_cases as tc
import track_pose_cases as pc
from conftest import synth_frames

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
ORB_SIZES = [(320, 240, 300), (640, 480, 500)]
SMALL = ORB_SIZES[0]
FRAMES = 8
BLANK = 4


def _same_scales(got, want):
    assert list(got["n_common"]) == list(want["n_common"])
    assert list(got["n_prev"]) == list(want["n_prev"])
    for f in ("ratio", "q1", "q3"):  # bit for bit
        assert got[f].tobytes() == want[f].tobytes(), (f, got[f], want[f])


def _same_poses(got, want):
    for f in ("status", "iters", "n_used", "n_inliers"):
        assert list(got[f]) == list(want[f]), (f, list(got[f]), list(want[f]))
    for f in ("R", "t", "scale", "rms"):  # bit for bit
        for p in range(len(want)):
            assert got[f][p].tobytes() == want[f][p].tobytes(), (f, p, got[f][p], want[f][p])


def _hook(gpu_ctx, case, kp_cap, stride, cap_out=None, **params):
    """The hook on a case (lms, xy2, matches, recs); checks it against the restatement."""
    from droplet_visual_odometry_amd import ops
    lms, xy2, matches, recs = case[:4]
    want_links, want_sc, want, info = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN, **params)
    cap = max(max(len(a[0]) for a in lms), 1)
    lm, count, mq, mt, m = pc.pack(lms, xy2, matches, recs, cap, stride)
    co = cap if cap_out is None else cap_out
    link = np.full((len(lms), co), FILL32, np.int32)
    link, scale, pose = ops.test_track_poses(lm, count, mq, mt, m, recs, kp_cap, pc.K_CHAIN, cap_out=co, link=link,
                                             ctx=gpu_ctx, **params)
    _same_scales(scale, want_sc)
    for p, w in enumerate(want_links):
        n = min(len(w), co)
        np.testing.assert_array_equal(link[p, :n], w[:n], err_msg=str(p))
        assert (link[p, n:] == FILL32).all(), p
    _same_poses(pose, want)
    return want_sc, want, info


# ---- 1. the hook at sizes around min_points, a wave, the lane stride and the LDS limits ----------
# (matches, landmarks, n_common): landmark counts around 256 and 512 and above, so that a pair's
# correspondences come from several tiles
SPEC = [(600, 520, 0), (600, 300, 0), (600, 255, 2), (600, 256, 5), (600, 257, 6), (600, 511, 7), (600, 512, 63),
        (600, 513, 64), (650, 600, 65), (700, 640, 255), (700, 600, 256), (700, 650, 257), (700, 690, 513)]
STRIDE, KP_CAP = 700, 2200
# past the pose kernel's LDS limit (1024 correspondences) and the select kernel's (2048 ratios)
BIG = [(2400, 2300, 0), (2400, 2200, 1024), (2400, 2350, 1025), (2400, 2390, 2049)]
_CASES = {}


def _case(name):
    if name not in _CASES:
        if name == "sizes":
            _CASES[name] = pc.chain(SPEC, KP_CAP, seed=11, noise=0.3)
        elif name == "big":
            _CASES[name] = pc.chain(BIG, 7300, seed=12, noise=0.3, outliers=0.05)
        elif name == "small":
            _CASES[name] = pc.chain([(300, 280, 0), (300, 280, 200), (300, 270, 65), (300, 260, 3), (300, 280, 4)], 900,
                                    seed=13, noise=0.3)
    return _CASES[name]


def test_hook_sizes(gpu_ctx):
    sc, po, _ = _hook(gpu_ctx, _case("sizes"), KP_CAP, STRIDE)
    print("n_common", list(sc["n_common"]), "status", list(po["status"]), "scale", list(po["scale"]), "rms", list(po["rms"]))
    assert list(sc["n_common"]) == [-1] + [s[2] for s in SPEC[1:]]
    assert list(po["status"]) == [pc.NONE] * 4 + [pc.OK] * 9  # 0, 2 and 5 shared points are below min_points
    assert not po[1]["R"].any() and po[2]["R"].any() and po[3]["scale"] > 0 and (po["iters"][4:] == 10).all()


def test_hook_beyond_lds(gpu_ctx):
    sc, po, _ = _hook(gpu_ctx, _case("big"), 7300, 2400)
    assert list(sc["n_common"]) == [-1, 1024, 1025, 2049] and list(po["status"]) == [pc.NONE, pc.OK, pc.OK, pc.OK]
    assert (po["n_inliers"][1:] < po["n_used"][1:]).all()  # the outliers


# ---- 2. hook variations ------------------------------------------------------------------------
@pytest.mark.parametrize("iters", (1, 10, 32))
def test_hook_iters(gpu_ctx, iters):
    _, po, _ = _hook(gpu_ctx, _case("small"), 900, 300, iters=iters)
    assert list(po["iters"]) == [0, iters, iters, 0, 0]


def test_hook_min_points_and_defaults(gpu_ctx):
    _, po, _ = _hook(gpu_ctx, _case("small"), 900, 300, min_points=3)
    assert (po["status"][1:] != pc.NONE).all() and (po["iters"][3:] > 0).all()  # 3 and 4 shared points are fitted
    # zero and negative parameters mean the defaults
    from droplet_visual_odometry_amd import ops
    lms, xy2, matches, recs = _case("small")[:4]
    *_, want, _ = pc.reference(lms, xy2, matches, recs, pc.K_CHAIN)
    lm, count, mq, mt, m = pc.pack(lms, xy2, matches, recs, 280, 300)
    *_, pose = ops.test_track_poses(lm, count, mq, mt, m, recs, 900, pc.K_CHAIN, iters=0, huber_px=-1.0, inlier_px=0.0,
                                    min_points=0, ctx=gpu_ctx)
    _same_poses(pose, want)
    from droplet_visual_odometry_amd._native import DVOError
    for bad in (dict(iters=33), dict(min_points=2), dict(huber_px=float("nan"))):
        with pytest.raises(DVOError):
            ops.test_track_poses(lm, count, mq, mt, m, recs, 900, pc.K_CHAIN, ctx=gpu_ctx, **bad)


def test_hook_outliers_take_both_huber_branches(gpu_ctx):
    case = pc.chain([(600, 560, 0), (600, 560, 400), (600, 540, 300)], 1800, seed=14, noise=0.3, outliers=0.2)
    _, po, info = _hook(gpu_ctx, case, 1800, 600)
    for p in (1, 2):
        assert info[p]["quad"] > 0 and info[p]["lin"] > 0
        assert po[p]["status"] == pc.OK and po[p]["n_inliers"] < 0.9 * po[p]["n_used"]
    _hook(gpu_ctx, case, 1800, 600, huber_px=float("inf"))  # no Huber weight at all
    _hook(gpu_ctx, case, 1800, 600, huber_px=0.5, inlier_px=4.0)


def test_hook_points_behind_the_camera(gpu_ctx):
    case = pc.chain([(400, 380, 0), (400, 380, 300), (400, 370, 260)], 1200, seed=15, noise=0.3, behind=40)
    sc, po, _ = _hook(gpu_ctx, case, 1200, 400)
    for p in (1, 2):
        assert po[p]["status"] == pc.OK and 0 < po[p]["n_used"] < sc[p]["n_common"]


def test_hook_identical_points(gpu_ctx):
    _, po, _ = _hook(gpu_ctx, pc.identical_points(8), 8, 8)
    assert po[1]["status"] == pc.DEGENERATE and po[1]["iters"] == 0 and po[1]["scale"] == 1.0


def test_hook_failed_predecessor(gpu_ctx):
    case = pc.chain([(300, 280, 0), (300, 280, 200), (300, 0, 0), (300, 270, 0), (300, 260, 180)], 900, seed=16, noise=0.3)
    sc, po, _ = _hook(gpu_ctx, case, 900, 300)
    assert list(sc["n_prev"][2:4]) == [280, 0] and list(po["status"]) == [pc.NONE, pc.OK, pc.NONE, pc.NONE, pc.OK]
    assert not po[3]["R"].any() and not po[3]["t"].any() and po[3]["scale"] == 0


def test_hook_cap_out(gpu_ctx):
    """A caller's landmark cap of 16: the same poses."""
    _, a, _ = _hook(gpu_ctx, _case("small"), 900, 300)
    _, b, _ = _hook(gpu_ctx, _case("small"), 900, 300, cap_out=16)
    assert a.tobytes() == b.tobytes()


# ---- 3. the ORB stream -------------------------------------------------------------------------
def _filled(n_pairs, cap, device="cuda"):
    import torch
    from droplet_visual_odometry_amd.stream import Landmarks, TrackPoses, Tracks
    lm, tr, tp = Landmarks(n_pairs, cap, device), Tracks(n_pairs, cap, device), TrackPoses(n_pairs, device)
    for t in (lm.entries, lm.counts, tr.links, tr.scales, tp.poses):
        t.view(torch.uint8).fill_(FILL)
    return lm, tr, tp


def _stream_reference(fs, lm, tr, recs, n_pairs, **params):
    """The restatement fed with the stream's own landmarks (a Landmarks that holds every one),
    matches and records; the stream's links and scales are checked on the way."""
    lms, xy2, matches = [], [], []
    none = np.zeros(0, np.int32)
    for i in range(n_pairs):
        assert lm.count(i) <= lm.cap
        e = lm.numpy(i)
        lms.append((e["match"], np.stack([e["X"], e["Y"], e["Z"]], 1) if len(e) else np.zeros((0, 3))))
        xy2.append(np.stack([e["x2"], e["y2"]], 1) if len(e) else np.zeros((0, 2), np.float32))
        m = fs.matches(i) if len(e) else None
        matches.append((m["queryIdx"], m["trainIdx"]) if len(e) else (none, none))
    links, scales, poses, _ = pc.reference(lms, xy2, matches, recs, fs.K, **params)
    _same_scales(tr.scales_numpy(), scales)
    for p, w in enumerate(links):
        np.testing.assert_array_equal(tr.numpy(p, lm.count(p)), w, err_msg=str(p))
    return scales, poses


def _bind(fs, lm, tr, tp, **params):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.bind_track_poses(tp, **params)


_ORB = {}


def _orb(gpu_ctx, size):
    if size not in _ORB:
        import torch
        from droplet_visual_odometry_amd.stream import FrameStream
        W, H, NF = size
        frames, K = synth_frames(W, H, range(FRAMES))
        cap = NF + 37
        fs = FrameStream(W, H, K, nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
        lm, tr, tp = _filled(FRAMES - 1, cap)
        _bind(fs, lm, tr, tp)
        rec = fs.process(torch.from_numpy(frames).cuda())
        fs.sync()
        recs = FrameStream.records_numpy(rec, FRAMES - 1)
        _ORB[size] = dict(frames=frames, K=K, cap=cap, recs=recs, lm=lm, tr=tr, tp=tp, fs=fs,
                          want=_stream_reference(fs, lm, tr, recs, FRAMES - 1))
    return _ORB[size]


@pytest.mark.parametrize("size", ORB_SIZES)
def test_orb_stream_process(gpu_ctx, size):
    r = _orb(gpu_ctx, size)
    sc, want = r["want"]
    got = r["tp"].numpy()
    print(size, "n_common", list(sc["n_common"]), "ratio", list(sc["ratio"]), "scale", list(got["scale"]),
          "status", list(got["status"]), "inliers", list(got["n_inliers"]), "rms", list(got["rms"]))
    assert want[0]["status"] == pc.NONE and (want["status"][1:] == pc.OK).sum() >= 3
    _same_poses(got, want)


def test_orb_blank_frame(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    frames = r["frames"].copy()
    frames[BLANK] = 90
    fs = r["fs"]
    lm, tr, tp = _filled(FRAMES - 1, r["cap"])
    _bind(fs, lm, tr, tp)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, FRAMES - 1)
    sc, want = _stream_reference(fs, lm, tr, recs, FRAMES - 1)
    got = tp.numpy()
    print("status", list(recs["status"]), "n_common", list(sc["n_common"]), "pose status", list(got["status"]))
    for i in (BLANK - 1, BLANK, BLANK + 1):  # the pairs that touch the blank frame, and the one after them
        assert got[i]["status"] == pc.NONE and not got[i]["R"].any() and got[i]["scale"] == 0, i
    assert recs[BLANK]["status"] != 0 and recs[BLANK + 1]["status"] == 0
    assert (got["status"] == pc.OK).sum() >= 2
    _same_poses(got, want)


def test_orb_submit_equals_process(gpu_ctx):
    """Three batches submitted back to back, poses on the first two, equal the same batches
    processed one at a time, byte for byte."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = SMALL
    sizes, cap = [4, 3, 4], NF + 37
    starts = np.concatenate([[0], np.cumsum(np.array(sizes) - 1)])[:-1]
    frames, K = synth_frames(W, H, range(int(starts[-1] + sizes[-1])))
    dev = torch.from_numpy(frames).cuda()
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    want = []
    for k, (s0, m) in enumerate(zip(starts, sizes)):
        lm, tr, tp = _filled(m - 1, cap)
        a.bind_landmarks(lm)
        a.bind_tracks(tr)
        if k < 2:
            a.bind_track_poses(tp)
        rec = a.process(dev[s0:s0 + m])
        a.sync()
        recs = FrameStream.records_numpy(rec, m - 1)
        if k < 2:  # and the process side is right to begin with
            _same_poses(tp.numpy(), _stream_reference(a, lm, tr, recs, m - 1)[1])
        want.append((recs, lm, tr, tp))
    assert sum(int((w[3].numpy()["status"] == pc.OK).sum()) for w in want[:2]) >= 2
    bufs = [_filled(m - 1, cap) for m in sizes]
    recs = [b.new_records(m - 1) for m in sizes]
    torch.cuda.synchronize()
    for k, (s0, m, (lm, tr, tp), rec) in enumerate(zip(starts, sizes, bufs, recs)):
        b.bind_landmarks(lm)
        b.bind_tracks(tr)
        if k < 2:
            b.bind_track_poses(tp)
        b.submit(dev[s0:s0 + m], rec, wait_torch=False)
    b.drain()
    b.sync()
    for k, m in enumerate(sizes):
        lm, tr, tp = bufs[k]
        assert FrameStream.records_numpy(recs[k], m - 1).tobytes() == want[k][0].tobytes(), k
        for got, ref in ((lm.entries, want[k][1].entries), (lm.counts, want[k][1].counts), (tr.links, want[k][2].links),
                         (tr.scales, want[k][2].scales), (tp.poses, want[k][3].poses)):
            assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), k
    assert (bufs[2][2].poses.cpu().numpy() == FILL).all()  # the third batch bound no poses
    a.close()
    b.close()


def test_orb_one_shot_and_unbound_bytes(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    W, H, NF = SMALL
    dev = torch.from_numpy(r["frames"]).cuda()
    fs, cap, n = r["fs"], r["cap"], FRAMES - 1
    lib = fs.ctx.lib

    def untouched(tp):
        return (tp.poses.cpu().numpy() == FILL).all()

    def same(x, y):
        return x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()

    # a stream that never binds poses: a landmarks + tracks batch writes these bytes
    plain = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
    lm0, tr0, _ = _filled(n, cap)
    plain.bind_landmarks(lm0)
    plain.bind_tracks(tr0)
    rec0 = plain.process(dev)
    plain.sync()
    # the Landmarks and Tracks bytes and the records of the pose-bound batch are those
    for got, ref in ((r["lm"].entries, lm0.entries), (r["lm"].counts, lm0.counts), (r["tr"].links, tr0.links),
                     (r["tr"].scales, tr0.scales)):
        assert same(got, ref)
    assert r["recs"].tobytes() == FrameStream.records_numpy(rec0, n).tobytes()
    # one-shot: the batch after a bound one leaves a refilled TrackPoses alone and writes the same tracks
    lm, tr, tp = _filled(n, cap)
    _bind(fs, lm, tr, tp)
    fs.process(dev)
    fs.sync()
    assert same(tp.poses, r["tp"].poses)
    lm, tr, tp = _filled(n, cap)
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.process(dev)
    fs.sync()
    assert untouched(tp) and same(tr.scales, tr0.scales) and same(tr.links, tr0.links) and same(lm.entries, lm0.entries)
    # cleared by None, by a later bind_tracks, and with the landmark binding
    for clear in ("none", "tracks", "landmarks"):
        lm, tr, tp = _filled(n, cap)
        _bind(fs, lm, tr, tp)
        if clear == "none":
            fs.bind_track_poses(None)
        elif clear == "tracks":
            fs.bind_tracks(tr)
        else:
            fs.bind_landmarks(None)
        fs.process(dev)
        fs.sync()
        assert untouched(tp), clear
        assert same(tr.scales, tr0.scales) == (clear != "landmarks")
    # poses go with a pending Tracks that has a scale buffer
    lm, tr, tp = _filled(n, cap)
    with pytest.raises(ValueError):
        fs.bind_track_poses(tp)
    fs.bind_landmarks(lm)
    with pytest.raises(ValueError):
        fs.bind_track_poses(tp)
    assert lib.dvo_stream_set_track_poses(fs.h, tp.poses.data_ptr(), 0, 0.0, 0.0, 0) == DVO_EINVAL
    assert lib.dvo_stream_set_tracks(fs.h, tr.links.data_ptr(), None) == 0  # links only: no ratio to start from
    assert lib.dvo_stream_set_track_poses(fs.h, tp.poses.data_ptr(), 0, 0.0, 0.0, 0) == DVO_EINVAL
    fs.bind_tracks(tr)
    for bad in (dict(iters=33), dict(min_points=2), dict(inlier_px=float("nan"))):
        from droplet_visual_odometry_amd._native import DVOError
        with pytest.raises(DVOError):
            fs.bind_track_poses(tp, **bad)
    # other parameters reach the kernel
    fs.bind_track_poses(tp, iters=3, huber_px=2.0, inlier_px=1.0, min_points=3)
    rec = fs.process(dev)
    fs.sync()
    _, want = _stream_reference(fs, lm, tr, FrameStream.records_numpy(rec, n), n, iters=3, huber_px=2.0, inlier_px=1.0,
                                min_points=3)
    _same_poses(tp.numpy(), want)
    assert (want["iters"][want["status"] == pc.OK] == 3).all()
    # pairs that share no frame: refused, every binding consumed
    lm, tr, tp = _filled(n, cap)
    _bind(fs, lm, tr, tp)
    with pytest.raises(ValueError):
        fs.process_pairs(dev)
    rec = fs.new_records(4)
    torch.cuda.synchronize()
    assert lib.dvo_stream_process_pairs(fs.h, dev.data_ptr(), 4, dev.stride(0), dev.stride(1), rec.data_ptr()) == DVO_EINVAL
    fs._lm_next = fs._tr_next = fs._tp_next = None  # what the wrapper holds for the call it did not make
    fs.process(dev)
    fs.sync()
    assert untouched(tp) and (tr.scales.cpu().numpy() == FILL).all()
    plain.close()


# ---- 4. the k-NN stream ------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_knn_stream(gpu_ctx, detector):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    W, H, n, cap = 640, 480, 4, 4096
    frames, K = synth_frames(W, H, range(n))
    dev = torch.from_numpy(frames).cuda()
    st = KnnFrameStream(W, H, K, n, detector=detector, feat_cap=4096, ctx=gpu_ctx)
    lm, tr, tp = _filled(n - 1, cap)
    _bind(st, lm, tr, tp)
    rec = st.process(dev)
    st.sync()
    recs = st.records_numpy(rec, n - 1)
    assert (recs["status"] == 0).all()
    sc, want = _stream_reference(st, lm, tr, recs, n - 1)
    got = tp.numpy()
    print(detector, "n_common", list(sc["n_common"]), "ratio", list(sc["ratio"]), "scale", list(got["scale"]),
          "inliers", list(got["n_inliers"]), "rms", list(got["rms"]))
    assert list(want["status"]) == [pc.NONE, pc.OK, pc.OK]
    _same_poses(got, want)
    # the two-phase call: detect() leaves the bindings for finish()
    lm2, tr2, tp2 = _filled(n - 1, cap)
    _bind(st, lm2, tr2, tp2)
    st.detect(dev)
    st.finish()
    st.sync()
    assert tp2.poses.cpu().numpy().tobytes() == tp.poses.cpu().numpy().tobytes()
    assert tr2.scales.cpu().numpy().tobytes() == tr.scales.cpu().numpy().tobytes()
    # one-shot here too, and poses go with a pending Tracks
    tp2.poses.fill_(FILL)
    st.process(dev)
    st.sync()
    assert (tp2.poses.cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        st.bind_track_poses(tp2)
    assert st.ctx.lib.dvo_knn_stream_set_track_poses(st.h, tp2.poses.data_ptr(), 0, 0.0, 0.0, 0) == DVO_EINVAL
    st.close()
