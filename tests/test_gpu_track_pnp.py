"""Track PnP on the device (dvo_stream_set_track_pnp, stream.TrackPnP): each pair's pose from a P3P
RANSAC on the previous pair's landmarks and the pair's raw matches.  Every comparison is exact
against the numpy restatement of the header's contract (track_pnp_cases.reference): the integers
equal, and R, t, scale, rms and the mask bit-identical."""
import numpy as np
import pytest

import track_pnp_cases as pn
import track_pose_cases as pc
from conftest import synth_frames

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
SMALL = (320, 240, 300)
FRAMES = 8
BLANK = 4
INTS = ("n_corr", "n_best", "n_used", "n_inliers", "sample", "solution", "iters", "status")


def _same_pnp(got, want):
    for f in INTS:
        assert list(got[f]) == list(want[f]), (f, list(got[f]), list(want[f]))
    for f in ("R", "t", "scale", "rms"):  # bit for bit
        for p in range(len(want)):
            assert got[f][p].tobytes() == want[f][p].tobytes(), (f, p, got[f][p], want[f][p])


def _same_masks(mask, masks, mask_cap):
    for p, w in enumerate(masks):
        n = min(len(w), mask_cap)
        np.testing.assert_array_equal(mask[p, :n], w[:n], err_msg=str(p))
        assert (mask[p, n:] == FILL).all(), p  # bytes outside the range are not touched


def _hook(gpu_ctx, c, kp_cap, stride, cap_out=None, mask_cap=None, **params):
    """The hook on a chain (track_pnp_cases.chain); checks it against the restatement."""
    from droplet_visual_odometry_amd import ops
    lms, xy2, matches, recs = c["lms"], c["xy2"], c["matches"], c["recs"]
    want, masks, info = pn.reference(lms, xy2, matches, recs, pn.K_CHAIN, **params)
    cap = max(max(len(a[0]) for a in lms), 1)
    lm, count, mq, mt, m, px = pn.pack(lms, xy2, matches, recs, cap, stride)
    mc = stride if mask_cap is None else mask_cap
    mask = np.full((len(lms), mc), FILL, np.uint8)
    *_, pose, pnp, mask = ops.test_track_pnp(lm, count, mq, mt, m, recs, kp_cap, pn.K_CHAIN, px, mask=mask,
                                             cap_out=cap_out, ctx=gpu_ctx, **params)
    _same_pnp(pnp, want)
    _same_masks(mask, masks, mc)
    return want, masks, pose, info


# ---- 1. the hook at sizes around min_points, a wave, a tile, the lane stride and the LDS limit -----
N_CORR = [0, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257]
SPEC = [(700, 650, 0)] + [(700, 500, n // 2) for n in N_CORR]
EXTRAS = [0] + [n - n // 2 for n in N_CORR]
STRIDE, KP_CAP = 700, 2200
# match lists of 2400: correspondences from ten tiles, at and past the 1024 the kernel keeps in LDS
BIG = [(2400, 2300, 0), (2400, 1300, 1024), (2400, 1300, 512), (2400, 1300, 512)]
BIG_EXTRAS = [0, 1025, 513, 512]
SMALL_SPEC = [(300, 280, 0), (300, 200, 100), (300, 200, 30), (300, 200, 2), (300, 200, 3)]
SMALL_EXTRAS = [0, 80, 35, 1, 1]
_CASES = {}


def _case(name):
    if name not in _CASES:
        if name == "sizes":
            _CASES[name] = pn.chain(SPEC, EXTRAS, KP_CAP, 21, outliers=0.3, noise=0.3)
        elif name == "big":
            _CASES[name] = pn.chain(BIG, BIG_EXTRAS, 7300, 22, outliers=0.4, noise=0.3)
        elif name == "small":
            _CASES[name] = pn.chain(SMALL_SPEC, SMALL_EXTRAS, 900, 23, outliers=0.3, noise=0.3)
    return _CASES[name]


def test_hook_sizes(gpu_ctx):
    want, *_ = _hook(gpu_ctx, _case("sizes"), KP_CAP, STRIDE)
    print("n_corr", list(want["n_corr"]), "status", list(want["status"]), "n_best", list(want["n_best"]),
          "inliers", list(want["n_inliers"]), "rms", list(want["rms"]))
    assert list(want["n_corr"]) == [0] + N_CORR
    assert list(want["status"][:6]) == [pn.NONE] * 6  # pair 0, and 0, 2, 3, 4, 5 correspondences are below min_points
    assert (want["status"][7:] == pn.OK).all() and (want["iters"][7:] == 10).all()


def test_hook_beyond_lds(gpu_ctx):
    want, *_ = _hook(gpu_ctx, _case("big"), 7300, 2400)
    assert list(want["n_corr"]) == [0, 2049, 1025, 1024] and list(want["status"]) == [pn.NONE, pn.OK, pn.OK, pn.OK]
    assert (want["n_inliers"][1:] < want["n_used"][1:]).all()  # the outliers


# ---- 2. hook variations ----------------------------------------------------------------------------
@pytest.mark.parametrize("hyps", (1, 63, 64, 65, 128, 512))
def test_hook_hyps(gpu_ctx, hyps):
    want, *_ = _hook(gpu_ctx, _case("small"), 900, 300, hyps=hyps)
    assert (want["sample"][1:3] < hyps).all()


@pytest.mark.parametrize("iters", (1, 10, 32))
def test_hook_iters(gpu_ctx, iters):
    want, *_ = _hook(gpu_ctx, _case("small"), 900, 300, iters=iters)
    assert list(want["iters"]) == [0, iters, iters, 0, 0]


def test_hook_min_points_defaults_and_einval(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    c = _case("small")
    want, *_ = _hook(gpu_ctx, c, 900, 300, min_points=4)
    assert want["n_corr"][4] == 4 and want["status"][4] != pn.NONE and want["status"][3] == pn.NONE
    # zero and negative parameters mean the defaults
    want, _, _ = pn.reference(c["lms"], c["xy2"], c["matches"], c["recs"], pn.K_CHAIN)
    lm, count, mq, mt, m, px = pn.pack(c["lms"], c["xy2"], c["matches"], c["recs"], 280, 300)
    *_, pnp, _ = ops.test_track_pnp(lm, count, mq, mt, m, c["recs"], 900, pn.K_CHAIN, px, hyps=0, iters=-1, huber_px=0.0,
                                    inlier_px=-1.0, min_points=0, seed=0, ctx=gpu_ctx)
    _same_pnp(pnp, want)
    for bad in (dict(hyps=513), dict(iters=33), dict(min_points=1), dict(min_points=3), dict(huber_px=float("nan")),
                dict(inlier_px=float("nan"))):
        with pytest.raises(DVOError):
            ops.test_track_pnp(lm, count, mq, mt, m, c["recs"], 900, pn.K_CHAIN, px, ctx=gpu_ctx, **bad)


def test_hook_huber_inf_and_seed(gpu_ctx):
    a, *_ = _hook(gpu_ctx, _case("small"), 900, 300, huber_px=float("inf"))
    b, *_ = _hook(gpu_ctx, _case("small"), 900, 300, seed=0x9E3779B97F4A7C15)
    c, *_ = _hook(gpu_ctx, _case("small"), 900, 300)
    assert list(b["sample"][1:3]) != list(c["sample"][1:3])  # other samples win under another seed
    assert (a["status"][1:3] == pn.OK).all()


def test_hook_behind_the_camera(gpu_ctx):
    c = pn.chain([(300, 280, 0), (300, 200, 100), (300, 200, 60)], [0, 80, 60], 900, 24, outliers=0.2, noise=0.3, behind=25)
    want, *_ = _hook(gpu_ctx, c, 900, 300)
    assert (want["n_used"][1:] < want["n_corr"][1:]).all() and (want["status"][1:] == pn.OK).all()


def test_hook_identical_points(gpu_ctx):
    c = pn.chain([(100, 80, 0), (100, 60, 20)], [0, 12], 400, 25, identical=True)
    want, *_ = _hook(gpu_ctx, c, 400, 100)
    assert want["n_corr"][1] == 32 and want["status"][1] in (pn.NO_MODEL, pn.DEGENERATE)


def test_hook_failed_middle_pair(gpu_ctx):
    """The middle pair's record failed and it has no landmarks: its track pose is NONE, its PnP pose is
    the truth within 1e-9 (noise-free, 30 % outliers), and the pair after it has no correspondences."""
    c = pn.chain([(300, 280, 0), (300, 0, 0), (300, 270, 0)], [0, 200, 0], 900, 26, outliers=0.3, fail=(1,))
    want, masks, pose, _ = _hook(gpu_ctx, c, 900, 300)
    assert list(want["status"]) == [pn.NONE, pn.OK, pn.NONE] and list(want["n_corr"]) == [0, 200, 0]
    assert list(pose["status"]) == [pc.NONE, pc.NONE, pc.NONE]
    R, t, good = c["truth"][1]
    assert np.abs(want["R"][1].reshape(3, 3) - R).max() <= 1e-9 and np.abs(want["t"][1] - t).max() <= 1e-9
    assert np.array_equal(np.flatnonzero(masks[1]), good) and len(good) == 140


def test_hook_mask_cap_and_cap_out(gpu_ctx):
    """A mask shorter than the match lists: the bytes past it are intact.  A caller's landmark cap of
    16: the same results."""
    a, *_ = _hook(gpu_ctx, _case("small"), 900, 300, mask_cap=100)
    b, *_ = _hook(gpu_ctx, _case("small"), 900, 300, cap_out=16)
    assert a.tobytes() == b.tobytes()


# ---- 3. the ORB stream -----------------------------------------------------------------------------
def _filled(n_pairs, cap, mask_cap, device="cuda"):
    import torch
    from droplet_visual_odometry_amd.stream import Landmarks, TrackPnP, TrackPoses, Tracks
    lm, tr, tp = Landmarks(n_pairs, cap, device), Tracks(n_pairs, cap, device), TrackPoses(n_pairs, device)
    pnp = TrackPnP(n_pairs, device, mask_cap=mask_cap)
    for t in (lm.entries, lm.counts, tr.links, tr.scales, tp.poses, pnp.pnp, pnp.mask):
        t.view(torch.uint8).fill_(FILL)
    return lm, tr, tp, pnp


def _stream_reference(fs, lm, recs, n_pairs, **params):
    """The restatement fed with the stream's own landmarks (a Landmarks that holds every one),
    matches, keypoints and records."""
    lms, xy2, matches = [], [], []
    for i in range(n_pairs):
        assert lm.count(i) <= lm.cap
        e = lm.numpy(i)
        lms.append((e["match"], np.stack([e["X"], e["Y"], e["Z"]], 1) if len(e) else np.zeros((0, 3))))
        m = fs.matches(i)
        assert len(m) == recs["n_matches"][i]
        kp = fs.features(i + 1)[0]
        px = np.stack([kp["x"][m["trainIdx"]], kp["y"][m["trainIdx"]]], 1).astype(np.float32)
        if len(e):  # the pixels the stream normalises are the keypoints': a landmark carries its match's
            assert np.array_equal(px[e["match"]], np.stack([e["x2"], e["y2"]], 1))
        xy2.append(px)
        matches.append((m["queryIdx"], m["trainIdx"]))
    return pn.reference(lms, xy2, matches, recs, fs.K, **params)


def _bind(fs, lm, tr, tp, pnp, **params):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.bind_track_poses(tp)
    fs.bind_pnp(pnp, **params)


def _check_stream(fs, lm, pnp, recs, n_pairs, mask_cap, **params):
    want, masks, _ = _stream_reference(fs, lm, recs, n_pairs, **params)
    _same_pnp(pnp.numpy(), want)
    _same_masks(pnp.mask_numpy(), masks, mask_cap)
    return want


_ORB = {}


def _orb(gpu_ctx):
    if not _ORB:
        import torch
        from droplet_visual_odometry_amd.stream import FrameStream
        W, H, NF = SMALL
        frames, K = synth_frames(W, H, range(FRAMES))
        frames = frames.copy()
        frames[BLANK] = 90
        cap = NF + 37
        fs = FrameStream(W, H, K, nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
        lm, tr, tp, pnp = _filled(FRAMES - 1, cap, cap)
        _bind(fs, lm, tr, tp, pnp)
        rec = fs.process(torch.from_numpy(frames).cuda())
        fs.sync()
        _ORB.update(frames=frames, K=K, cap=cap, recs=FrameStream.records_numpy(rec, FRAMES - 1), lm=lm, tr=tr, tp=tp,
                    pnp=pnp, fs=fs)
    return _ORB


def test_orb_stream_blank_frame(gpu_ctx):
    r = _orb(gpu_ctx)
    want = _check_stream(r["fs"], r["lm"], r["pnp"], r["recs"], FRAMES - 1, r["cap"])
    print("record status", list(r["recs"]["status"]), "n_corr", list(want["n_corr"]), "pnp status", list(want["status"]),
          "n_best", list(want["n_best"]), "inliers", list(want["n_inliers"]), "scale", list(want["scale"]))
    assert r["recs"][BLANK]["status"] != 0 and want[0]["status"] == pn.NONE
    assert want[BLANK + 1]["status"] == pn.NONE and want[BLANK + 1]["n_corr"] == 0  # its predecessor has no landmarks
    assert (want["status"] == pn.OK).sum() >= 2


def test_orb_submit_equals_process_and_unbound_bytes(gpu_ctx):
    """Submitted batches equal processed ones byte for byte; the binding is one-shot; and every other
    output of a batch, and its records, are those of a stream that never bound PnP."""
    import torch
    from droplet_visual_odometry_amd.stream import (FrameStream, Landmarks, RefinedLandmarks, TrackBundle, TrackPnP,
                                                    TrackPoses, Tracks)
    r = _orb(gpu_ctx)
    W, H, NF = SMALL
    cap, n = r["cap"], FRAMES - 1
    dev = torch.from_numpy(r["frames"]).cuda()

    def run(fs, with_pnp, submit):
        lm, tr, tp, pnp = _filled(n, cap, cap)
        rf, bd = RefinedLandmarks(n, cap, "cuda"), TrackBundle(n, cap, "cuda")
        for t in (rf.refined, rf.ids, bd.bundle, bd.points):
            t.fill_(FILL)
        fs.bind_landmarks(lm)
        fs.bind_tracks(tr)
        fs.bind_track_poses(tp)
        fs.bind_refine(rf)
        fs.bind_bundle(bd)
        if with_pnp:
            fs.bind_pnp(pnp)
        if submit:
            rec = fs.new_records(n)
            torch.cuda.synchronize()
            fs.submit(dev, rec, wait_torch=False)
            fs.drain()
        else:
            rec = fs.process(dev)
        fs.sync()
        outs = [lm.entries, lm.counts, tr.links, tr.scales, tp.poses, rf.refined, rf.ids, bd.bundle, bd.points]
        return [t.cpu().numpy().tobytes() for t in outs] + [FrameStream.records_numpy(rec, n).tobytes()], pnp

    plain = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
    base, untouched = run(plain, False, False)
    assert (untouched.pnp.cpu().numpy() == FILL).all() and (untouched.mask.cpu().numpy() == FILL).all()
    fs = r["fs"]
    got, pnp = run(fs, True, False)
    assert got == base  # the pose, refine and bundle setters did not clear it, and it changed none of their bytes
    assert pnp.pnp.cpu().numpy().tobytes() == r["pnp"].pnp.cpu().numpy().tobytes()
    assert pnp.mask.cpu().numpy().tobytes() == r["pnp"].mask.cpu().numpy().tobytes()
    got, sub = run(fs, True, True)
    assert got == base
    assert sub.pnp.cpu().numpy().tobytes() == pnp.pnp.cpu().numpy().tobytes()
    assert sub.mask.cpu().numpy().tobytes() == pnp.mask.cpu().numpy().tobytes()
    # one-shot, and cleared by None, by a later bind_tracks and with the landmark binding
    for clear in ("next", "none", "tracks", "landmarks"):
        lm, tr, tp, p2 = _filled(n, cap, cap)
        if clear != "next":
            _bind(fs, lm, tr, tp, p2)
        if clear == "none":
            fs.bind_pnp(None)
        elif clear == "tracks":
            fs.bind_tracks(tr)
        elif clear == "landmarks":
            fs.bind_landmarks(None)
        fs.process(dev)
        fs.sync()
        assert (p2.pnp.cpu().numpy() == FILL).all() and (p2.mask.cpu().numpy() == FILL).all(), clear
    # it goes with a pending Tracks; either of its buffers will do
    lm, tr, tp, p2 = _filled(n, cap, cap)
    with pytest.raises(ValueError):
        fs.bind_pnp(p2)
    fs.bind_landmarks(lm)
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    lib = fs.ctx.lib
    assert lib.dvo_stream_set_track_pnp(fs.h, p2.pnp.data_ptr(), None, 0, 0, 0, 0.0, 0.0, 0, 0) == DVO_EINVAL
    assert lib.dvo_stream_set_tracks(fs.h, tr.links.data_ptr(), None) == 0
    assert lib.dvo_stream_set_track_pnp(fs.h, p2.pnp.data_ptr(), None, 0, 0, 0, 0.0, 0.0, 0, 0) == 0
    assert lib.dvo_stream_set_track_pnp(fs.h, p2.pnp.data_ptr(), p2.mask.data_ptr(), 0, 0, 0, 0.0, 0.0, 0, 0) == DVO_EINVAL
    fs.bind_tracks(tr)
    for bad in (dict(hyps=513), dict(iters=33), dict(min_points=3), dict(inlier_px=float("nan"))):
        with pytest.raises(DVOError):
            fs.bind_pnp(p2, **bad)
    # other parameters reach the kernels
    params = dict(hyps=65, iters=3, huber_px=2.0, inlier_px=1.0, min_points=4, seed=7)
    fs.bind_pnp(p2, **params)
    rec = fs.process(dev)
    fs.sync()
    _check_stream(fs, lm, p2, FrameStream.records_numpy(rec, n), n, cap, **params)
    # pairs that share no frame: refused with the tracks
    lm, tr, tp, p2 = _filled(n, cap, cap)
    _bind(fs, lm, tr, tp, p2)
    with pytest.raises(ValueError):
        fs.process_pairs(dev)
    fs._lm_next = fs._tr_next = fs._tp_next = fs._pn_next = None  # what the wrapper holds for the call it did not make
    fs.bind_landmarks(None)
    plain.close()


# ---- 4. the k-NN stream ------------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_knn_stream(gpu_ctx, detector):
    import torch
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    W, H, n, cap = 640, 480, 4, 4096
    frames, K = synth_frames(W, H, range(n))
    dev = torch.from_numpy(frames).cuda()
    st = KnnFrameStream(W, H, K, n, detector=detector, feat_cap=4096, ctx=gpu_ctx)
    lm, tr, tp, pnp = _filled(n - 1, cap, cap)
    _bind(st, lm, tr, tp, pnp)
    rec = st.process(dev)
    st.sync()
    recs = st.records_numpy(rec, n - 1)
    assert (recs["status"] == 0).all()
    want = _check_stream(st, lm, pnp, recs, n - 1, cap)
    print(detector, "n_corr", list(want["n_corr"]), "n_best", list(want["n_best"]), "inliers", list(want["n_inliers"]),
          "scale", list(want["scale"]), "pose scale", list(tp.numpy()["scale"]))
    assert list(want["status"]) == [pn.NONE, pn.OK, pn.OK]
    # the two-phase call: detect() leaves the binding for finish()
    lm2, tr2, tp2, pnp2 = _filled(n - 1, cap, cap)
    _bind(st, lm2, tr2, tp2, pnp2)
    st.detect(dev)
    st.finish()
    st.sync()
    assert pnp2.pnp.cpu().numpy().tobytes() == pnp.pnp.cpu().numpy().tobytes()
    assert pnp2.mask.cpu().numpy().tobytes() == pnp.mask.cpu().numpy().tobytes()
    assert tp2.poses.cpu().numpy().tobytes() == tp.poses.cpu().numpy().tobytes()
    # one-shot here too, and it goes with a pending Tracks
    pnp2.pnp.fill_(FILL)
    st.process(dev)
    st.sync()
    assert (pnp2.pnp.cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        st.bind_pnp(pnp2)
    st.close()


def test_carry_scale_bridges_the_failed_pair(gpu_ctx):
    """carry_scale(pnp=) on a hook chain whose middle pair failed: the scale crosses it on the host."""
    from droplet_visual_odometry_amd.stream import carry_scale
    from droplet_visual_odometry_amd import ops
    c = pn.chain([(300, 280, 0), (300, 0, 0), (300, 270, 0)], [0, 200, 0], 900, 26, outliers=0.3, fail=(1,))
    lm, count, mq, mt, m, px = pn.pack(c["lms"], c["xy2"], c["matches"], c["recs"], 280, 300)
    _, scale, pose, pnp, _ = ops.test_track_pnp(lm, count, mq, mt, m, c["recs"], 900, pn.K_CHAIN, px, ctx=gpu_ctx)
    anchor = np.array([2.0, np.nan, np.nan])
    plain = carry_scale(anchor, scale, poses=pose)
    assert np.array_equal(plain, carry_scale(anchor, scale, poses=pose, pnp=None), equal_nan=True)
    assert plain[0] == 2.0 and np.isnan(plain[1:]).all()
    out = carry_scale(anchor, scale, poses=pose, pnp=pnp)
    assert out[1] == 2.0 * pnp["scale"][1] and abs(out[1] - 2.0 * np.linalg.norm(c["truth"][1][1])) <= 1e-8
    assert np.isnan(out[2])  # the pair after the failed one has no correspondences: out of scope
