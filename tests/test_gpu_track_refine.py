"""Track ids and refined landmarks on the device (dvo_stream_set_track_refine,
stream.RefinedLandmarks).  Every comparison is exact: ids, views, counts, iters and status equal,
and X, Y, Z, rms bit-identical to the numpy restatement of the header's contract
(track_refine_cases.reference); links, scales and poses are checked as test_gpu_track_poses.py
checks them."""
import numpy as np
import pytest

import track_pose_cases as pc
import track_refine_cases as rc
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


def _same_refined(got, want, where=""):
    for f in ("views", "n_used", "n_inliers", "iters", "status", "reserved"):
        assert list(got[f]) == list(want[f]), (where, f, list(got[f]), list(want[f]))
    for f in ("X", "Y", "Z", "rms"):  # bit for bit
        assert got[f].tobytes() == want[f].tobytes(), (where, f, got[f], want[f])


def _filled_out(P, co):
    from droplet_visual_odometry_amd._native import LANDMARK_REFINED_DTYPE, TRACK_ID_DTYPE
    refined = np.frombuffer(bytes([FILL]) * (P * co * 56), LANDMARK_REFINED_DTYPE).reshape(P, co).copy()
    ids = np.frombuffer(bytes([FILL]) * (P * co * 16), TRACK_ID_DTYPE).reshape(P, co).copy()
    return refined, ids


def _hook(gpu_ctx, case, kp_cap, stride, cap_out=None, use_poses=False, want_refined=True, want_ids=True, **params):
    """The hook on a case (lms, xy1, xy2, matches, recs); checks everything against the restatement."""
    from droplet_visual_odometry_amd import ops
    lms, xy1, xy2, matches, recs = case[:5]
    P = len(lms)
    links, scales, poses, refined, ids, info = rc.reference(lms, xy1, xy2, matches, recs, pc.K_CHAIN,
                                                            use_poses=use_poses, **params)
    cap = max(max(len(a[0]) for a in lms), 1)
    lm, count, mq, mt, m = rc.pack(lms, xy1, xy2, matches, recs, cap, stride)
    co = cap if cap_out is None else cap_out
    link = np.full((P, co), FILL32, np.int32)
    g_ref, g_ids = _filled_out(P, co)
    link, scale, pose, g_ref, g_ids = ops.test_track_refine(
        lm, count, mq, mt, m, recs, kp_cap, pc.K_CHAIN, use_poses=use_poses, cap_out=co, link=link, refined=g_ref,
        ids=g_ids, want_refined=want_refined, want_ids=want_ids, ctx=gpu_ctx, **params)
    _same_scales(scale, scales)
    _same_poses(pose, poses)
    for p in range(P):
        n = min(len(links[p]), co)
        np.testing.assert_array_equal(link[p, :n], links[p][:n], err_msg=str(p))
        assert (link[p, n:] == FILL32).all(), p
        if want_ids:
            assert g_ids[p, :n].tobytes() == ids[p][:n].tobytes(), (p, g_ids[p, :n], ids[p][:n])
            assert (g_ids[p, n:].view(np.uint8) == FILL).all(), p
        if want_refined:
            _same_refined(g_ref[p, :n], refined[p][:n], p)
            assert (g_ref[p, n:].view(np.uint8) == FILL).all(), p
    return dict(links=links, scales=scales, poses=poses, refined=refined, ids=ids, info=info, got=(g_ref, g_ids))


def _ages(r):
    return sorted({int(a) for i in r["ids"] for a in i["age"]})


# ---- 1. the hook: sizes ------------------------------------------------------------------------
# landmark counts 1, 63, 64, 65, 255, 256, 257 and 513 with every n_common of the list, the chains
# hopping between tiles: (matches, landmarks, n_common)
SPEC = [(600, 520, 0), (600, 513, 257), (600, 257, 256), (600, 256, 255), (600, 255, 65), (600, 65, 64), (600, 64, 63),
        (600, 63, 2), (600, 300, 1), (600, 1, 0), (600, 400, 1), (600, 513, 257)]
STRIDE, KP_CAP = 600, 1900
_CASES = {}


def _case(name):
    if name not in _CASES:
        if name == "sizes":
            _CASES[name] = rc.scene_chain(SPEC, KP_CAP, seed=21, noise=0.3, rot_sigma=0.003, dlt=True)
        elif name == "small":
            _CASES[name] = rc.scene_chain([(300, 280, 0)] + [(300, 280, 200), (300, 270, 180)] * 5, 900, seed=22,
                                          noise=0.3, rot_sigma=0.003, dlt=True)
    return _CASES[name]


def test_hook_sizes(gpu_ctx):
    r = _hook(gpu_ctx, _case("sizes"), KP_CAP, STRIDE)
    assert list(r["scales"]["n_common"]) == [-1] + [s[2] for s in SPEC[1:]]
    print("views", list(r["info"]["views"]), "ages", _ages(r), "huber", r["info"]["quad"], r["info"]["lin"])
    assert r["info"]["views"][3:7].all() and r["info"]["quad"] and r["info"]["lin"]
    assert any((x["status"] == rc.OK).sum() >= 200 for x in r["refined"])


@pytest.mark.parametrize("views", (3, 6, 8))
@pytest.mark.parametrize("use_poses", (False, True))
def test_hook_window(gpu_ctx, views, use_poses):
    """Chains shorter than, equal to and longer than the window; motions from records only, and
    from the poses where they are OK (pair 0 and the pairs of an 11-pair chain whose poses are NONE
    at min_points 190 fall back to the records)."""
    r = _hook(gpu_ctx, _case("small"), 900, 300, views=views, use_poses=use_poses, pose_params=(10, 1.0, 2.0, 190))
    hist = r["info"]["views"]
    assert hist[2] and hist[3] and hist[views] and not hist[views + 1:].any(), list(hist)
    st = list(r["poses"]["status"])
    assert pc.OK in st[1:] and pc.NONE in st[1:]
    assert max(_ages(r)) == 10 > views


@pytest.mark.parametrize("pairs", (1, 2, 3, 4, 5, 8, 9, 16, 17, 33))
def test_hook_ids_every_round(gpu_ctx, pairs):
    """Tracks of every age up to pairs - 1, starting and ending at different pairs: the ages 2^r - 1,
    2^r and 2^r + 1 on both sides of every jumping round."""
    r0 = np.random.RandomState(pairs)
    spec = [(120, 100, 0)] + [(120, 100, int(r0.randint(20, 45))) for _ in range(pairs - 1)]
    max_age = pairs - 2 if pairs % 2 == 0 and pairs > 2 else None  # the even batches also end their oldest tracks
    case = rc.scene_chain(spec, 400, seed=30 + pairs, noise=0.3, max_age=max_age)
    r = _hook(gpu_ctx, case, 400, 120, views=6)
    ages = _ages(r)
    assert ages == list(range((pairs - 1 if max_age is None else max_age) + 1)), ages
    roots = {int(x) for i in r["ids"] for x in i["root_pair"][i["age"] > 0]}
    assert pairs < 8 or len(roots) >= 2


def test_hook_empty_pair_cuts_chains_and_windows(gpu_ctx):
    spec = [(300, 280, 0), (300, 280, 200), (300, 280, 200), (300, 0, 0), (300, 270, 0), (300, 260, 180), (300, 260, 180)]
    r = _hook(gpu_ctx, rc.scene_chain(spec, 900, seed=23, noise=0.3), 900, 300, views=8)
    assert (r["refined"][4]["status"] == rc.NONE).all() and r["refined"][5]["views"].max() == 3
    assert r["refined"][6]["views"].max() == 4 and r["refined"][2]["views"].max() == 4
    assert max(_ages(r)) == 2


def test_hook_duplicate_train_indices(gpu_ctx):
    spec = [(300, 280, 0)] + [(300, 280, 150)] * 4
    r = _hook(gpu_ctx, rc.scene_chain(spec, 900, seed=24, noise=0.3, dups=60), 900, 300)
    assert max(_ages(r)) == 4


def test_hook_cap_out(gpu_ctx):
    """A caller's cap of 16 under counts in the hundreds: the first 16 slots of the full run."""
    full = _hook(gpu_ctx, _case("small"), 900, 300)
    capped = _hook(gpu_ctx, _case("small"), 900, 300, cap_out=16)
    for got_f, got_c in zip(full["got"], capped["got"]):
        assert got_f[:, :16].tobytes() == got_c.tobytes()
    ids = capped["got"][1]
    assert (ids["root_ord"] >= 16).any() and any((l[:16] >= 16).any() for l in capped["links"])


@pytest.mark.parametrize("iters", (1, 5, 16))
def test_hook_iters(gpu_ctx, iters):
    r = _hook(gpu_ctx, _case("small"), 900, 300, iters=iters)
    for x in r["refined"][1:]:
        assert (x["iters"][x["status"] == rc.OK] == iters).all() and (x["status"] == rc.OK).any()


def test_hook_defaults_and_ranges(gpu_ctx):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    lms, xy1, xy2, matches, recs = _case("small")[:5]
    want = rc.reference(lms, xy1, xy2, matches, recs, pc.K_CHAIN)[3]
    lm, count, mq, mt, m = rc.pack(lms, xy1, xy2, matches, recs, 280, 300)
    *_, got, _ = ops.test_track_refine(lm, count, mq, mt, m, recs, 900, pc.K_CHAIN, views=0, iters=-1, huber_px=0.0,
                                       inlier_px=-2.0, ctx=gpu_ctx)
    for p, w in enumerate(want):
        _same_refined(got[p, :len(w)], w, p)
    for bad in (dict(views=9), dict(views=2), dict(views=1), dict(iters=17), dict(huber_px=float("nan")),
                dict(inlier_px=float("nan"))):
        with pytest.raises(DVOError):
            ops.test_track_refine(lm, count, mq, mt, m, recs, 900, pc.K_CHAIN, ctx=gpu_ctx, **bad)


def test_hook_outliers_take_both_huber_branches(gpu_ctx):
    spec = [(300, 280, 0)] + [(300, 280, 220)] * 5
    case = rc.scene_chain(spec, 900, seed=25, noise=0.3, outliers=0.2, dlt=True)
    r = _hook(gpu_ctx, case, 900, 300)
    assert r["info"]["quad"] > 0 and r["info"]["lin"] > 0
    assert any((x["n_inliers"] < x["n_used"]).any() for x in r["refined"])
    r = _hook(gpu_ctx, case, 900, 300, huber_px=float("inf"))  # no Huber weight at all
    assert r["info"]["lin"] == 0
    _hook(gpu_ctx, case, 900, 300, huber_px=0.5, inlier_px=4.0)


def test_hook_views_behind_the_camera(gpu_ctx):
    spec = [(300, 280, 0)] + [(300, 280, 220)] * 4
    r = _hook(gpu_ctx, rc.scene_chain(spec, 900, seed=26, noise=0.3, behind=40), 900, 300)
    assert any(((x["n_used"] < x["views"]) & (x["status"] != rc.NONE)).any() for x in r["refined"])


def test_hook_one_ray(gpu_ctx):
    r = _hook(gpu_ctx, rc.one_ray(4, 3), 4, 4)
    for p in (1, 2):
        x = r["refined"][p]
        assert (x["status"] == rc.DEGENERATE).all() and (x["iters"] == 0).all() and (x["Z"] == 5.0).all()
        assert (x["views"] == p + 2).all() and (x["n_used"] == p + 2).all()


def test_hook_ratio_not_positive_ends_the_window(gpu_ctx):
    """A pair that links nothing has ratio 0.0: the windows of the pairs after it stop there."""
    spec = [(300, 280, 0), (300, 280, 200), (300, 280, 0), (300, 270, 200), (300, 260, 180)]
    r = _hook(gpu_ctx, rc.scene_chain(spec, 900, seed=27, noise=0.3), 900, 300, views=8)
    assert r["scales"][2]["ratio"] == 0.0
    assert [int(x["views"].max()) for x in r["refined"]] == [2, 3, 2, 3, 4]


def test_hook_ids_only_and_refined_only(gpu_ctx):
    _hook(gpu_ctx, _case("small"), 900, 300, want_refined=False)
    _hook(gpu_ctx, _case("small"), 900, 300, want_ids=False)


# ---- 2. the ORB stream -------------------------------------------------------------------------
def _filled(n_pairs, cap, device="cuda"):
    import torch
    from droplet_visual_odometry_amd.stream import Landmarks, RefinedLandmarks, TrackPoses, Tracks
    lm, tr, tp = Landmarks(n_pairs, cap, device), Tracks(n_pairs, cap, device), TrackPoses(n_pairs, device)
    rf = RefinedLandmarks(n_pairs, cap, device)
    for t in (lm.entries, lm.counts, tr.links, tr.scales, tp.poses, rf.refined, rf.ids):
        t.view(torch.uint8).fill_(FILL)
    return lm, tr, tp, rf


def _bind(fs, lm, tr, tp, rf, poses=True, **params):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    if poses:
        fs.bind_track_poses(tp)
    fs.bind_refine(rf, **params)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _stream_check(fs, lm, tr, tp, rf, recs, n_pairs, poses=True, **params):
    """The restatement fed with the stream's own landmarks (a Landmarks that holds every one),
    matches, records, scales and poses; returns the refined lists."""
    lms, xy1, xy2, matches = [], [], [], []
    none = np.zeros(0, np.int32)
    for i in range(n_pairs):
        assert lm.count(i) <= lm.cap
        e = lm.numpy(i)
        lms.append((e["match"], np.stack([e["X"], e["Y"], e["Z"]], 1) if len(e) else np.zeros((0, 3))))
        xy1.append(np.stack([e["x1"], e["y1"]], 1) if len(e) else np.zeros((0, 2), np.float32))
        xy2.append(np.stack([e["x2"], e["y2"]], 1) if len(e) else np.zeros((0, 2), np.float32))
        m = fs.matches(i) if len(e) else None
        matches.append((m["queryIdx"], m["trainIdx"]) if len(e) else (none, none))
    links, scales, want_poses, _ = pc.reference(lms, xy2, matches, recs, fs.K)
    _same_scales(tr.scales_numpy(), scales)
    if poses:
        _same_poses(tp.numpy(), want_poses)
    refined, info = rc.refine_reference(lms, xy1, xy2, matches, links, recs, scales, fs.K,
                                        poses=want_poses if poses else None, **params)
    ids = rc.ids_reference(links)
    for p in range(n_pairs):
        np.testing.assert_array_equal(tr.numpy(p, lm.count(p)), links[p], err_msg=str(p))
        assert rf.ids_numpy(p, lm.count(p)).tobytes() == ids[p].tobytes(), p
        _same_refined(rf.numpy(p, lm.count(p)), refined[p], p)
        # a linked landmark's first pixel is its predecessor's second: the same keypoint
        on = np.flatnonzero(links[p] >= 0)
        assert (xy1[p][on] == xy2[p - 1][links[p][on]]).all()
    return refined, ids, info


_ORB = {}


def _orb(gpu_ctx, size):
    if size not in _ORB:
        import torch
        from droplet_visual_odometry_amd.stream import FrameStream
        W, H, NF = size
        frames, K = synth_frames(W, H, range(FRAMES))
        cap = NF + 37
        fs = FrameStream(W, H, K, nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
        bufs = _filled(FRAMES - 1, cap)
        _bind(fs, *bufs)
        rec = fs.process(torch.from_numpy(frames).cuda())
        fs.sync()
        recs = FrameStream.records_numpy(rec, FRAMES - 1)
        _ORB[size] = dict(frames=frames, K=K, cap=cap, recs=recs, bufs=bufs, fs=fs,
                          want=_stream_check(fs, *bufs, recs, FRAMES - 1))
    return _ORB[size]


@pytest.mark.parametrize("size", ORB_SIZES)
def test_orb_stream_process(gpu_ctx, size):
    r = _orb(gpu_ctx, size)
    refined, ids, info = r["want"]
    print(size, "views", list(info["views"]), "max age", max(int(i["age"].max()) for i in ids if len(i)),
          "huber", info["quad"], info["lin"])
    assert info["views"][3:7].all() and max(int(i["age"].max()) for i in ids if len(i)) >= 4
    assert sum(int((x["status"] == rc.OK).sum()) for x in refined) >= 30  # enough fits for the comparison to mean something


def test_orb_blank_frame(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    frames = r["frames"].copy()
    frames[BLANK] = 90
    fs = r["fs"]
    bufs = _filled(FRAMES - 1, r["cap"])
    _bind(fs, *bufs, views=8, iters=3)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, FRAMES - 1)
    refined, ids, info = _stream_check(fs, *bufs, recs, FRAMES - 1, views=8, iters=3)
    assert recs[BLANK]["status"] != 0 and len(refined[BLANK]) == 0
    assert (refined[BLANK + 1]["status"] == rc.NONE).all() and refined[BLANK + 2]["views"].max() == 3
    assert all((x["root_pair"] > BLANK).all() for x in ids[BLANK + 1:])


def test_orb_records_only_motions(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    fs = r["fs"]
    bufs = _filled(FRAMES - 1, r["cap"])
    _bind(fs, *bufs, poses=False)
    rec = fs.process(torch.from_numpy(r["frames"]).cuda())
    fs.sync()
    _stream_check(fs, *bufs, FrameStream.records_numpy(rec, FRAMES - 1), FRAMES - 1, poses=False)
    assert (bufs[2].poses.cpu().numpy() == FILL).all()
    assert _bytes(bufs[3].ids) == _bytes(r["bufs"][3].ids) and _bytes(bufs[3].refined) != _bytes(r["bufs"][3].refined)


def test_orb_submit_equals_process(gpu_ctx):
    """Three batches submitted back to back, refine on the first two, equal the same batches
    processed one at a time, byte for byte."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = SMALL
    sizes, cap = [5, 4, 5], NF + 37
    starts = np.concatenate([[0], np.cumsum(np.array(sizes) - 1)])[:-1]
    frames, K = synth_frames(W, H, range(int(starts[-1] + sizes[-1])))
    dev = torch.from_numpy(frames).cuda()
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    want = []
    for k, (s0, m) in enumerate(zip(starts, sizes)):
        bufs = _filled(m - 1, cap)
        if k < 2:
            _bind(a, *bufs)
        else:
            _bind(a, *bufs[:3], None)
        rec = a.process(dev[s0:s0 + m])
        a.sync()
        recs = FrameStream.records_numpy(rec, m - 1)
        if k < 2:  # and the process side is right to begin with
            _stream_check(a, *bufs, recs, m - 1)
        want.append((recs, bufs))
    got = [(_filled(m - 1, cap), b.new_records(m - 1)) for m in sizes]
    torch.cuda.synchronize()
    for k, (s0, m, (bufs, rec)) in enumerate(zip(starts, sizes, got)):
        if k < 2:
            _bind(b, *bufs)
        else:
            _bind(b, *bufs[:3], None)
        b.submit(dev[s0:s0 + m], rec, wait_torch=False)
    b.drain()
    b.sync()
    for k, m in enumerate(sizes):
        (lm, tr, tp, rf), rec = got[k]
        wl, wt, wp, wr = want[k][1]
        assert FrameStream.records_numpy(rec, m - 1).tobytes() == want[k][0].tobytes(), k
        for x, y in ((lm.entries, wl.entries), (lm.counts, wl.counts), (tr.links, wt.links), (tr.scales, wt.scales),
                     (tp.poses, wp.poses), (rf.refined, wr.refined), (rf.ids, wr.ids)):
            assert _bytes(x) == _bytes(y), k
    assert (got[2][0][3].refined.cpu().numpy() == FILL).all() and (got[2][0][3].ids.cpu().numpy() == FILL).all()
    a.close()
    b.close()


def test_orb_one_shot_and_unbound_bytes(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, SMALL)
    W, H, NF = SMALL
    dev = torch.from_numpy(r["frames"]).cuda()
    fs, cap, n = r["fs"], r["cap"], FRAMES - 1
    lib = fs.ctx.lib

    def untouched(rf):
        return (rf.refined.cpu().numpy() == FILL).all() and (rf.ids.cpu().numpy() == FILL).all()

    # a stream that never binds refine, and one that binds nothing at all
    plain = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
    lm0, tr0, tp0, _ = _filled(n, cap)
    plain.bind_landmarks(lm0)
    plain.bind_tracks(tr0)
    plain.bind_track_poses(tp0)
    rec0 = plain.process(dev)
    plain.sync()
    bare = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=FRAMES, ctx=gpu_ctx)
    rec1 = bare.process(dev)
    bare.sync()
    lm, tr, tp, rf = r["bufs"]
    for x, y in ((lm.entries, lm0.entries), (lm.counts, lm0.counts), (tr.links, tr0.links), (tr.scales, tr0.scales),
                 (tp.poses, tp0.poses)):
        assert _bytes(x) == _bytes(y)
    assert r["recs"].tobytes() == FrameStream.records_numpy(rec0, n).tobytes()
    assert r["recs"].tobytes() == FrameStream.records_numpy(rec1, n).tobytes()
    # one-shot: a second bound batch writes the same, the batch after it leaves a refilled buffer alone
    bufs = _filled(n, cap)
    _bind(fs, *bufs)
    fs.process(dev)
    fs.sync()
    assert _bytes(bufs[3].refined) == _bytes(rf.refined) and _bytes(bufs[3].ids) == _bytes(rf.ids)
    bufs = _filled(n, cap)
    _bind(fs, *bufs[:3], None)
    fs.process(dev)
    fs.sync()
    assert untouched(bufs[3]) and _bytes(bufs[2].poses) == _bytes(tp0.poses)
    # cleared by None, by a later bind_track_poses or bind_tracks, and with the landmark binding
    for clear in ("none", "poses", "tracks", "landmarks"):
        bufs = _filled(n, cap)
        _bind(fs, *bufs)
        if clear == "none":
            fs.bind_refine(None)
        elif clear == "poses":
            fs.bind_track_poses(bufs[2])
        elif clear == "tracks":
            fs.bind_tracks(bufs[1])
        else:
            fs.bind_landmarks(None)
        assert fs._rf_next is None
        fs.process(dev)
        fs.sync()
        assert untouched(bufs[3]), clear
        assert (_bytes(bufs[1].scales) == _bytes(tr0.scales)) == (clear != "landmarks")
    # refine goes with a pending Tracks that has both buffers
    lm, tr, tp, rf = _filled(n, cap)
    args = (rf.refined.data_ptr(), rf.ids.data_ptr(), 0, 0, 0.0, 0.0)
    with pytest.raises(ValueError):
        fs.bind_refine(rf)
    fs.bind_landmarks(lm)
    with pytest.raises(ValueError):
        fs.bind_refine(rf)
    assert lib.dvo_stream_set_track_refine(fs.h, *args) == DVO_EINVAL
    assert lib.dvo_stream_set_tracks(fs.h, tr.links.data_ptr(), None) == 0
    assert lib.dvo_stream_set_track_refine(fs.h, *args) == DVO_EINVAL
    assert lib.dvo_stream_set_tracks(fs.h, None, tr.scales.data_ptr()) == 0
    assert lib.dvo_stream_set_track_refine(fs.h, *args) == DVO_EINVAL
    fs.bind_tracks(tr)
    for bad in (dict(views=9), dict(views=2), dict(iters=17), dict(inlier_px=float("nan"))):
        with pytest.raises(DVOError):
            fs.bind_refine(rf, **bad)
    # ids only, refined only, and other parameters reach the kernel
    fs.bind_refine(rf, ids=False, views=4, iters=2, huber_px=2.0, inlier_px=1.0)
    rec = fs.process(dev)
    fs.sync()
    assert (rf.ids.cpu().numpy() == FILL).all()
    lm2, tr2, tp2, rf2 = _filled(n, cap)
    _bind(fs, lm2, tr2, tp2, rf2, poses=False, refined=False)
    fs.process(dev)
    fs.sync()
    assert (rf2.refined.cpu().numpy() == FILL).all()
    rf.ids.copy_(rf2.ids)
    refined, _, _ = _stream_check(fs, lm, tr, tp, rf, FrameStream.records_numpy(rec, n), n, poses=False, views=4, iters=2,
                                  huber_px=2.0, inlier_px=1.0)
    assert max(int(x["views"].max()) for x in refined if len(x)) == 4
    # pairs that share no frame: refused, every binding consumed
    bufs = _filled(n, cap)
    _bind(fs, *bufs)
    with pytest.raises(ValueError):
        fs.process_pairs(dev)
    rec = fs.new_records(4)
    torch.cuda.synchronize()
    assert lib.dvo_stream_process_pairs(fs.h, dev.data_ptr(), 4, dev.stride(0), dev.stride(1), rec.data_ptr()) == DVO_EINVAL
    fs._lm_next = fs._tr_next = fs._tp_next = fs._rf_next = None  # what the wrapper holds for the call it did not make
    fs.process(dev)
    fs.sync()
    assert untouched(bufs[3]) and (bufs[1].scales.cpu().numpy() == FILL).all()
    plain.close()
    bare.close()


# ---- 3. the k-NN stream ------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_knn_stream(gpu_ctx, detector):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    W, H, n, cap = 640, 480, 5, 4096
    frames, K = synth_frames(W, H, range(n))
    dev = torch.from_numpy(frames).cuda()
    st = KnnFrameStream(W, H, K, n, detector=detector, feat_cap=4096, ctx=gpu_ctx)
    bufs = _filled(n - 1, cap)
    _bind(st, *bufs)
    rec = st.process(dev)
    st.sync()
    recs = st.records_numpy(rec, n - 1)
    assert (recs["status"] == 0).all()
    refined, ids, info = _stream_check(st, *bufs, recs, n - 1)
    print(detector, "views", list(info["views"]), "huber", info["quad"], info["lin"])
    assert info["views"][3] and info["views"][4] and max(int(i["age"].max()) for i in ids) >= 2
    # the two-phase call: detect() leaves the bindings for finish()
    bufs2 = _filled(n - 1, cap)
    _bind(st, *bufs2)
    st.detect(dev)
    st.finish()
    st.sync()
    for x, y in zip(bufs2[1:], bufs[1:]):
        for f in ("links", "scales", "poses", "refined", "ids"):
            if hasattr(x, f):
                assert _bytes(getattr(x, f)) == _bytes(getattr(y, f)), f
    # one-shot here too, and refine goes with a pending Tracks
    for t in (bufs2[3].refined, bufs2[3].ids):
        t.fill_(FILL)
    st.process(dev)
    st.sync()
    assert (bufs2[3].refined.cpu().numpy() == FILL).all() and (bufs2[3].ids.cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        st.bind_refine(bufs2[3])
    assert st.ctx.lib.dvo_knn_stream_set_track_refine(st.h, bufs2[3].refined.data_ptr(), None, 0, 0, 0.0, 0.0) == DVO_EINVAL
    st.close()
