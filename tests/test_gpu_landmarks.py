"""Landmarks on the device (dvo_stream_set_landmarks, stream.Landmarks): per pair the matches that
findEssentialMat's mask and recoverPose's mask both keep, with their triangulated positions.
Counts, match indices and pixel coordinates must be equal and X, Y, Z bit-identical to the CPU
oracle's (landmark_cases.expected), and every byte outside the written slots must keep the 0xA5
the buffers were filled with."""
import numpy as np
import pytest

import landmark_cases as lc
from conftest import synth_frames

pytestmark = pytest.mark.gpu

FILL = 0xA5
STRIDE = 550
ORB_SIZES = [(320, 240, 300), (640, 480, 500)]
SMALL = ORB_SIZES[0]
BLANK = 3


def _filled(n_pairs, cap, device="cuda"):
    import torch
    from droplet_visual_odometry_amd.stream import Landmarks
    lm = Landmarks(n_pairs, cap, device)
    lm.entries.fill_(FILL)
    lm.counts.view(torch.uint8).fill_(FILL)
    return lm


def _raw(lm):
    return lm.entries.cpu().numpy(), lm.counts.cpu().numpy()


# ---- 1. the kernels at sizes around their tiles of 256 matches ---------------------------------
_SYN = {}


def _synthetic(oracle_mod):
    if not _SYN:
        pts = np.zeros((len(lc.SIZES), STRIDE, 4), np.float32)
        want, pp = [], []
        for p, m in enumerate(lc.SIZES):
            p1, p2, K = lc.case(m)
            pts[p, :m, :2], pts[p, :m, 2:] = p1, p2
            pp.append((p1, p2))
            want.append(lc.expected(oracle_mod, p1.astype(np.float64), p2.astype(np.float64), K))
        _SYN.update(pts=pts, K=K, want=want, pp=pp)
    return _SYN


@pytest.mark.parametrize("cap", (STRIDE, 64))
def test_synthetic_sizes(gpu_ctx, oracle_mod, cap):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import LANDMARK_DTYPE
    s = _synthetic(oracle_mod)
    want = s["want"]
    # the conditions the sizes were chosen for, on the oracle's output
    assert want[0]["count"] == 0 and all(w["count"] > 0 for w in want[1:])
    assert sum(w["only_pose"] for w in want) > 0 and sum(w["only_inlier"] for w in want) > 0
    assert max(w["count"] for w in want) > 64 and want[1]["count"] < 64  # cap 64 overflows some pairs only
    P = len(lc.SIZES)
    out = np.full(P * cap * LANDMARK_DTYPE.itemsize, FILL, np.uint8).view(LANDMARK_DTYPE).reshape(P, cap)
    out, count, rec = ops.test_landmarks(s["pts"], lc.SIZES, s["K"], cap, out=out, ctx=gpu_ctx)
    print("cap", cap, "m", lc.SIZES, "landmarks", list(count), "oracle", [w["count"] for w in want], "models", list(rec["n_models"]))
    assert rec[0]["status"] == 0 and rec[0]["n_models"] > 1  # five matches: several E, the reference stops
    for p, m in enumerate(lc.SIZES):
        p1, p2 = s["pp"][p]
        w = lc.expected(oracle_mod, p1.astype(np.float64), p2.astype(np.float64), s["K"], rec=rec[p])
        assert w["count"] == want[p]["count"] and rec[p]["n_matches"] == m
        lc.check_pair(out[p, :min(count[p], cap)], int(count[p]), cap, want[p], p1, p2)
    lc.untouched(out.view(np.uint8).reshape(P, cap, -1), count, cap, FILL)


# ---- 2.-6. the ORB stream ----------------------------------------------------------------------
_ORB = {}


def _pair_points(fs, i):
    """(p1, p2) float32 [m, 2] of pair i in match order, from the stream's own features and matches."""
    m = fs.matches(i)
    (k1, _), (k2, _) = fs.features(i), fs.features(i + 1)
    return (np.stack([k1["x"][m["queryIdx"]], k1["y"][m["queryIdx"]]], 1),
            np.stack([k2["x"][m["trainIdx"]], k2["y"][m["trainIdx"]]], 1))


def _orb(gpu_ctx, oracle_mod, size):
    """Once per size: frames 0-5 through process() with a binding that holds every landmark; the
    records, raw buffers, the pairs' points and the oracle's expectation."""
    if size not in _ORB:
        import torch
        from droplet_visual_odometry_amd.stream import FrameStream
        W, H, NF = size
        frames, K = synth_frames(W, H, range(6))
        cap = NF + 37
        fs = FrameStream(W, H, K, nfeatures=NF, max_frames=6, ctx=gpu_ctx)
        lm = _filled(5, cap)
        fs.bind_landmarks(lm)
        rec = fs.process(torch.from_numpy(frames).cuda())
        fs.sync()
        recs = FrameStream.records_numpy(rec, 5)
        pts = [_pair_points(fs, i) for i in range(5)]
        want = [lc.expected(oracle_mod, p1.astype(np.float64), p2.astype(np.float64), K, rec=recs[i])
                for i, (p1, p2) in enumerate(pts)]
        _ORB[size] = dict(frames=frames, K=K, cap=cap, recs=recs, pts=pts, want=want, lm=lm, fs=fs)
    return _ORB[size]


@pytest.mark.parametrize("size", ORB_SIZES)
def test_orb_stream_process(gpu_ctx, oracle_mod, size):
    r = _orb(gpu_ctx, oracle_mod, size)
    raw, counts = _raw(r["lm"])
    print(size, "m", [len(p1) for p1, _ in r["pts"]], "landmarks", list(counts), "oracle", [w["count"] for w in r["want"]],
          "only pose", [w["only_pose"] for w in r["want"]], "only inlier", [w["only_inlier"] for w in r["want"]])
    assert all(w["count"] > 0 for w in r["want"])
    assert sum(w["only_pose"] for w in r["want"]) > 0 and sum(w["only_inlier"] for w in r["want"]) > 0
    if size != SMALL:
        assert max(len(p1) for p1, _ in r["pts"]) > 256  # more than one tile
    for i, w in enumerate(r["want"]):
        assert r["lm"].count(i) == counts[i]
        lc.check_pair(r["lm"].numpy(i), int(counts[i]), r["cap"], w, *r["pts"][i])
    lc.untouched(raw, counts, r["cap"], FILL)


def test_orb_overflow(gpu_ctx, oracle_mod):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, oracle_mod, SMALL)
    cap = 48
    full = [w["count"] for w in r["want"]]
    assert min(full) <= cap < max(full)  # some pairs fit whole, some overflow
    fs = r["fs"]
    lm = _filled(5, cap)
    fs.bind_landmarks(lm)
    fs.process(torch.from_numpy(r["frames"]).cuda())
    fs.sync()
    raw, counts = _raw(lm)
    assert list(counts) == full
    for i, w in enumerate(r["want"]):
        lc.check_pair(lm.numpy(i), int(counts[i]), cap, w, *r["pts"][i])
    lc.untouched(raw, counts, cap, FILL)


def test_orb_failed_pairs(gpu_ctx, oracle_mod):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, oracle_mod, SMALL)
    frames = r["frames"].copy()
    frames[BLANK] = 90
    fs = r["fs"]
    lm = _filled(5, r["cap"])
    fs.bind_landmarks(lm)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, 5)
    raw, counts = _raw(lm)
    for i, w in enumerate(r["want"]):
        if i in (BLANK - 1, BLANK):
            assert recs[i]["status"] != 0 and counts[i] == 0 and len(lm.numpy(i)) == 0, i
        else:
            lc.check_pair(lm.numpy(i), int(counts[i]), r["cap"], w, *r["pts"][i])
    lc.untouched(raw, counts, r["cap"], FILL)


def test_orb_submit_equals_process(gpu_ctx):
    """Four pipelined batches, each with its own Landmarks, equal the same batches processed one at
    a time: entries, counts and records byte for byte."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = SMALL
    sizes, cap = [4, 3, 4, 2], NF + 37
    starts = np.concatenate([[0], np.cumsum(np.array(sizes) - 1)])[:-1]
    frames, K = synth_frames(W, H, range(int(starts[-1] + sizes[-1])))
    dev = torch.from_numpy(frames).cuda()
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx)
    want = []
    for s0, m in zip(starts, sizes):
        lm = _filled(m - 1, cap)
        a.bind_landmarks(lm)
        rec = a.process(dev[s0:s0 + m])
        a.sync()
        want.append((FrameStream.records_numpy(rec, m - 1), *_raw(lm)))
    lms = [_filled(m - 1, cap) for m in sizes]
    recs = [b.new_records(m - 1) for m in sizes]
    torch.cuda.synchronize()
    for s0, m, lm, rec in zip(starts, sizes, lms, recs):
        b.bind_landmarks(lm)
        b.submit(dev[s0:s0 + m], rec, wait_torch=False)
    b.drain()
    b.sync()
    total = 0
    for i, m in enumerate(sizes):
        raw, counts = _raw(lms[i])
        assert FrameStream.records_numpy(recs[i], m - 1).tobytes() == want[i][0].tobytes(), i
        assert counts.tobytes() == want[i][2].tobytes(), i
        assert raw.tobytes() == want[i][1].tobytes(), i
        lc.untouched(raw, counts, cap, FILL)
        total += int(counts.sum())
    assert total > 0
    a.close()
    b.close()


def test_orb_one_shot_and_default(gpu_ctx, oracle_mod):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import FrameStream
    r = _orb(gpu_ctx, oracle_mod, SMALL)
    W, H, NF = SMALL
    dev = torch.from_numpy(r["frames"]).cuda()
    # a stream that never binds: the bound stream's records are its bytes
    plain = FrameStream(W, H, r["K"], nfeatures=NF, max_frames=6, ctx=gpu_ctx)
    rec = plain.process(dev)
    plain.sync()
    assert FrameStream.records_numpy(rec, 5).tobytes() == r["recs"].tobytes()
    # one-shot: the call after a bound one writes nothing, and its records are the same again
    fs = r["fs"]
    lm = _filled(5, r["cap"])
    fs.bind_landmarks(lm)
    fs.process(dev)
    fs.sync()
    assert lm.count(0) == r["want"][0]["count"]
    lm.entries.fill_(FILL)
    lm.counts.view(torch.uint8).fill_(FILL)
    rec = fs.process(dev)
    fs.sync()
    raw, counts = _raw(lm)
    assert (raw == FILL).all() and (counts.view(np.uint8) == FILL).all()
    assert FrameStream.records_numpy(rec, 5).tobytes() == r["recs"].tobytes()
    # a cleared binding writes nothing either
    fs.bind_landmarks(lm)
    fs.bind_landmarks(None)
    fs.process(dev)
    fs.sync()
    raw, counts = _raw(lm)
    assert (raw == FILL).all() and (counts.view(np.uint8) == FILL).all()
    lib = fs.ctx.lib
    assert lib.dvo_stream_set_landmarks(fs.h, lm.entries.data_ptr(), lm.counts.data_ptr(), 0) == DVO_EINVAL
    assert lib.dvo_stream_set_landmarks(fs.h, lm.entries.data_ptr(), None, 8) == DVO_EINVAL
    with pytest.raises(ValueError):  # a Landmarks with fewer rows than the batch has pairs
        fs.bind_landmarks(_filled(2, 8))
        fs.process(dev)
    fs.bind_landmarks(None)
    plain.close()


# ---- 7. the k-NN stream ------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_knn_stream(gpu_ctx, oracle_mod, detector):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    W, H, n, cap = 640, 480, 4, 1200
    frames, K = synth_frames(W, H, range(n))
    dev = torch.from_numpy(frames).cuda()
    st = KnnFrameStream(W, H, K, n, detector=detector, feat_cap=4096, ctx=gpu_ctx)
    a = _filled(n - 1, cap)
    st.bind_landmarks(a)
    rec = st.process(dev)
    st.sync()
    recs = st.records_numpy(rec, n - 1)
    assert (recs["status"] == 0).all() and (recs["n_matches"] > 256).all()  # several tiles per pair
    raw_a, counts_a = _raw(a)
    print(detector, "m", list(recs["n_matches"]), "landmarks", list(counts_a))
    for i in range(n - 1):
        m = st.matches(i)
        (k1, _), (k2, _) = st.features(i), st.features(i + 1)
        p1 = np.stack([k1["x"][m["queryIdx"]], k1["y"][m["queryIdx"]]], 1)
        p2 = np.stack([k2["x"][m["trainIdx"]], k2["y"][m["trainIdx"]]], 1)
        w = lc.expected(oracle_mod, p1.astype(np.float64), p2.astype(np.float64), K, rec=recs[i])
        assert 0 < w["count"] < len(m), i
        lc.check_pair(a.numpy(i), int(counts_a[i]), cap, w, p1, p2)
    lc.untouched(raw_a, counts_a, cap, FILL)
    # the two-phase call: detect() leaves the binding for finish()
    b = _filled(n - 1, cap)
    st.bind_landmarks(b)
    st.detect(dev)
    rec2 = st.finish()
    st.sync()
    raw_b, counts_b = _raw(b)
    assert st.records_numpy(rec2, n - 1).tobytes() == recs.tobytes()
    assert raw_b.tobytes() == raw_a.tobytes() and counts_b.tobytes() == counts_a.tobytes()
    # one-shot here too
    b.entries.fill_(FILL)
    st.process(dev)
    st.sync()
    assert (b.entries.cpu().numpy() == FILL).all()
    assert st.ctx.lib.dvo_knn_stream_set_landmarks(st.h, b.entries.data_ptr(), b.counts.data_ptr(), 0) == DVO_EINVAL
    st.close()
