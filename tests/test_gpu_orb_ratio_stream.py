"""FrameStream(ratio=): the ORB stream matching with knnMatch(k = 2) and the ratio test
(dvo_stream_set_ratio_test) instead of the cross check.  The expected record of a pair is chained
by hand: the oracle's ORB, the numpy Hamming 2-NN and ratio test of hamming_knn_cases (kept matches
in ascending queryIdx), the oracle's findEssentialMat on the kept points in that order, its
recoverPose.  Whatever the schedule (process, submit / drain, the fused pair call) the records are
the same, and a stream with the test off is the stream it always was."""
import numpy as np
import pytest

import hamming_knn_cases as hk
from conftest import synth_frames

pytestmark = pytest.mark.gpu

RATIO = 0.75
BLANK = 3


def _frames(W, H, n=6, blank=(BLANK,)):
    frames, K = synth_frames(W, H, range(n))
    frames = frames.copy()
    for b in blank:
        frames[b] = 90
    return frames, K


_EXPECT = {}


def _expected(oracle_mod, W, H, NF):
    """Per pair: None where the reference raises (an empty frame, fewer than 2 trains), else the
    oracle chain's values; computed once per size."""
    if (W, H, NF) in _EXPECT:
        return _EXPECT[(W, H, NF)]
    frames, K = _frames(W, H)
    feats = [oracle_mod.detect_and_compute(f, NF) for f in frames]
    out = []
    for i in range(len(frames) - 1):
        (k1, d1), (k2, d2) = feats[i], feats[i + 1]
        e = dict(nq=len(k1), nt=len(k2), ok=len(k1) > 0 and len(k2) >= 2)
        if e["ok"]:
            m = hk.ratio_matches(d1, d2, RATIO)
            # the condition of the case: the ratio test keeps enough to estimate from, and drops
            assert len(m) >= 8 and len(k1) - len(m) >= 1, (i, len(m), len(k1))
            q = np.array([a for a, _, _ in m])
            t = np.array([b for _, b, _ in m])
            p1 = oracle_mod.keypoints_to_points(k1[q]).astype(np.float64)
            p2 = oracle_mod.keypoints_to_points(k2[t]).astype(np.float64)
            E, mask, iters = oracle_mod.find_essential(p1, p2, K)
            assert E is not None and E.shape[0] == 3, i
            good, R, tv, _ = oracle_mod.recover_pose(E, p1, p2, K)
            e.update(m=m, E=E, iters=iters, good=good, R=R, t=tv.ravel(), inliers=int(mask.sum()))
        out.append(e)
    assert [e["ok"] for e in out] == [i not in (BLANK - 1, BLANK) for i in range(len(out))]
    _EXPECT[(W, H, NF)] = (frames, K, out)
    return _EXPECT[(W, H, NF)]


def _same(got, want, skip=()):
    bad = [k for k in got.dtype.names if k not in skip and not np.array_equal(got[k], want[k])]
    assert bad == [], (bad, got["status"], want["status"], got["n_matches"], want["n_matches"])


@pytest.mark.parametrize("W,H,NF", [(320, 240, 300), (640, 480, 500)])
def test_stream_equals_the_oracle_chain(gpu_ctx, oracle_mod, W, H, NF):
    import torch
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT
    from droplet_visual_odometry_amd.stream import FrameStream
    frames, K, want = _expected(oracle_mod, W, H, NF)
    fs = FrameStream(W, H, K, nfeatures=NF, max_frames=len(frames), ctx=gpu_ctx, ratio=RATIO)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    recs = FrameStream.records_numpy(rec, len(frames) - 1)
    for i, e in enumerate(want):
        r = recs[i]
        assert (r["n_kp_prev"], r["n_kp_cur"]) == (e["nq"], e["nt"]), i
        mg = fs.matches(i)
        if not e["ok"]:
            assert r["status"] == DVO_ENOFEAT, i
            assert r["n_matches"] == 0 and len(mg) == 0 and r["n_good"] == 0 and r["n_inliers"] == 0, i
            assert not np.any(r["R"]) and not np.any(r["t"]) and not np.any(r["E"]), i
            continue
        assert r["status"] == 0, i
        assert [(int(g["queryIdx"]), int(g["trainIdx"]), float(g["distance"])) for g in mg] == e["m"], i
        assert r["n_matches"] == len(e["m"]), i
        assert r["ransac_iters"] == e["iters"], i
        assert r["n_inliers"] == e["inliers"], i
        np.testing.assert_array_equal(r["E"].reshape(3, 3), e["E"])
        np.testing.assert_array_equal(r["R"].reshape(3, 3), e["R"])
        np.testing.assert_array_equal(r["t"], e["t"])
        assert r["n_good"] == e["good"], i
    # the pair whose train frame is empty: the counts, zeros elsewhere
    r = recs[BLANK - 1]
    for name in ("n_matches", "n_inliers", "n_good", "ransac_iters", "n_models", "n_hypotheses"):
        assert r[name] == 0, name
    fs.close()


def test_submit_equals_process(gpu_ctx):
    """Four pipelined batches with the ratio test equal the same batches processed one at a time,
    byte for byte (a blank frame among them)."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF, sizes = 320, 240, 300, [4, 3, 4, 2]
    starts = np.concatenate([[0], np.cumsum(np.array(sizes) - 1)])[:-1]
    n = int(starts[-1] + sizes[-1])
    frames, K = _frames(W, H, n, blank=(5,))
    dev = torch.from_numpy(frames).cuda()
    a = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx, ratio=RATIO)
    b = FrameStream(W, H, K, nfeatures=NF, max_frames=max(sizes), ctx=gpu_ctx, ratio=RATIO)
    want = []
    for s0, m in zip(starts, sizes):
        r = a.process(dev[s0:s0 + m])
        a.sync()
        want.append(FrameStream.records_numpy(r, m - 1))
    recs = [b.new_records(m - 1) for m in sizes]
    torch.cuda.synchronize()
    for (s0, m), r in zip(zip(starts, sizes), recs):
        b.submit(dev[s0:s0 + m], r, wait_torch=False)
    b.drain()
    b.sync()
    for i, m in enumerate(sizes):
        assert FrameStream.records_numpy(recs[i], m - 1).tobytes() == want[i].tobytes(), i
    allrec = np.concatenate(want)
    assert np.any(allrec["status"] != 0) and np.sum(allrec["status"] == 0) >= 6
    a.close()
    b.close()


def test_pair_equals_stream(gpu_ctx):
    """The fused pair call follows the setting: its records equal the stream's, n_hypotheses aside
    (the per-call RANSAC schedule solves every hypothesis in one round)."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = 320, 240, 300
    frames, K = _frames(W, H)
    fs = FrameStream(W, H, K, nfeatures=NF, max_frames=len(frames), ctx=gpu_ctx, ratio=RATIO)
    rec = fs.process(torch.from_numpy(frames).cuda())
    fs.sync()
    want = FrameStream.records_numpy(rec, len(frames) - 1)
    ps = ops.PairStream(W, H, K, nfeatures=NF, ctx=gpu_ctx, ratio=RATIO)
    got = [ps.pair(frames[0], frames[1])]
    got += [ps.pair(None, frames[i + 1], reuse_prev=True) for i in range(1, len(frames) - 1)]
    _same(np.array(got), want, skip=("n_hypotheses",))
    fresh = ops.PairStream(W, H, K, nfeatures=NF, ctx=gpu_ctx)
    fresh.set_ratio_test(RATIO)
    _same(np.array([fresh.pair(frames[4], frames[5])]), want[4:5], skip=("n_hypotheses",))
    for s in (fs, ps, fresh):
        s.close()


def test_ratio_off_is_the_cross_check_stream(gpu_ctx):
    """set_ratio_test(0) after ratio batches: records and matches byte-equal to a stream that never
    had the test set; and the ratio records do differ from them."""
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = 320, 240, 300
    frames, K = _frames(W, H)
    dev = torch.from_numpy(frames).cuda()
    plain = FrameStream(W, H, K, nfeatures=NF, max_frames=len(frames), ctx=gpu_ctx)
    r = plain.process(dev)
    plain.sync()
    want = FrameStream.records_numpy(r, len(frames) - 1)
    want_m = [plain.matches(p) for p in range(len(frames) - 1)]
    fs = FrameStream(W, H, K, nfeatures=NF, max_frames=len(frames), ctx=gpu_ctx, ratio=RATIO)
    r = fs.process(dev)
    fs.sync()
    with_ratio = FrameStream.records_numpy(r, len(frames) - 1)
    assert np.any(with_ratio["n_matches"] != want["n_matches"])
    fs.set_ratio_test(0)
    r = fs.process(dev)
    fs.sync()
    assert FrameStream.records_numpy(r, len(frames) - 1).tobytes() == want.tobytes()
    for p, m in enumerate(want_m):
        assert fs.matches(p).tobytes() == m.tobytes(), p
    fs.set_ratio_test(None)
    plain.close()
    fs.close()


def test_set_ratio_test_refuses(gpu_ctx):
    import torch
    from droplet_visual_odometry_amd._native import DVO_EINVAL
    from droplet_visual_odometry_amd.stream import FrameStream
    W, H, NF = 320, 240, 300
    frames, K = _frames(W, H)
    dev = torch.from_numpy(frames).cuda()
    fs = FrameStream(W, H, K, nfeatures=NF, max_frames=3, ctx=gpu_ctx)
    lib = fs.ctx.lib
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
        assert lib.dvo_stream_set_ratio_test(fs.h, bad) == DVO_EINVAL, bad
    assert lib.dvo_stream_set_ratio_test(fs.h, 0.75) == 0
    rec = fs.new_records(2)
    torch.cuda.synchronize()
    fs.submit(dev[0:3], rec, wait_torch=False)
    assert lib.dvo_stream_set_ratio_test(fs.h, 0.8) == DVO_EINVAL  # a batch is pending
    assert lib.dvo_stream_set_ratio_test(fs.h, 0.0) == DVO_EINVAL
    fs.drain()
    fs.sync()
    assert lib.dvo_stream_set_ratio_test(fs.h, 0.8) == 0
    fs.close()
