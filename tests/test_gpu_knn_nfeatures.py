"""SIFT_create(nfeatures = 300) in the k-NN paths: stream.KnnFrameStream (frame by frame, with a
detect group, BFMatcher and FLANN, in one call and in two phases), ops.KnnPairStream, the drop-in's
fused pair path and dist.ShardedKnnRunner, on the 320 x 240 synthetic frames.  Their full counts
(750 / 783 / 945 / 1131) are all above the streams' feat_cap of 304; retain keeps 300 / 300 / 302 /
300.  Every frame's features must be the oracle's default detection permuted by oracle.retain_best
(sift_nfeatures_cases.expected), and the records those of the paths that already agree with each
other at nfeatures = 0: the oracle chain, the chained pair path, one stream."""
import os
import socket
import sys
import time

import numpy as np
import pytest

import sift_nfeatures_cases as sc

pytestmark = pytest.mark.gpu

W, H = sc.SYNTH_WH
N, CAP = 300, 304
SEED = 0xFFFFFFFF
DEADLINE_S = 240.0  # sharded workers are joined against it; never waited for unless one hangs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PAIRS = {}


def _stream(K, ctx, max_frames=4, **kw):
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    kw.setdefault("feat_cap", CAP)
    kw.setdefault("nfeatures", N)
    return KnnFrameStream(W, H, K, max_frames, detector="sift", ctx=ctx, **kw)


def _run(st, frames):
    import torch
    rec = st.process(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    st.sync()
    return st.records_numpy(rec, len(frames) - 1)


def _same(a, b, skip=()):
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    assert len(a) == len(b)
    for name in PAIR_RECORD_DTYPE.names:
        if name not in skip:
            np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def _pair_chain(ctx, matcher):
    """Once per matcher: (records, match lists, final theRNG state) of ops.KnnPairStream(nfeatures =
    300) over the 3 consecutive pairs, each from both frames, the state chained."""
    if matcher not in _PAIRS:
        from droplet_visual_odometry_amd import ops
        from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
        frames, K = sc.synth()
        ks = ops.KnnPairStream(W, H, K, detector="sift", matcher=matcher, ctx=ctx, nfeatures=N)
        recs, matches, state = np.zeros(3, PAIR_RECORD_DTYPE), [], SEED
        for p in range(3):
            recs[p], state = ks.pair(frames[p], frames[p + 1], rng_state=state)
            matches.append(ks.matches())
        ks.close()
        _PAIRS[matcher] = (recs, matches, state)
    return _PAIRS[matcher]


def _check_stream(st, rec, oracle_mod, ctx, matcher):
    """The slots hold the retained features; records and match lists are the chained pair path's."""
    from droplet_visual_odometry_amd import ops
    frames, _ = sc.synth()
    for f in range(4):
        got = st.features(f)
        sc.same_features(got, sc.expected(oracle_mod, ("synth", f), N))
        sc.same_features(got, ops.sift_detect_and_compute(frames[f], ctx=ctx, nfeatures=N))
    want, matches, state = _pair_chain(ctx, matcher)
    assert (want["status"] == 0).all()
    _same(rec, want, skip=("n_hypotheses",))
    kept = sc.SYNTH_KEPT[N]
    np.testing.assert_array_equal(rec["n_kp_prev"], kept[:3])
    np.testing.assert_array_equal(rec["n_kp_cur"], kept[1:])
    for p in range(3):
        np.testing.assert_array_equal(st.matches(p).view(np.uint8), matches[p].view(np.uint8))
    if matcher == "flann":
        assert st.rng_state == state != SEED


@pytest.mark.parametrize("kw", [dict(), dict(detect_group=2), dict(matcher="flann"), dict(matcher="flann", detect_group=2)],
                         ids=["bf", "bf-group2", "flann", "flann-group2"])
def test_stream_equals_single_frame_detector_and_pair_path(gpu_ctx, oracle_mod, kw):
    _, K = sc.synth()
    st = _stream(K, gpu_ctx, **kw)
    rec = _run(st, sc.synth()[0])
    _check_stream(st, rec, oracle_mod, gpu_ctx, kw.get("matcher", "bf"))
    if "matcher" not in kw:
        np.testing.assert_array_equal(rec["n_matches"], (78, 119, 99))  # the CPU oracle chain's counts
    st.close()


def test_first_record_equals_the_oracle_chain(gpu_ctx, oracle_mod):
    """test_gpu_knn_stream.py::test_record_equals_oracle_chain, built from the retained features."""
    _, K = sc.synth()
    st = _stream(K, gpu_ctx)
    rec = _run(st, sc.synth()[0])[0]
    m = st.matches(0)
    st.close()
    k1, d1 = sc.expected(oracle_mod, ("synth", 0), N)
    k2, d2 = sc.expected(oracle_mod, ("synth", 1), N)
    idx, dist = oracle_mod.bf_knn_float(d1, d2, 2, 0)
    keep = [q for q in range(len(d1)) if float(dist[q, 0]) < 0.75 * float(dist[q, 1])]
    p1 = np.stack([k1["x"][keep], k1["y"][keep]], 1).astype(np.float64)
    p2 = np.stack([k2["x"][idx[keep, 0]], k2["y"][idx[keep, 0]]], 1).astype(np.float64)
    E, _, _ = oracle_mod.find_essential(p1, p2, K)
    assert rec["status"] == 0 and rec["n_models"] == 1
    np.testing.assert_array_equal(rec["E"].reshape(3, 3), E)
    assert (rec["n_kp_prev"], rec["n_kp_cur"], rec["n_matches"]) == (len(k1), len(k2), len(keep)) == (300, 300, 78)
    np.testing.assert_array_equal(m["queryIdx"], keep)
    np.testing.assert_array_equal(m["trainIdx"], idx[keep, 0])
    np.testing.assert_array_equal(m["distance"].view(np.uint32), dist[keep, 0].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("matcher", ["bf", "flann"])
def test_detect_then_finish(gpu_ctx, oracle_mod, matcher):
    import torch
    frames, K = sc.synth()
    st = _stream(K, gpu_ctx, matcher=matcher, detect_group=2)
    st.detect(torch.from_numpy(frames).cuda())
    rec = st.finish()
    st.sync()
    _check_stream(st, st.records_numpy(rec, 3), oracle_mod, gpu_ctx, matcher)
    st.close()


def test_setter_between_calls_and_the_default(gpu_ctx, oracle_mod):
    """nfeatures 0 on a stream with room is today's result; the setter takes effect in both routes;
    a setter that changes the value drops a pending detection, one that does not keeps it."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVO_EINVAL, DVOError
    frames, K = sc.synth()
    d = torch.from_numpy(frames).cuda()
    st = _stream(K, gpu_ctx, feat_cap=max(sc.SYNTH_FULL) + 5, nfeatures=0)
    _run(st, frames)
    for f in range(4):
        sc.same_features(st.features(f), ops.sift_detect_and_compute(frames[f], ctx=gpu_ctx))
    for group in (0, 2):
        st.set_detect_group(group)
        for n in (64, N, 0):
            st.set_nfeatures(n)
            rec = _run(st, frames)
            want = sc.SYNTH_KEPT.get(n, sc.SYNTH_FULL)
            np.testing.assert_array_equal(rec["n_kp_cur"], want[1:])
            for f in (2, 3):
                sc.same_features(st.features(f), sc.expected(oracle_mod, ("synth", f), n))
    st.set_nfeatures(N)
    st.detect(d)
    st.set_nfeatures(N)  # no change: the detection stays pending
    st.finish()
    st.detect(d)
    st.set_nfeatures(64)  # a change: dropped
    with pytest.raises(DVOError) as e:
        st.finish()
    assert e.value.code == DVO_EINVAL
    with pytest.raises(DVOError) as e:
        st.set_nfeatures(-1)
    assert e.value.code == DVO_EINVAL
    st.close()


def test_kept_count_above_feat_cap(gpu_ctx, oracle_mod):
    """feat_cap 301: frame 2 keeps 302, so pairs 1 and 2 are DVO_ECAP; pair 0 is unchanged."""
    from droplet_visual_odometry_amd._native import DVO_ECAP
    frames, K = sc.synth()
    want, _, _ = _pair_chain(gpu_ctx, "bf")
    for group in (0, 2):
        st = _stream(K, gpu_ctx, feat_cap=301, detect_group=group)
        rec = _run(st, frames)
        st.close()
        assert tuple(rec["status"]) == (0, DVO_ECAP, DVO_ECAP)
        _same(rec[:1], want[:1], skip=("n_hypotheses",))
        np.testing.assert_array_equal(rec["n_kp_cur"], sc.SYNTH_KEPT[N][1:])  # the kept counts all the same
        assert not np.any(rec["n_matches"][1:])


def test_pair_handle_redetects_after_a_change(gpu_ctx, oracle_mod):
    from droplet_visual_odometry_amd import ops
    frames, K = sc.synth()
    ks = ops.KnnPairStream(W, H, K, detector="sift", ctx=gpu_ctx)
    r0, _ = ks.pair(frames[0], frames[1])
    assert (r0["n_kp_prev"], r0["n_kp_cur"]) == sc.SYNTH_FULL[:2]
    ks.set_nfeatures(N)
    r1, _ = ks.pair(frames[1], frames[2], reuse_prev=True)  # frame 1 is detected again, under nfeatures = 300
    sc.same_features(ks.features(0), sc.expected(oracle_mod, ("synth", 1), N))
    sc.same_features(ks.features(1), sc.expected(oracle_mod, ("synth", 2), N))
    want, _, _ = _pair_chain(gpu_ctx, "bf")
    _same(np.array([r1]), want[1:2])
    r2, _ = ks.pair(None, frames[3], reuse_prev=True)  # and from then on the cache serves again
    _same(np.array([r2]), want[2:3])
    ks.set_nfeatures(N)  # no change: the cache stays
    r2b, _ = ks.pair(None, frames[3], reuse_prev=True)
    assert (r2b["n_kp_prev"], r2b["n_kp_cur"]) == (300, 300)
    ks.close()


def _v3():
    sys.path.insert(0, os.path.join(ROOT, "droplet_visual_odometry_amd", "dropin"))
    try:
        import visual_odometry_v3 as v3
    finally:
        sys.path.pop(0)
    return v3


def test_dropin_fused_equals_operator_path(gpu_ctx, tmp_path):
    """feature_detector = SIFT_create(nfeatures = 300) in mode knn_sift: the pairs stay on the
    one-call path, and the 4 x 4s equal the operator-by-operator path's."""
    from test_gpu_knn_pair import _make
    from droplet_visual_odometry_amd import cv
    from droplet_visual_odometry_amd.synth import marker_corners
    v3 = _v3()
    frames, K = sc.synth()
    corners = [marker_corners(i, K) for i in range(4)]
    runs = {}
    for slow in (False, True):
        vo = _make(v3, K, tmp_path, "knn_sift", slow)
        vo.feature_detector = cv.SIFT_create(nfeatures=N)
        hits, inner = [], vo._fused_pair
        vo._fused_pair = lambda p, c: hits.append(inner(p, c)) or hits[-1]
        T, out = vo.robot_curr_position, []
        for a in range(3):
            T, rel = vo.visual_odometry_calculations(frames[a], frames[a + 1], T, corners[a], corners[a + 1])
            out.append((rel, T, np.array(vo.essential_matrix)))
        assert sum(h is not None for h in hits) == (0 if slow else 3)
        runs[slow] = (vo, out)
    (fused, of), (slow, os_) = runs[False], runs[True]
    assert fused._pair_engine is not None and fused._pair_engine[1].nfeatures == N and slow._pair_engine is None
    want, _, _ = _pair_chain(gpu_ctx, "bf")
    for p, ((rf, Tf, Ef), (rs, Ts, Es)) in enumerate(zip(of, os_)):
        np.testing.assert_array_equal(rf, rs)
        np.testing.assert_array_equal(Tf, Ts)
        np.testing.assert_array_equal(Ef, Es)
        np.testing.assert_array_equal(Ef, want["E"][p].reshape(3, 3))


# ---- sharded: two gloo ranks on the one GPU, and world 1 over RCCL, in the manner of
# test_gpu_knn_sharded.py.  A window has the same number of pairs on every step and every rank needs
# a pair of it, so two windows take 4 pairs: synthetic frames 0..4 (frame 4: 936 keypoints, 300 kept).
def _sharded_input():
    from conftest import synth_frames
    from droplet_visual_odometry_amd.synth import marker_corners
    frames, K = synth_frames(W, H, range(5))
    return frames, np.stack([marker_corners(i, K) for i in range(5)]), K


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, backend, out):
    import faulthandler
    import torch
    faulthandler.enable()
    torch.set_num_threads(2)
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import torch.distributed as dist
    from droplet_visual_odometry_amd import dist as ddist
    from droplet_visual_odometry_amd._native import Context
    from droplet_visual_odometry_amd.synth import MARKER_LEN
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ddist.init_process_group(backend, rank, world, device=dev, timeout_s=120.0)
    frames, corners, K = _sharded_input()
    d_frames, d_corners = torch.from_numpy(frames).to(dev), torch.from_numpy(corners).to(dev)
    run = ddist.ShardedKnnRunner(W, H, K, 2, world, rank, MARKER_LEN, detector="sift", matcher="flann", feat_cap=CAP,
                                 ctx=Context(0), host_gather=backend == "gloo", nfeatures=N)
    pending = []
    for w in range(2):
        p0, p1, f0, f1 = ddist.shard_window(2, world, rank, w * 2)
        for recs, T_rel, T_abs in run.step(d_frames[f0:f1], d_corners[f0:f1 - 1], d_corners[f0 + 1:f1]):
            pending.append((recs.clone(), T_rel.clone() if T_rel is not None else None, T_abs))
    assert run.drain() == []
    run.sync()
    rec = np.concatenate([r.cpu().numpy() for r, _, _ in pending]).tobytes()
    Trel = b"".join(T.cpu().numpy().tobytes() for _, T, _ in pending if T is not None)
    Tabs = b"".join(f.result().tobytes() for _, _, f in pending if f is not None)
    out[rank] = (rec, Trel, Tabs, run.rng_state)
    run.close()
    dist.destroy_process_group()


def _spawn(world, backend):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, out), nprocs=world, join=False)
    end = time.monotonic() + DEADLINE_S
    while not ctx.join(timeout=1.0):  # raises when a worker failed
        if time.monotonic() > end:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            pytest.fail(f"sharded workers still running after {DEADLINE_S:.0f} s")
    return dict(out)


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (1, "nccl")])
def test_sharded_equals_one_stream(gpu_ctx, world, backend):
    import torch
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    from droplet_visual_odometry_amd.stream import PoseTail
    from droplet_visual_odometry_amd.synth import MARKER_LEN
    frames, corners, K = _sharded_input()
    st = _stream(K, gpu_ctx, max_frames=5, matcher="flann")
    rec = st.process(torch.from_numpy(frames).cuda())
    st.sync()
    dc = torch.from_numpy(corners).cuda()
    T_rel, T_abs = PoseTail(K, MARKER_LEN, ctx=gpu_ctx).run(rec, dc[:-1], dc[1:])
    torch.cuda.synchronize()
    want = st.records_numpy(rec, 4).copy()
    state = st.rng_state
    st.close()
    assert (want["status"] == 0).all()
    np.testing.assert_array_equal(want["n_kp_cur"], sc.SYNTH_KEPT[N][1:] + (300,))
    out = _spawn(world, backend)
    for r in range(world):
        got = np.frombuffer(out[r][0], PAIR_RECORD_DTYPE)
        _same(got, want)  # every field, n_hypotheses too
        assert out[r][3] == state, f"rank {r}: final rng_state"
    assert out[0][1] == T_rel.cpu().numpy().tobytes(), "rank 0 T_rel"
    assert out[0][2] == T_abs.cpu().numpy().tobytes(), "rank 0 T_abs"
