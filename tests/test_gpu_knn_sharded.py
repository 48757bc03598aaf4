"""dist.ShardedKnnRunner: one pose stream of the k-NN modes (SIFT or SURF, BFMatcher or FLANN)
sharded across ranks, the FLANN theRNG state handed from rank to rank on the device.  Two ranks
share the box's one GPU over gloo (host_gather), and world size 1 runs the RCCL path.  The result
must equal one KnnFrameStream.process over all frames plus PoseTail.run: both ranks' gathered
records in every field, rank 0's T_rel and T_abs byte for byte, and every rank's final rng_state."""
import os
import socket
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 480
DEADLINE_S = 240.0  # workers are joined against it; never waited for unless one hangs
COMBOS = [("sift", "bf"), ("surf", "bf"), ("sift", "flann"), ("surf", "flann")]
_COUNTS, _REF = {}, {}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _stream(F, blank):
    """F synthetic frames + marker corners; frames in `blank` are featureless and keep the previous
    frame's corners."""
    from conftest import synth_frames
    from droplet_visual_odometry_amd.synth import marker_corners
    frames, K = synth_frames(W, H, range(F))
    frames = frames.copy()
    corners = [marker_corners(i, K) for i in range(F)]
    for b in blank:
        frames[b] = 90
        corners[b] = corners[b - 1]
    return frames, np.stack(corners), K


def _worker(rank, world, port, backend, detector, matcher, cap, n_pairs, windows, blank, kw, out):
    import faulthandler
    import sys
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
    frames, corners, K = _stream(n_pairs * windows + 1, blank)
    d_frames = torch.from_numpy(frames).to(dev)
    d_corners = torch.from_numpy(corners).to(dev)
    run = ddist.ShardedKnnRunner(W, H, K, n_pairs, world, rank, MARKER_LEN, detector=detector, matcher=matcher,
                                 feat_cap=cap, ctx=Context(0), host_gather=backend == "gloo", **kw)
    pending = []
    for w in range(windows):
        p0, p1, f0, f1 = ddist.shard_window(n_pairs, world, rank, w * n_pairs)
        # device copies on torch's stream, read back only at the end: no host sync between windows
        # on the RCCL path, so the send slots are reused while earlier collectives are queued
        for recs, T_rel, T_abs in run.step(d_frames[f0:f1], d_corners[f0:f1 - 1], d_corners[f0 + 1:f1]):
            pending.append((recs.clone(), T_rel.clone() if T_rel is not None else None, T_abs))
    assert run.drain() == []
    run.sync()
    rec = np.concatenate([r.cpu().numpy() for r, _, _ in pending]).tobytes()
    Trel = b"".join(T.cpu().numpy().tobytes() for _, T, _ in pending if T is not None)
    Tabs = b"".join(f.result().tobytes() for _, _, f in pending if f is not None)
    out[rank] = (rec, Trel, Tabs, run.rng_state if matcher == "flann" else None)
    run.close()
    dist.destroy_process_group()


def _spawn(world, backend, detector, matcher, cap, n_pairs, windows, blank, kw):
    """Start the workers, join them against the deadline; at the deadline terminate them and fail."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, detector, matcher, cap, n_pairs, windows, blank, kw, out),
                   nprocs=world, join=False)
    end = time.monotonic() + DEADLINE_S
    while not ctx.join(timeout=1.0):  # raises when a worker failed
        if time.monotonic() > end:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            pytest.fail(f"sharded workers still running after {DEADLINE_S:.0f} s")
    return dict(out)


def _cap(detector, F, ctx):
    """The largest detector count of the case's frames + 37 (as tests/test_gpu_knn_stream_flann.py)."""
    import torch
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    if detector not in _COUNTS:  # once per detector: a BF stream with room for every frame's features
        frames, _, K = _stream(19, ())
        st = KnnFrameStream(W, H, K, len(frames), detector=detector, feat_cap=4096, ctx=ctx)
        rec = st.process(torch.from_numpy(frames).cuda())
        st.sync()
        rec = st.records_numpy(rec, len(frames) - 1)
        st.close()
        _COUNTS[detector] = [int(rec["n_kp_prev"][0])] + [int(c) for c in rec["n_kp_cur"]]
        assert 0 < max(_COUNTS[detector]) <= 4096
    return max(_COUNTS[detector][:F]) + 37


def _single_rank(ctx, detector, matcher, F, blank):
    """Once per (detector, matcher, F, blank): one stream over all frames and one pose tail."""
    import torch
    from droplet_visual_odometry_amd._native import DVO_ENOFEAT, PAIR_RECORD_DTYPE
    from droplet_visual_odometry_amd.stream import KnnFrameStream, PoseTail
    from droplet_visual_odometry_amd.synth import MARKER_LEN
    key = detector, matcher, F, tuple(blank)
    if key not in _REF:
        frames, corners, K = _stream(F, blank)
        cap = _cap(detector, F, ctx)
        st = KnnFrameStream(W, H, K, F, detector=detector, feat_cap=cap, ctx=ctx, matcher=matcher)
        rec = st.process(torch.from_numpy(frames).cuda())
        st.sync()
        dc = torch.from_numpy(corners).cuda()
        T_rel, T_abs = PoseTail(K, MARKER_LEN, ctx=ctx).run(rec, dc[:-1], dc[1:])
        torch.cuda.synchronize()
        status = np.frombuffer(rec.cpu().numpy().tobytes(), PAIR_RECORD_DTYPE)["status"]
        for p in range(F - 1):  # the non-blank pairs succeed, a blank frame's two pairs have no features
            assert status[p] == (DVO_ENOFEAT if p in blank or p + 1 in blank else 0), (p, status[p])
        _REF[key] = dict(cap=cap, rec=rec.cpu().numpy().tobytes(), T_rel=T_rel.cpu().numpy(), T_abs=T_abs.cpu().numpy(),
                         state=st.rng_state if matcher == "flann" else None)
        st.close()
    return _REF[key]


def _check(ref, out, ranks, matcher):
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    want = np.frombuffer(ref["rec"], PAIR_RECORD_DTYPE)
    for r in range(ranks):
        got = np.frombuffer(out[r][0], PAIR_RECORD_DTYPE)
        assert len(got) == len(want)
        for name in PAIR_RECORD_DTYPE.names:  # every field, n_hypotheses too
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"rank {r}: {name}")
        assert out[r][0] == ref["rec"], f"rank {r}: gathered records differ from the single stream's"
        if matcher == "flann":
            assert out[r][3] == ref["state"], f"rank {r}: final rng_state"
    assert out[0][1] == ref["T_rel"].tobytes(), "rank 0 T_rel"
    got_Tabs = np.frombuffer(out[0][2]).reshape(-1, 4, 4)
    bad = [i for i in range(len(ref["T_abs"])) if got_Tabs[i].tobytes() != ref["T_abs"][i].tobytes()]
    assert not bad, f"rank 0 T_abs differs at pairs {bad}"


@pytest.mark.parametrize("detector,matcher", COMBOS)
def test_two_ranks_equal_the_single_stream(gpu_ctx, detector, matcher):
    """(a) 7 frames in two windows of 3 pairs, 2 + 1 pairs per rank: the state crosses a rank
    boundary and a window boundary."""
    ref = _single_rank(gpu_ctx, detector, matcher, 7, ())
    out = _spawn(2, "gloo", detector, matcher, ref["cap"], 3, 2, (), {})
    _check(ref, out, 2, matcher)


@pytest.mark.parametrize("detector", ("sift", "surf"))
def test_blank_frame_at_the_rank_boundary(gpu_ctx, detector):
    """(b) Frame 2 blank: rank 0's last pair and rank 1's only pair of window 0 build nothing, so
    rank 1's draws word is 0 and window 1 starts from what pair 0 left; T_abs skips the failed pairs
    as the single-rank tail does."""
    ref = _single_rank(gpu_ctx, detector, "flann", 7, (2,))
    assert np.array_equal(ref["T_abs"][1], ref["T_abs"][0]) and np.array_equal(ref["T_abs"][2], ref["T_abs"][0])
    out = _spawn(2, "gloo", detector, "flann", ref["cap"], 3, 2, (2,), {})
    _check(ref, out, 2, "flann")


@pytest.mark.parametrize("detector,matcher", [("sift", "flann"), ("surf", "bf")])
def test_rccl_path_reuses_the_send_slots(gpu_ctx, detector, matcher):
    """(c) World 1 over RCCL, 9 windows of 2 pairs: no host synchronisation between the windows, so
    the two send slots are rewritten while earlier collectives and tails are still queued.  A
    missing stream order shows as a mismatch with the single stream."""
    ref = _single_rank(gpu_ctx, detector, matcher, 19, ())
    out = _spawn(1, "nccl", detector, matcher, ref["cap"], 2, 9, (), {})
    _check(ref, out, 1, matcher)


@pytest.mark.parametrize("detector,kw", [("sift", dict(detect_group=2)), ("surf", dict(surf_group=2))])
def test_group_detection_in_the_sharded_stream(gpu_ctx, detector, kw):
    """(d) The shape of (a) with the group detectors, FLANN."""
    ref = _single_rank(gpu_ctx, detector, "flann", 7, ())
    out = _spawn(2, "gloo", detector, "flann", ref["cap"], 3, 2, (), kw)
    _check(ref, out, 2, "flann")
