"""dist.ShardedKnnRunner on raw input: JPEG files with an undistorter (SIFT, FLANN) and colour
tensors (SURF, BFMatcher), two ranks on the box's one GPU over gloo and world size 1 over RCCL.
The stream is the 7 frames [0, 1, 2, 3, 2, 1, 0] of the 320x240 JPEG fixtures, 2 windows of 3 pairs.
The result must equal one KnnFrameStream.process_jpeg / process over all 7 frames plus
PoseTail.run: the gathered records, rank 0's T_rel and T_abs and every rank's final rng_state, byte
for byte."""
import os
import socket
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDER = [0, 1, 2, 3, 2, 1, 0]
N_PAIRS, WINDOWS = 3, 2
DEADLINE_S = 240.0  # workers are joined against it; never waited for unless one hangs
CASES = {"jpeg": ("sift", "flann"), "colour": ("surf", "bf")}
_REF = {}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _inputs(form, ctx):
    """(frames, corners, K of the stream, undistorter): 7 JPEG files remapped on the way, or 7 colour frames."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd.synth import marker_corners
    from test_gpu_knn_stream_input import H, W, camera, fixture_frames
    blobs, bgr = fixture_frames()
    K, dist, newK = camera()
    if form == "jpeg":
        frames, Ks, u = [blobs[i] for i in ORDER], newK, ops.Undistorter(K, dist, newK, W, H, ctx=ctx)
    else:
        frames, Ks, u = torch.from_numpy(bgr[ORDER]).to("cuda:0"), K, None
    corners = torch.from_numpy(np.stack([marker_corners(i, Ks) for i in ORDER])).to("cuda:0")
    return frames, corners, Ks, u


def _worker(rank, world, port, backend, form, out):
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
    from test_gpu_knn_stream_input import CAP, H, W
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ddist.init_process_group(backend, rank, world, device=dev, timeout_s=120.0)
    ctx = Context(0)
    frames, corners, K, u = _inputs(form, ctx)
    detector, matcher = CASES[form]
    run = ddist.ShardedKnnRunner(W, H, K, N_PAIRS, world, rank, MARKER_LEN, detector=detector, matcher=matcher,
                                 feat_cap=CAP, ctx=ctx, host_gather=backend == "gloo", undistort=u, raw_input=True)
    pending = []
    for w in range(WINDOWS):
        p0, p1, f0, f1 = ddist.shard_window(N_PAIRS, world, rank, w * N_PAIRS)
        for recs, T_rel, T_abs in run.step(frames[f0:f1], corners[f0:f1 - 1], corners[f0 + 1:f1]):
            pending.append((recs.clone(), T_rel.clone() if T_rel is not None else None, T_abs))
    assert run.drain() == []
    run.sync()
    rec = np.concatenate([r.cpu().numpy() for r, _, _ in pending]).tobytes()
    Trel = b"".join(T.cpu().numpy().tobytes() for _, T, _ in pending if T is not None)
    Tabs = b"".join(f.result().tobytes() for _, _, f in pending if f is not None)
    out[rank] = (rec, Trel, Tabs, run.rng_state if matcher == "flann" else None)
    run.close()
    dist.destroy_process_group()


def _spawn(world, backend, form):
    """Start the workers, join them against the deadline; at the deadline terminate them and fail."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, form, out), nprocs=world, join=False)
    end = time.monotonic() + DEADLINE_S
    while not ctx.join(timeout=1.0):  # raises when a worker failed
        if time.monotonic() > end:
            for p in ctx.processes:
                if p.is_alive():
                    p.terminate()
            pytest.fail(f"sharded workers still running after {DEADLINE_S:.0f} s")
    return dict(out)


def _single_rank(ctx, form):
    """Once per input form: one stream over all 7 frames and one pose tail."""
    import torch
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    from droplet_visual_odometry_amd.stream import KnnFrameStream, PoseTail
    from droplet_visual_odometry_amd.synth import MARKER_LEN
    from test_gpu_knn_stream_input import CAP, H, W
    if form not in _REF:
        frames, corners, K, u = _inputs(form, ctx)
        detector, matcher = CASES[form]
        st = KnnFrameStream(W, H, K, len(ORDER), detector=detector, feat_cap=CAP, ctx=ctx, matcher=matcher,
                            raw_input=True)
        rec = st.process_jpeg(frames, undistort=u) if form == "jpeg" else st.process(frames)
        st.sync()
        T_rel, T_abs = PoseTail(K, MARKER_LEN, ctx=ctx).run(rec, corners[:-1], corners[1:])
        torch.cuda.synchronize()
        r = np.frombuffer(rec.cpu().numpy().tobytes(), PAIR_RECORD_DTYPE)
        assert (r["status"] == 0).all() and (r["n_matches"] >= 5).all(), (r["status"], r["n_matches"])
        _REF[form] = dict(rec=rec.cpu().numpy().tobytes(), T_rel=T_rel.cpu().numpy(), T_abs=T_abs.cpu().numpy(),
                          state=st.rng_state if matcher == "flann" else None)
        st.close()
        if u is not None:
            u.close()
    return _REF[form]


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


@pytest.mark.parametrize("form", list(CASES))
def test_two_ranks_equal_the_single_stream(gpu_ctx, form):
    """2 + 1 pairs per rank and window: the input stage runs on every rank's own frames."""
    ref = _single_rank(gpu_ctx, form)
    _check(ref, _spawn(2, "gloo", form), 2, CASES[form][1])


@pytest.mark.parametrize("form", list(CASES))
def test_rccl_path(gpu_ctx, form):
    """World 1 over RCCL: no host synchronisation between the input stage, the phases and the collectives."""
    ref = _single_rank(gpu_ctx, form)
    _check(ref, _spawn(1, "nccl", form), 1, CASES[form][1])
