"""The sharded k-NN stream (dvo_knn_stream_detect / dvo_knn_stream_finish, dist.ShardedKnnRunner)
without a GPU: the new entry points are declared, exported and bound, null handles are refused,
the runner checks its arguments before it makes a context, and the sharded RNG plan's host twin
(dvo_flann_rng_shard_host, the text of the device plan) hands the theRNG state from rank to rank so
that every rank's start states are the whole-list plan's slice for its pairs and every rank ends a
window with the whole list's final state."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_knn_stream_detect", "dvo_knn_stream_finish", "dvo_flann_rng_shard_host"]
COUNTS = [0, 1, 2, 3, 5, 100, 101, 102, 256, 257, 0, 300, 1, 64, 513, 2]
WORLDS = (1, 2, 3, 5, 16)  # 15 pairs: world 16 leaves rank 15 without a pair


def test_new_symbols_declared_exported_bound():
    from droplet_visual_odometry_amd import _native, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    lib = _native.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in _native._SIGNATURES and getattr(lib, name).argtypes is not None, name


def test_python_surface_exists():
    from droplet_visual_odometry_amd import dist, ops, stream
    assert callable(stream.KnnFrameStream.detect) and callable(stream.KnnFrameStream.finish)
    assert callable(ops.flann_rng_shard_host)
    for name in ("step", "drain", "reset_pose", "sync", "close"):
        assert callable(getattr(dist.ShardedKnnRunner, name)), name
    assert isinstance(dist.ShardedKnnRunner.rng_state, property)


def test_null_handles_are_refused():
    from droplet_visual_odometry_amd import _native
    lib = _native.load_library()
    st = ctypes.c_uint64()
    assert lib.dvo_knn_stream_detect(None, None, 2, 0, 0, None) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_finish(None, None, None, 1, 0) == _native.DVO_EINVAL
    # two frames need counts and starts
    assert lib.dvo_flann_rng_shard_host(1, None, 2, 8, 5, None, 1, 0, None, ctypes.byref(st),
                                        ctypes.byref(st)) == _native.DVO_EINVAL


@pytest.mark.parametrize("kw", [dict(matcher="kdtree"), dict(detector="orb"), dict(rank=2), dict(rank=-1),
                                dict(window_pairs=0), dict(matcher="bf", rng_state=1)])
def test_runner_arguments_checked_before_any_device_work(kw):
    """These raise ValueError before a context exists, so they need no GPU."""
    from droplet_visual_odometry_amd.dist import ShardedKnnRunner
    args = dict(window_pairs=4, world=2, rank=0)
    args.update(kw)
    with pytest.raises(ValueError):
        ShardedKnnRunner(640, 480, np.eye(3), marker_length=0.1, **args)


def _sharded_window(ops, ddist, counts, cap, trees, state, world):
    """One window over counts (len - 1 pairs) on `world` ranks: every rank's own draws word with
    world 1 first, then the array of them fed to every rank.  Returns (starts in pair order, the
    ranks' final states, the draws words)."""
    n_pairs = len(counts) - 1
    shards = [ddist.shard_window(n_pairs, world, r) for r in range(world)]
    own = [ops.flann_rng_shard_host(counts[f0:f1], cap, trees, state)[2] for _, _, f0, f1 in shards]
    starts, finals = [], []
    for r, (p0, p1, f0, f1) in enumerate(shards):
        s, fin, own_r = ops.flann_rng_shard_host(counts[f0:f1], cap, trees, state, shard_draws=own, world=world, rank=r)
        assert own_r == own[r] and len(s) == p1 - p0
        starts.append(s)
        finals.append(fin)
    return np.concatenate(starts), finals, own


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("cap,trees", [(520, 5), (520, 3), (256, 5)])
def test_shard_plan_equals_the_whole_list_plan(cap, trees, world):
    from droplet_visual_odometry_amd import dist as ddist, ops
    state = 0xFFFFFFFF
    want_starts, want_final = ops.flann_rng_plan_host(COUNTS, cap, trees, state)
    starts, finals, own = _sharded_window(ops, ddist, COUNTS, cap, trees, state, world)
    np.testing.assert_array_equal(starts, want_starts)
    assert finals == [want_final] * world
    assert want_final != state
    if world == 16:
        assert ddist.shard_window(len(COUNTS) - 1, world, 15)[:2] == (15, 15) and own[15] == 0
    # the draws words are the plan's own count: trees (2 nt - 1) per built pair
    brings = [0 if c > cap else c for c in COUNTS]
    total = sum(trees * (2 * brings[p + 1] - 1) for p in range(len(COUNTS) - 1) if brings[p] >= 1 and brings[p + 1] >= 2)
    assert sum(own) == total
    if world == 16:
        assert own[0] == 0  # rank 0's only pair (0, 1) builds nothing
    # a second window chained from that state: the list reversed, so it starts with the first
    # window's last frame and the marked and empty frames fall on other shard boundaries
    second = COUNTS[::-1]
    want2, want_final2 = ops.flann_rng_plan_host(second, cap, trees, want_final)
    starts2, finals2, _ = _sharded_window(ops, ddist, second, cap, trees, finals[-1], world)
    np.testing.assert_array_equal(starts2, want2)
    assert finals2 == [want_final2] * world


def test_entry_of_the_own_rank_is_not_read():
    from droplet_visual_odometry_amd import ops
    a = ops.flann_rng_shard_host(COUNTS[:6], 520, 5, 0x1234567, shard_draws=[7, 0, 11], world=3, rank=1)
    b = ops.flann_rng_shard_host(COUNTS[:6], 520, 5, 0x1234567, shard_draws=[7, 2 ** 63 + 12345, 11], world=3, rank=1)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:]
    # and the hand-off is a jump: 7 draws before, 11 after
    _, after7 = ops.flann_rng_plan_host([3, 4], 8, 1, 0x1234567)  # one pair of 1 * (2 * 4 - 1) = 7 draws
    assert a[0][0] == after7
    _, after_all = ops.flann_rng_plan_host(COUNTS[:6], 520, 5, after7)
    assert a[1] == ops.flann_rng_plan_host([3, 6], 8, 1, after_all)[1]  # 2 * 6 - 1 = 11 draws more


@pytest.mark.parametrize("kw", [dict(world=0), dict(world=1025), dict(world=2, rank=2), dict(world=2, rank=-1),
                                dict(trees=0), dict(trees=65), dict(cap=0)])
def test_shard_host_bad_arguments(kw):
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    args = dict(counts=[3, 4], cap=8, trees=5)
    args.update(kw)
    with pytest.raises(DVOError):
        ops.flann_rng_shard_host(**args)
