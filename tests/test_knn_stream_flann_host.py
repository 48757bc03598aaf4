"""The batched k-NN stream's FLANN mode (dvo_knn_stream_set_flann, stream.KnnFrameStream(matcher=
"flann")) without a GPU: the new entry points are declared, exported and bound, null handles are
refused, the footprint equals the documented formula, and the RNG plan's host twin (the device
kernel's text) gives every pair's start state and the call's final state as the oracle's
generator does, stepped built pair by built pair."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_knn_stream_set_flann", "dvo_knn_stream_set_rng_state", "dvo_knn_stream_get_rng_state",
       "dvo_knn_stream_flann_bytes", "dvo_flann_rng_plan_host", "dvo_test_flann_batch"]
COUNTS = [0, 1, 2, 3, 5, 100, 101, 102, 256, 257, 0, 300, 1, 64, 513, 2]


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
    from droplet_visual_odometry_amd import ops, stream
    assert callable(stream.KnnFrameStream.set_flann)
    assert isinstance(stream.KnnFrameStream.rng_state, property) and stream.KnnFrameStream.rng_state.fset is not None
    for name in ("test_flann_batch", "flann_rng_plan_host", "knn_stream_flann_bytes"):
        assert callable(getattr(ops, name)), name


def test_null_handles_are_refused():
    from droplet_visual_odometry_amd import _native
    lib = _native.load_library()
    st = ctypes.c_uint64()
    n = ctypes.c_int()
    assert lib.dvo_knn_stream_set_flann(None, 5, 50) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_set_rng_state(None, 1) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_get_rng_state(None, ctypes.byref(st)) == _native.DVO_EINVAL
    assert lib.dvo_test_flann_batch(None, None, None, 2, 2, 128, 5, 50, 1, 0, None, None, None, ctypes.byref(st),
                                    ctypes.byref(n), ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_flann_rng_plan_host(1, None, 2, 8, 5, None, ctypes.byref(st)) == _native.DVO_EINVAL


@pytest.mark.parametrize("F,C,T", [(2, 2, 1), (5, 520, 5), (128, 4096, 64)])
def test_footprint_is_the_documented_formula(F, C, T):
    from droplet_visual_odometry_amd import ops
    P = F - 1
    assert ops.knn_stream_flann_bytes(F, C, T) == P * (84 * C + 32 * T * C + 512 * T + 20) + 512 * C + 24
    hdr = open(os.path.join(ROOT, "include", "dvo.h")).read()
    assert "P (84 C + 32 T C + 512 T + 20) + 512 C + 24" in hdr


@pytest.mark.parametrize("F,C,T", [(1, 520, 5), (65537, 520, 5), (5, 1, 5), (5, 65537, 5), (5, 520, 0), (5, 520, 65)])
def test_footprint_of_bad_arguments_is_zero(F, C, T):
    from droplet_visual_odometry_amd import ops
    assert ops.knn_stream_flann_bytes(F, C, T) == 0


def _oracle_plan(oracle_mod, counts, cap, trees, state):
    """Start states and the final state with the oracle's generator, stepped through every built pair."""
    brings = [0 if c > cap else c for c in counts]
    starts = []
    for p in range(len(counts) - 1):
        starts.append(state)
        if brings[p] >= 1 and brings[p + 1] >= 2:
            state = oracle_mod.flann_rng_after(state, [brings[p + 1]], trees)
    return np.array(starts, np.uint64), state


@pytest.mark.parametrize("counts,cap,trees,state", [
    (COUNTS, 520, 5, 0xFFFFFFFF),
    (COUNTS, 520, 3, 0x1234567),
    (COUNTS, 256, 5, 0xFFFFFFFF),  # 257, 300 and 513 are marked: five more pairs build nothing
    ([65536, 65536, 0, 40000, 1, 65536, 3, 65536], 65536, 64, 0xFFFFFFFF),
])
def test_rng_plan_host_equals_the_oracle_generator(oracle_mod, counts, cap, trees, state):
    from droplet_visual_odometry_amd import ops
    starts, final = ops.flann_rng_plan_host(counts, cap, trees, state)
    want_starts, want_final = _oracle_plan(oracle_mod, counts, cap, trees, state)
    np.testing.assert_array_equal(starts, want_starts)
    assert final == want_final
    assert final != state


def test_rng_plan_host_bad_arguments():
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    for kw in (dict(trees=0), dict(trees=65), dict(cap=0)):
        args = dict(counts=[3, 4], cap=8, trees=5)
        args.update(kw)
        with pytest.raises(DVOError):
            ops.flann_rng_plan_host(**args)


@pytest.mark.parametrize("kw", [dict(matcher="kdtree"), dict(matcher="flann", trees=0), dict(matcher="flann", trees=65),
                                dict(matcher="flann", checks=0), dict(matcher="bf", rng_state=1)])
def test_stream_arguments_checked_before_any_device_work(kw):
    """These raise ValueError before a context is made, so they need no GPU."""
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    with pytest.raises(ValueError):
        KnnFrameStream(640, 480, np.eye(3), 4, **kw)
