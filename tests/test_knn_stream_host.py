"""The k-NN modes' batched frame stream (dvo_knn_stream, stream.KnnFrameStream) without a GPU: the
new entry points are declared, exported and bound, the config struct has the header's layout, and
null handles are refused."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_knn_stream_create", "dvo_knn_stream_destroy", "dvo_knn_stream_process", "dvo_knn_stream_sync",
       "dvo_knn_stream_hip_stream", "dvo_knn_stream_get_features", "dvo_knn_stream_get_matches",
       "dvo_knn_stream_set_profiling", "dvo_knn_stream_stage_times", "dvo_test_knn_batch"]


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
    assert "typedef struct dvo_knn_stream dvo_knn_stream;" in hdr


def test_python_surface_exists():
    from droplet_visual_odometry_amd import ops, stream
    for name in ("new_records", "process", "sync", "records_numpy", "features", "matches", "close"):
        assert callable(getattr(stream.KnnFrameStream, name)), name
    assert callable(ops.test_knn_batch)


def test_config_struct_matches_header_layout():
    """dvo_knn_stream_config as a C compiler lays it out: 5 int32 (+ padding), 2 doubles, 9 doubles,
    2 doubles, int32 (+ padding), double."""
    from droplet_visual_odometry_amd._native import KnnStreamConfig
    f = KnnStreamConfig
    assert (f.width.offset, f.height.offset, f.max_frames.offset, f.detector.offset, f.feat_cap.offset) == \
        (0, 4, 8, 12, 16)
    assert (f.hessian_threshold.offset, f.ratio.offset, f.K.offset) == (24, 32, 40)
    assert (f.prob.offset, f.threshold.offset, f.max_iters.offset, f.dist_thresh.offset) == (112, 120, 128, 136)
    assert ctypes.sizeof(f) == 144
    # the header declares the same fields in the same order
    hdr = open(os.path.join(ROOT, "include", "dvo.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dvo_knn_stream_config;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in KnnStreamConfig._fields_]


def test_null_handles_are_refused():
    from droplet_visual_odometry_amd import _native
    lib = _native.load_library()
    n = ctypes.c_int()
    ms = (ctypes.c_double * 3)()
    assert lib.dvo_knn_stream_create(None, None, None) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_process(None, None, 2, 0, 0, None) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_sync(None) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_hip_stream(None) is None
    assert lib.dvo_knn_stream_get_features(None, 0, None, None, 0, ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_get_matches(None, 0, None, 0, ctypes.byref(n)) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_set_profiling(None, 1) == _native.DVO_EINVAL
    assert lib.dvo_knn_stream_stage_times(None, ms) == _native.DVO_EINVAL
    assert lib.dvo_test_knn_batch(None, None, None, None, 2, 2, 128, 0, 0.75, None, None, None, None, None, None, None,
                                  None) == _native.DVO_EINVAL
    lib.dvo_knn_stream_destroy(None)  # a no-op
