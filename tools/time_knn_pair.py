"""What the one-call pair path costs in the k-NN modes: the drop-in's
visual_odometry_calculations (v3:384-408) in modes knn_sift, surf and flann with the fused
call (ops.KnnPairStream / dvo_knn_pair_run) against the same class with the fused path
disabled, i.e. operator by operator (detectAndCompute, knnMatch, the Python ratio loop,
KeyPoint_convert, findEssentialMat, recoverPose: what these modes did before D8).

Method: synthetic frames at 640x480 and 1280x720; per mode the two legs alternate run by run
in one process; a run is a warm-up pair and then `--pairs` consecutive pairs (frame i, i + 1)
on the host clock (every call ends synchronised); the value is the median of `--runs` runs.
Every run, the spread (max - min) and the library's source hash go to `--out`.  Verdict per
mode and size: the fused default stays only if its median beats the operator leg's best run
by more than 3 x that leg's spread, the margin of the project's A/B notes.

usage: python tools/time_knn_pair.py [--out profiles/knn_pair_time.txt] [--runs 5 --pairs 32]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "droplet_visual_odometry_amd", "dropin"))
import visual_odometry_v3 as v3  # noqa: E402
from droplet_visual_odometry_amd import build, cv  # noqa: E402
from droplet_visual_odometry_amd.synth import MARKER_LEN, SceneStream, marker_corners  # noqa: E402

MODES = ("knn_sift", "surf", "flann")


class OperatorByOperator(v3.VisualOdometry):  # an overridden per-pair method disables the fused path
    def compute_current_image_elements(self, input_image):
        return super().compute_current_image_elements(input_image)


def make(cls, mode, K, tmp):
    d = ", ".join(repr(float(v)) for v in K.ravel())
    y = os.path.join(tmp, "cal.yaml")
    with open(y, "w") as f:
        f.write(f"camera_matrix:\n  rows: 3\n  cols: 3\n  data: [{d}]\n"
                "distortion_coefficients:\n  rows: 1\n  cols: 5\n  data: [0.0, 0.0, 0.0, 0.0, 0.0]\n")
    return cls(mode=mode, calibration_file_path=y, controlled=True, real_marker_length=MARKER_LEN)


def run(vo, frames, corners, pairs):
    """Seconds for `pairs` consecutive pairs after a warm-up pair; the last absolute pose."""
    cv.setRNGSeed(0)
    T = vo.robot_curr_position
    T, _ = vo.visual_odometry_calculations(frames[0], frames[1], T, corners[0], corners[1])
    t0 = time.perf_counter()
    for i in range(1, pairs + 1):
        T, _ = vo.visual_odometry_calculations(frames[i], frames[i + 1], T, corners[i], corners[i + 1])
    return time.perf_counter() - t0, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_pair_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_knn_pair.py measures on the GPU; none is visible")
    lines = [f"time_knn_pair: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs} x {a.pairs} consecutive pairs after a warm-up pair; legs alternate; ms per pair",
             "one machine, one process; host clock around synchronous calls"]
    tmp = tempfile.mkdtemp()
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = SceneStream(W, H, device="cuda")
        n = a.pairs + 2
        frames = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).cpu().numpy()
        corners = [marker_corners(i, scene.K) for i in range(n)]
        for mode in a.modes.split(","):
            legs = {"fused": make(v3.VisualOdometry, mode, scene.K, tmp),
                    "operator": make(OperatorByOperator, mode, scene.K, tmp)}
            ms = {k: [] for k in legs}
            last = {}
            for _ in range(a.runs):
                for k, vo in legs.items():
                    t, T = run(vo, frames, corners, a.pairs)
                    ms[k].append(1e3 * t / a.pairs)
                    last[k] = T
            same = bool(np.array_equal(last["fused"], last["operator"]))
            used = legs["fused"]._pair_engine is not None and legs["operator"]._pair_engine is None
            f, o = ms["fused"], ms["operator"]
            spread = max(o) - min(o)
            verdict = float(np.median(f)) < min(o) - 3 * spread
            lines.append(f"{W}x{H} {mode}:")
            for k in ("fused", "operator"):
                lines.append(f"  {k:9s} runs {' '.join(f'{v:.3f}' for v in ms[k])}  median {np.median(ms[k]):.3f}"
                             f"  spread {max(ms[k]) - min(ms[k]):.3f}")
            lines.append(f"  operator / fused (medians) {np.median(o) / np.median(f):.2f}x; poses equal {same}; "
                         f"fused call in use {used}; fused median < operator best - 3 x operator spread "
                         f"({min(o) - 3 * spread:.3f}): {verdict}")
            del legs
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
