"""What the batched frame stream of the k-NN modes costs (dvo_knn_stream_process):
stream.KnnFrameStream.process on device-resident frames at 8, 32 and 128 frames per call against
ops.KnnPairStream.pair over the same consecutive pairs (host frames, reuse_prev: one frame up and
one record back per pair), in modes knn_sift and surf at 640x480 and 1280x720.

Method: synthetic frames; per mode and size the legs alternate run by run in one process; a run of
the pair leg is a warm-up pair and then every consecutive pair of the frames; a run of a stream leg
is one process call on n resident frames ended by a synchronise (after one warm-up call per n); host
clock, ms per pair; the value is the median of `--runs` runs.  The split of a stream call into
detection, matching + ratio test and geometry comes from HIP events on the stream in one extra
call per n.  The records of the legs must agree in every field but n_hypotheses (the schedules
differ).  Every run, the spread (max - min) and the library's source hash go to `--out`.
Verdict per stream leg: faster only if its median is below the pair leg's best run minus 3 x that
leg's spread, the margin of the project's A/B notes.

usage: python tools/time_knn_stream.py [--out profiles/knn_stream_time.txt] [--runs 5 --frames 128]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE  # noqa: E402
from droplet_visual_odometry_amd.stream import KnnFrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

MODES = {"knn_sift": "sift", "surf": "surf"}


def pair_leg(ks, frames):
    """Seconds for the consecutive pairs of `frames` after a warm-up pair; their records."""
    ks.pair(frames[0], frames[1])
    recs = np.zeros(len(frames) - 1, PAIR_RECORD_DTYPE)
    t0 = time.perf_counter()
    for i in range(len(frames) - 1):
        # the cache is valid only after a pair whose record status is 0
        reuse = i > 0 and recs[i - 1]["status"] == 0
        recs[i], _ = ks.pair(None if reuse else frames[i], frames[i + 1], reuse_prev=reuse)
    return time.perf_counter() - t0, recs


def stream_leg(st, d_frames, records):
    st.sync()
    t0 = time.perf_counter()
    st.process(d_frames, records, wait_torch=False)
    st.sync()
    return time.perf_counter() - t0


def same_records(a, b):
    return all(np.array_equal(a[n], b[n]) for n in PAIR_RECORD_DTYPE.names if n != "n_hypotheses")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_stream_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128, help="frames rendered: the pair leg's run and the largest call")
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--modes", default=",".join(MODES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_knn_stream.py measures on the GPU; none is visible")
    batches = [min(int(b), a.frames) for b in a.batches.split(",")]
    lines = [f"time_knn_stream: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs}; pair leg: {a.frames - 1} consecutive pairs (reuse_prev) after a warm-up pair; stream legs: "
             f"one call on n resident frames; legs alternate; ms per pair",
             "one machine, one process; host clock around synchronous calls / call + synchronise"]
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = SceneStream(W, H, device="cuda")
        d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, a.frames))) for i in range(0, a.frames, 8)])
        d_frames = d_frames.contiguous()
        frames = d_frames.cpu().numpy()
        torch.cuda.synchronize()
        for mode in a.modes.split(","):
            det = MODES[mode]
            ks = ops.KnnPairStream(W, H, scene.K, detector=det, matcher="bf")
            _, recs_pair = pair_leg(ks, frames)  # also the counts that size the stream's slots
            top = int(max(recs_pair["n_kp_prev"].max(), recs_pair["n_kp_cur"].max()))
            cap = (top + 255) // 256 * 256 + 256
            st = KnnFrameStream(W, H, scene.K, max(batches), detector=det, feat_cap=cap)
            records = {n: st.new_records(n - 1) for n in batches}
            torch.cuda.synchronize()
            for n in batches:
                stream_leg(st, d_frames[:n], records[n])  # warm-up
            ms = {"pair": []}
            ms.update({n: [] for n in batches})
            for _ in range(a.runs):
                t, recs_pair = pair_leg(ks, frames)
                ms["pair"].append(1e3 * t / (a.frames - 1))
                for n in batches:
                    ms[n].append(1e3 * stream_leg(st, d_frames[:n], records[n]) / (n - 1))
            same = all(same_records(st.records_numpy(records[n], n - 1), recs_pair[:n - 1]) for n in batches)
            ok = int((recs_pair["status"] == 0).sum())
            st.set_profiling(True)
            split = {}
            for n in batches:
                st.process(d_frames[:n], records[n], wait_torch=False)
                split[n] = st.stage_times()
            st.set_profiling(False)
            p = ms["pair"]
            spread = max(p) - min(p)
            bar = min(p) - 3 * spread
            lines.append(f"{W}x{H} {mode}: features per frame <= {top}, feat_cap {cap}, {ok} of {a.frames - 1} pairs "
                         f"status 0; records equal (n_hypotheses aside) {same}")
            lines.append(f"  pair path         runs {' '.join(f'{v:.3f}' for v in p)}  median {np.median(p):.3f}"
                         f"  spread {spread:.3f}")
            for n in batches:
                v, s = ms[n], split[n]
                tot = sum(s.values())
                lines.append(f"  stream {n:3d} frames runs {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}"
                             f"  spread {max(v) - min(v):.3f}  pair / stream {np.median(p) / np.median(v):.2f}x; "
                             f"median < pair best - 3 x pair spread ({bar:.3f}): {float(np.median(v)) < bar}")
                lines.append(f"    one call, device ms: detection {s['detect']:.3f}  matching + ratio {s['match']:.3f}"
                             f"  geometry {s['geometry']:.3f}  (of {tot:.3f}: "
                             f"{100 * s['detect'] / tot:.0f} / {100 * s['match'] / tot:.0f} / "
                             f"{100 * s['geometry'] / tot:.0f} %)")
            st.close()
            ks.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
