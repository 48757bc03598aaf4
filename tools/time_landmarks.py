"""What a landmark binding costs the ORB stream (dvo_stream_set_landmarks):
stream.FrameStream.process on device-resident frames without a binding (A) against the same stream
shape with a stream.Landmarks bound before every call (B: the two landmark kernels after the
records), at the benchmark's headline shape 1280x720 / 2000 features and at 320x240 / 300 features,
64 frames per call.

Method: synthetic frames; one process; two streams of one shape, A never bound, alternating run by
run.  A run is one process call on the resident frames ended by a synchronise (after a warm-up call
each), host clock, ms per call; B's bind_landmarks is inside the timed span.  The recoverPose +
records stage's device time (which the landmark kernels fall into) comes from HIP events
(dvo_stream_stage_times) in `--runs` further calls per stream, alternating in the same way.  Mean
matches and landmarks per pair come from the records and counts of the pairs with status 0.  Every
run, the spread (max - min) and the library's source hash go to `--out`.  Verdict per comparison:
different only if a median lies outside the other leg's best or worst run by 3 x that leg's spread,
the margin of the project's A/B notes.

usage: python tools/time_landmarks.py [--out profiles/landmarks_time.txt] [--runs 7 --frames 64] [--commit ID]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build  # noqa: E402
from droplet_visual_odometry_amd.stream import FrameStream, Landmarks  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402


def call_leg(fs, d_frames, records, lm):
    fs.sync()
    t0 = time.perf_counter()
    if lm is not None:
        fs.bind_landmarks(lm)
    fs.process(d_frames, records, wait_torch=False)
    fs.sync()
    return 1e3 * (time.perf_counter() - t0)


def pose_leg(fs, d_frames, records, lm):
    fs.set_profiling(True)
    if lm is not None:
        fs.bind_landmarks(lm)
    fs.process(d_frames, records, wait_torch=False)
    ms, _ = fs.stage_times()
    fs.set_profiling(False)
    return ms["recover_pose"]


def stats(v):
    return f"runs {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}  spread {max(v) - min(v):.3f}"


def verdict(a, b):
    """b against a by the spread rule: 'slower', 'faster' or 'same'."""
    sa = max(a) - min(a)
    mb = float(np.median(b))
    if mb > max(a) + 3 * sa:
        return "slower"
    if mb < min(a) - 3 * sa:
        return "faster"
    return "same"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmarks_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", default="1280x720x2000,320x240x300")
    ap.add_argument("--commit", default="", help="the commit the measured tree stands on (goes into the header)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_landmarks.py measures on the GPU; none is visible")
    lines = [f"time_landmarks: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}"
             + (f" on top of commit {a.commit}" if a.commit else ""),
             f"runs {a.runs}; one process call on {a.frames} resident frames, A no binding (default), "
             "B a Landmarks bound before each call; legs alternate; ms per call",
             "one machine, one process; host clock around (bind +) call + synchronise; "
             "recoverPose + records stage from HIP events"]
    for shape in a.shapes.split(","):
        W, H, NF = (int(v) for v in shape.split("x"))
        scene = SceneStream(W, H, device="cuda")
        d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, a.frames))) for i in range(0, a.frames, 8)])
        d_frames = d_frames.contiguous()
        torch.cuda.synchronize()
        pairs = a.frames - 1
        legs = {"A no binding": FrameStream(W, H, scene.K, nfeatures=NF, max_frames=a.frames),
                "B landmarks": FrameStream(W, H, scene.K, nfeatures=NF, max_frames=a.frames)}
        lms = {"A no binding": None, "B landmarks": Landmarks(pairs, NF, "cuda")}
        recs = {k: fs.new_records(pairs) for k, fs in legs.items()}
        torch.cuda.synchronize()
        for k, fs in legs.items():
            call_leg(fs, d_frames, recs[k], lms[k])  # warm-up (B: the scratch is allocated here)
        call = {k: [] for k in legs}
        pose = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fs in legs.items():
                call[k].append(call_leg(fs, d_frames, recs[k], lms[k]))
        for _ in range(a.runs):
            for k, fs in legs.items():
                pose[k].append(pose_leg(fs, d_frames, recs[k], lms[k]))
        lines.append(f"{W}x{H} nfeatures {NF}, {pairs} pairs per call, cap {NF} landmarks per pair")
        for k, fs in legs.items():
            fs.sync()
            r = FrameStream.records_numpy(recs[k], pairs)
            ok = r["status"] == 0
            extra = ""
            if lms[k] is not None:
                c = lms[k].counts.cpu().numpy()
                extra = f"  mean landmarks {c[ok].mean():.1f} (max {int(c.max())})"
            lines.append(f"  {k}: {int(ok.sum())} pairs status 0; per pair: mean matches {r['n_matches'][ok].mean():.1f}"
                         f"{extra}")
            lines.append(f"    whole call ms                  {stats(call[k])}")
            lines.append(f"    recoverPose + records stage ms {stats(pose[k])}")
        ka, kb = list(legs)
        same = FrameStream.records_numpy(recs[ka], pairs).tobytes() == FrameStream.records_numpy(recs[kb], pairs).tobytes()
        lines.append(f"  records of A and B byte-equal: {same}")
        lines.append(f"  B against A (median outside A's runs by 3 x A's spread): whole call {verdict(call[ka], call[kb])}"
                     f" ({np.median(call[kb]) / np.median(call[ka]):.3f}x, {np.median(call[kb]) - np.median(call[ka]):+.3f} ms),"
                     f" recoverPose + records stage {verdict(pose[ka], pose[kb])}"
                     f" ({np.median(pose[kb]) - np.median(pose[ka]):+.3f} ms)")
        for fs in legs.values():
            fs.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
