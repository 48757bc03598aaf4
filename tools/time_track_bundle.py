"""What a bundle binding costs the ORB stream (dvo_stream_set_track_bundle).

One process: stream.FrameStream.process on device-resident frames with a Landmarks, a Tracks, a
TrackPoses and a RefinedLandmarks bound before every call (A) against the same stream shape with a
TrackBundle bound too (B: the bundle kernel follows the refine kernel, a workgroup per pair), at
the benchmark's headline shape 1280x720 / 2000 features and at 320x240 / 300 features, 64 frames
per call.  Two streams of one shape alternate run by run.  A run is one process call on the
resident frames ended by a synchronise (after a warm-up call each), host clock, ms per call, the
bindings inside the timed span.  The device time of the recoverPose + records stage (which the
landmark, track, pose, id, refine and bundle kernels fall into) comes from HIP events
(dvo_stream_stage_times) in `--runs` further calls per stream, alternating in the same way; the
match stage is reported as a control.

Verdict per comparison: different only if a median lies outside the other leg's best or worst run
by 3 x that leg's spread, the margin of the project's A/B notes.  The binding is opt-in, so its
cost is reported, not gated.  Not measured here: the k-NN stream, and batches of thousands of
pairs.  Everything goes to `--out`.

usage: python tools/time_track_bundle.py [--out profiles/track_bundle_time.txt] [--runs 7 --frames 64] [--commit ID]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from droplet_visual_odometry_amd import build  # noqa: E402
from droplet_visual_odometry_amd.stream import (FrameStream, Landmarks, RefinedLandmarks, TrackBundle, TrackPoses,  # noqa: E402
                                                Tracks)
from time_tracks import frames_of, stats, verdict  # noqa: E402


def bind(fs, lm, tr, tp, rf, bd):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.bind_track_poses(tp)
    fs.bind_refine(rf)
    if bd is not None:
        fs.bind_bundle(bd)


def call_leg(fs, d_frames, records, *bufs):
    fs.sync()
    t0 = time.perf_counter()
    bind(fs, *bufs)
    fs.process(d_frames, records, wait_torch=False)
    fs.sync()
    return 1e3 * (time.perf_counter() - t0)


def stage_leg(fs, d_frames, records, *bufs):
    fs.set_profiling(True)
    bind(fs, *bufs)
    fs.process(d_frames, records, wait_torch=False)
    ms, _ = fs.stage_times()
    fs.set_profiling(False)
    return ms["recover_pose"], ms["match"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bundle_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", default="1280x720x2000,320x240x300")
    ap.add_argument("--commit", default="", help="the commit the measured tree stands on (goes into the header)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_track_bundle.py measures on the GPU; none is visible")
    lines = [f"time_track_bundle: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}"
             + (f" on top of commit {a.commit}" if a.commit else ""),
             f"runs {a.runs}; one process call on {a.frames} resident frames, A a Landmarks, a Tracks, a TrackPoses and a "
             "RefinedLandmarks bound before each call, B a TrackBundle too (6 views, 5 steps, lambda 1e-6, Huber 1 px, "
             "inliers 2 px, min_points 8, pairs and points); legs alternate; ms per call",
             "one machine, one process; host clock around bind + call + synchronise; "
             "recoverPose + records stage and match stage from HIP events",
             "not measured: the k-NN stream, batches of thousands of pairs"]
    for shape in a.shapes.split(","):
        W, H, NF, K, d_frames = frames_of(shape, a.frames)
        pairs = a.frames - 1
        names = ("A landmarks + tracks + poses + refine", "B landmarks + tracks + poses + refine + bundle")
        legs = {k: FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames) for k in names}
        bufs = {k: (Landmarks(pairs, NF, "cuda"), Tracks(pairs, NF, "cuda"), TrackPoses(pairs, "cuda"),
                    RefinedLandmarks(pairs, NF, "cuda"), TrackBundle(pairs, NF, "cuda") if k == names[1] else None)
                for k in names}
        recs = {k: fs.new_records(pairs) for k, fs in legs.items()}
        torch.cuda.synchronize()
        for k, fs in legs.items():
            call_leg(fs, d_frames, recs[k], *bufs[k])  # warm-up (the scratch is allocated here)
        call = {k: [] for k in legs}
        pose = {k: [] for k in legs}
        match = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fs in legs.items():
                call[k].append(call_leg(fs, d_frames, recs[k], *bufs[k]))
        for _ in range(a.runs):
            for k, fs in legs.items():
                p, m = stage_leg(fs, d_frames, recs[k], *bufs[k])
                pose[k].append(p)
                match[k].append(m)
        lines.append(f"{W}x{H} nfeatures {NF}, {pairs} pairs per call, cap {NF} landmarks per pair")
        for k, fs in legs.items():
            fs.sync()
            lm, tr, tp, rf, bd = bufs[k]
            r = FrameStream.records_numpy(recs[k], pairs)
            sc = tr.scales_numpy()
            extra = ""
            if bd is not None:
                b = bd.numpy()
                on = b["status"] != 1
                extra = (f"; bundle: status histogram (OK, NONE, DEGENERATE, NOT_IMPROVED) "
                         f"{np.bincount(b['status'], minlength=4).tolist()}, cameras histogram "
                         f"{np.bincount(b['n_cams'], minlength=9)[2:].tolist()}, {int(b['n_points'].sum())} points, "
                         f"{int(b['n_obs'].sum())} observations, mean rms0 {b['rms0'][on].mean():.3f} px, mean rms "
                         f"{b['rms'][on].mean():.3f} px")
            lines.append(f"  {k}: {int((r['status'] == 0).sum())} pairs status 0; mean n_common "
                         f"{sc['n_common'][1:].mean():.1f}{extra}")
            lines.append(f"    whole call ms                  {stats(call[k])}")
            lines.append(f"    recoverPose + records stage ms {stats(pose[k])}")
            lines.append(f"    match stage ms                 {stats(match[k])}")
        ka, kb = names

        def raw(t):
            return t.cpu().numpy().tobytes()

        same = all(raw(getattr(x, f)) == raw(getattr(y, f)) for x, y in zip(bufs[ka][:4], bufs[kb][:4])
                   for f in ("entries", "counts", "links", "scales", "poses", "refined", "ids") if hasattr(x, f))
        lines.append(f"  landmarks, links, scales, poses, refined and ids of A and B byte-equal: {same}; records byte-equal: "
                     f"{FrameStream.records_numpy(recs[ka], pairs).tobytes() == FrameStream.records_numpy(recs[kb], pairs).tobytes()}")
        lines.append(f"  B against A (median outside A's runs by 3 x A's spread): whole call {verdict(call[ka], call[kb])}"
                     f" ({np.median(call[kb]) / np.median(call[ka]):.3f}x, {np.median(call[kb]) - np.median(call[ka]):+.3f} ms),"
                     f" recoverPose + records stage {verdict(pose[ka], pose[kb])}"
                     f" ({np.median(pose[kb]) - np.median(pose[ka]):+.3f} ms),"
                     f" match stage {verdict(match[ka], match[kb])} ({np.median(match[kb]) - np.median(match[ka]):+.3f} ms)")
        for fs in legs.values():
            fs.close()
        del legs, bufs, recs, d_frames
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
