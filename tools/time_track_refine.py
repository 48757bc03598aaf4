"""What a refine binding costs the ORB stream (dvo_stream_set_track_refine).

One process: stream.FrameStream.process on device-resident frames with a Landmarks, a Tracks and a
TrackPoses bound before every call (A) against the same stream shape with a RefinedLandmarks bound
too (B: the link kernel also writes the full links, and the id launches and the refine kernel
follow the pose kernel), at the benchmark's headline shape 1280x720 / 2000 features and at
320x240 / 300 features, 64 frames per call.  Two streams of one shape alternate run by run.  A run
is one process call on the resident frames ended by a synchronise (after a warm-up call each),
host clock, ms per call, the bindings inside the timed span.  The device time of the recoverPose +
records stage (which the landmark, track, pose, id and refine kernels fall into) comes from HIP
events (dvo_stream_stage_times) in `--runs` further calls per stream, alternating in the same way;
the match stage is reported as a control.

Verdict per comparison: different only if a median lies outside the other leg's best or worst run
by 3 x that leg's spread, the margin of the project's A/B notes.  The binding is opt-in, so its
cost is reported, not gated.  Not measured here: the k-NN stream, and batches of thousands of
pairs.  Everything goes to `--out`.

usage: python tools/time_track_refine.py [--out profiles/track_refine_time.txt] [--runs 7 --frames 64] [--commit ID]"""
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
from droplet_visual_odometry_amd.stream import FrameStream, Landmarks, RefinedLandmarks, TrackPoses, Tracks  # noqa: E402
from time_tracks import frames_of, stats, verdict  # noqa: E402


def bind(fs, lm, tr, tp, rf):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    fs.bind_track_poses(tp)
    if rf is not None:
        fs.bind_refine(rf)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_refine_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", default="1280x720x2000,320x240x300")
    ap.add_argument("--commit", default="", help="the commit the measured tree stands on (goes into the header)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_track_refine.py measures on the GPU; none is visible")
    lines = [f"time_track_refine: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}"
             + (f" on top of commit {a.commit}" if a.commit else ""),
             f"runs {a.runs}; one process call on {a.frames} resident frames, A a Landmarks, a Tracks and a TrackPoses bound "
             "before each call, B a RefinedLandmarks too (6 views, 5 steps, Huber 1 px, inliers 2 px, ids and refined); "
             "legs alternate; ms per call",
             "one machine, one process; host clock around bind + call + synchronise; "
             "recoverPose + records stage and match stage from HIP events",
             "not measured: the k-NN stream, batches of thousands of pairs"]
    for shape in a.shapes.split(","):
        W, H, NF, K, d_frames = frames_of(shape, a.frames)
        pairs = a.frames - 1
        names = ("A landmarks + tracks + poses", "B landmarks + tracks + poses + refine")
        legs = {k: FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames) for k in names}
        bufs = {k: (Landmarks(pairs, NF, "cuda"), Tracks(pairs, NF, "cuda"), TrackPoses(pairs, "cuda"),
                    RefinedLandmarks(pairs, NF, "cuda") if k == names[1] else None) for k in names}
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
            lm, tr, tp, rf = bufs[k]
            r = FrameStream.records_numpy(recs[k], pairs)
            sc = tr.scales_numpy()
            extra = ""
            if rf is not None:
                ref = np.concatenate([rf.numpy(p, lm.count(p)) for p in range(pairs)])
                ids = np.concatenate([rf.ids_numpy(p, lm.count(p)) for p in range(pairs)])
                fit = ref["status"] == 0
                extra = (f"; refine: {len(ref)} landmarks, {int(fit.sum())} status 0, {int((ref['status'] == 2).sum())} "
                         f"degenerate, views histogram {np.bincount(ref['views'], minlength=9)[2:].tolist()}, mean rms "
                         f"{ref['rms'][fit].mean():.3f} px, max age {int(ids['age'].max())}")
            lines.append(f"  {k}: {int((r['status'] == 0).sum())} pairs status 0; mean n_common "
                         f"{sc['n_common'][1:].mean():.1f}{extra}")
            lines.append(f"    whole call ms                  {stats(call[k])}")
            lines.append(f"    recoverPose + records stage ms {stats(pose[k])}")
            lines.append(f"    match stage ms                 {stats(match[k])}")
        ka, kb = names

        def raw(t):
            return t.cpu().numpy().tobytes()

        same = all(raw(getattr(x, f)) == raw(getattr(y, f)) for x, y in zip(bufs[ka][:3], bufs[kb][:3])
                   for f in ("entries", "counts", "links", "scales", "poses") if hasattr(x, f))
        lines.append(f"  landmarks, links, scales and poses of A and B byte-equal: {same}; records byte-equal: "
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
