"""What the group SURF detector buys the batched k-NN stream ("Group SURF
detection"): stream.KnnFrameStream.process on `--frames` device-resident frames in mode surf with
surf_group 0 (frame by frame: the baseline) against surf_group 4, 16 and 32, at 640x480 and
1280x720.

Method: synthetic frames; per size one stream per leg on one context, in one process; the legs
alternate run by run, after one warm-up call each; a run is one process call ended by a
synchronise.  Detection time is the stream's own stage events (dvo_knn_stream_stage_times), in ms
per frame; the whole call is the sum of the three stages, in ms per pair.  The value is the median
of `--runs` runs, the spread max - min.  The records of every leg must equal the baseline's in every
field (asserted).  Verdict per group leg: faster only if its median is below the baseline's best run
minus 3 x the baseline's spread, the margin of the project's A/B notes.  Every run and the
library's source hash go to `--out`.  `--plain-describe G,...` adds legs whose group detector
describes every frame's list in a plain stride (DVO_SURF_LARGE_FIRST=0 while their stream is made)
beside the default, the large windows first from per-frame queues: the A/B of that queue, same
process, same rule, against the plain leg of the same group.

usage: python tools/time_surf_batch.py [--out profiles/surf_batch_time.txt] [--runs 5 --frames 128]
       python tools/time_surf_batch.py --trace-leg G --sizes 640x480   (one leg, no file: the
       workload of a kernel trace, e.g. rocprofv3 --kernel-trace --stats -- python tools/...)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE  # noqa: E402
from droplet_visual_odometry_amd.stream import KnnFrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

THRESHOLD = 400.0  # SURF_create(400), the reference's


def run(st, d_frames, records):
    """One profiled call: the stage times (device ms)."""
    st.process(d_frames, records, wait_torch=False)
    s = st.stage_times()  # waits for the call's last event
    st.sync()
    return s


def frames_and_cap(W, H, n, count=True):
    scene = SceneStream(W, H, device="cuda")
    d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).contiguous()
    torch.cuda.synchronize()
    if not count:  # slots of the detector's list capacity: no counting pass in a trace
        return scene, d_frames, None, None
    sb = ops.SurfBatch(W, H, 8)  # the counts that size the streams' slots
    _, _, counts = sb.detect_device(d_frames, 16, THRESHOLD)
    top = int(counts[:, 0].max().item())
    sb.close()
    return scene, d_frames, top, (top + 255) // 256 * 256 + 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surf_batch_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--groups", default="0,4,16,32", help="surf_group per leg; 0, the baseline, must be among them")
    ap.add_argument("--plain-describe", default="4,16,32",
                    help="groups that also run with describe's plain stride ('' for none)")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--trace-leg", type=int, default=None, help="run this one surf_group only, --runs calls, no file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_surf_batch.py measures on the GPU; none is visible")
    n = a.frames
    if a.trace_leg is not None:
        for size in a.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            scene, d_frames, _, cap = frames_and_cap(W, H, n, count=False)
            st = KnnFrameStream(W, H, scene.K, n, detector="surf", feat_cap=cap, hessian_threshold=THRESHOLD,
                                surf_group=a.trace_leg)
            records = st.new_records(n - 1)
            torch.cuda.synchronize()
            for _ in range(a.runs):
                st.process(d_frames, records, wait_torch=False)
                st.sync()
            st.close()
            print(f"{W}x{H} surf_group {a.trace_leg}: {a.runs} calls of {n} frames")
        return
    groups = [int(g) for g in a.groups.split(",")]
    if 0 not in groups:
        sys.exit("--groups must contain 0, the baseline")
    plain = [int(g) for g in a.plain_describe.split(",") if g]
    # a leg is (surf_group, large windows first); the baseline has no group detector
    keys = [(g, True) for g in groups] + [(g, False) for g in plain if g > 0]
    lines = [f"time_surf_batch: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs}; surf (hessianThreshold {THRESHOLD:g}), one process call on {n} resident frames per run; "
             "legs (surf_group) alternate; stage events of the stream",
             "one machine, one process; detection in ms per frame, the whole call (3 stages) in ms per pair"]
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene, d_frames, top, cap = frames_and_cap(W, H, n)
        legs = {}
        for g, first in keys:
            os.environ["DVO_SURF_LARGE_FIRST"] = "1" if first else "0"  # read when the group's scratch is made
            legs[(g, first)] = KnnFrameStream(W, H, scene.K, n, detector="surf", feat_cap=cap,
                                              hessian_threshold=THRESHOLD, surf_group=g)
        del os.environ["DVO_SURF_LARGE_FIRST"]
        groups = keys  # from here on a "group" is a leg's key
        zero = (0, True)
        records = {g: legs[g].new_records(n - 1) for g in groups}
        torch.cuda.synchronize()
        for g in groups:
            legs[g].set_profiling(True)
            run(legs[g], d_frames, records[g])  # warm-up
        det = {g: [] for g in groups}
        call = {g: [] for g in groups}
        for _ in range(a.runs):
            for g in groups:
                s = run(legs[g], d_frames, records[g])
                det[g].append(s["detect"] / n)
                call[g].append(sum(s.values()) / (n - 1))
        recs = {g: legs[g].records_numpy(records[g], n - 1) for g in groups}
        for g in groups:
            for f in PAIR_RECORD_DTYPE.names:
                assert np.array_equal(recs[g][f], recs[zero][f]), (size, g, f)
        ok = int((recs[zero]["status"] == 0).sum())
        base = det[zero]
        spread = max(base) - min(base)
        bar = min(base) - 3 * spread
        lines.append(f"{W}x{H} surf: features per frame <= {top}, feat_cap {cap}, {ok} of {n - 1} pairs status 0; "
                     "records of every leg equal the baseline's in every field True (asserted)")
        for key in groups:
            g, first = key
            v, c = det[key], call[key]
            mem = ops.SurfBatch.scratch_bytes(W, H, g) / 1e6 if g else 0.0
            name = f"surf_group {g:2d}" + ("" if first else " plain describe")
            line = (f"  {name}  detection runs {' '.join(f'{x:.4f}' for x in v)}  median {np.median(v):.4f}"
                    f"  spread {max(v) - min(v):.4f}  call median {np.median(c):.4f} ms/pair"
                    f"  detection share {100 * np.median(v) * n / (np.median(c) * (n - 1)):.0f} %  scratch {mem:.0f} MB")
            if g:
                line += (f"  baseline / group {np.median(base) / np.median(v):.2f}x; median < baseline best - 3 x "
                         f"baseline spread ({bar:.4f}): {float(np.median(v)) < bar}")
            lines.append(line)
        for g in plain:
            if (g, True) in det and (g, False) in det:
                pl, lf = det[(g, False)], det[(g, True)]
                bar2 = min(pl) - 3 * (max(pl) - min(pl))
                lines.append(f"  large windows first at surf_group {g}: plain / first {np.median(pl) / np.median(lf):.2f}x; first "
                             f"median < plain best - 3 x plain spread ({bar2:.4f}): {float(np.median(lf)) < bar2}")
        for st in legs.values():
            st.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
