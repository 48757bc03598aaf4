"""What the group SIFT detector buys the batched k-NN stream ("Group SIFT
detection"): stream.KnnFrameStream.process on `--frames` device-resident frames in mode knn_sift with
detect_group 0 (frame by frame: the baseline) against detect_group 4, 16 and 32, at 640x480 and
1280x720.

Method: synthetic frames; per size one stream per leg on one context, in one process; the legs
alternate run by run, after one warm-up call each; a run is one process call ended by a
synchronise.  Detection time is the stream's own stage events (dvo_knn_stream_stage_times), in ms
per frame; the whole call is the sum of the three stages, in ms per pair.  The value is the median
of `--runs` runs, the spread max - min.  The records of every leg must equal the baseline's in every
field.  Verdict per group leg: faster only if its median is below the baseline's best run minus 3 x
the baseline's spread, the margin of the project's A/B notes.  Every run and the library's source
hash go to `--out`.  `--two-pass G,...` adds legs whose group detector blurs in two passes through
global memory (DVO_SIFT_FUSED_BLUR=0 while their stream is made) beside the default, the row and
column pass fused through LDS: the A/B of the fused blur, same process, same rule, against the
two-pass leg of the same group.

usage: python tools/time_sift_batch.py [--out profiles/sift_batch_time.txt] [--runs 5 --frames 128]"""
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


def run(st, d_frames, records):
    """One profiled call: the stage times (device ms)."""
    st.process(d_frames, records, wait_torch=False)
    s = st.stage_times()  # waits for the call's last event
    st.sync()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_batch_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--groups", default="0,4,16,32", help="detect_group per leg; 0, the baseline, must be among them")
    ap.add_argument("--two-pass", default="4,16,32", help="groups that also run with the two-pass blur ('' for none)")
    ap.add_argument("--sizes", default="640x480,1280x720")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sift_batch.py measures on the GPU; none is visible")
    groups = [int(g) for g in a.groups.split(",")]
    if 0 not in groups:
        sys.exit("--groups must contain 0, the baseline")
    two_pass = [int(g) for g in a.two_pass.split(",") if g]
    # a leg is (detect_group, fused blur); the baseline has no group detector
    keys = [(g, True) for g in groups] + [(g, False) for g in two_pass if g > 0]
    n = a.frames
    lines = [f"time_sift_batch: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs}; knn_sift, one process call on {n} resident frames per run; legs (detect_group) alternate; "
             "stage events of the stream",
             "one machine, one process; detection in ms per frame, the whole call (3 stages) in ms per pair"]
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = SceneStream(W, H, device="cuda")
        d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).contiguous()
        torch.cuda.synchronize()
        sb = ops.SiftBatch(W, H, 8)  # the counts that size the streams' slots
        _, _, counts = sb.detect_device(d_frames, 16)
        top = int(counts[:, 0].max().item())
        sb.close()
        cap = (top + 255) // 256 * 256 + 256
        legs = {}
        for g, fused in keys:
            os.environ["DVO_SIFT_FUSED_BLUR"] = "1" if fused else "0"  # read when the group's scratch is made
            legs[(g, fused)] = KnnFrameStream(W, H, scene.K, n, detector="sift", feat_cap=cap, detect_group=g)
        del os.environ["DVO_SIFT_FUSED_BLUR"]
        groups = keys  # from here on a "group" is a leg's key
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
        zero = (0, True)
        same = all(np.array_equal(recs[g][f], recs[zero][f]) for g in groups for f in PAIR_RECORD_DTYPE.names)
        ok = int((recs[zero]["status"] == 0).sum())
        base = det[zero]
        spread = max(base) - min(base)
        bar = min(base) - 3 * spread
        lines.append(f"{W}x{H} knn_sift: features per frame <= {top}, feat_cap {cap}, {ok} of {n - 1} pairs status 0; "
                     f"records of every leg equal the baseline's in every field {same}")
        for key in groups:
            g, fused = key
            v, c = det[key], call[key]
            mem = ops.SiftBatch.scratch_bytes(W, H, g) / 1e6 if g else 0.0
            name = f"detect_group {g:2d}" + ("" if fused else " two-pass blur")
            line = (f"  {name}  detection runs {' '.join(f'{x:.4f}' for x in v)}  median {np.median(v):.4f}"
                    f"  spread {max(v) - min(v):.4f}  call median {np.median(c):.4f} ms/pair"
                    f"  detection share {100 * np.median(v) * n / (np.median(c) * (n - 1)):.0f} %  scratch {mem:.0f} MB")
            if g:
                line += (f"  baseline / group {np.median(base) / np.median(v):.2f}x; median < baseline best - 3 x "
                         f"baseline spread ({bar:.4f}): {float(np.median(v)) < bar}")
            lines.append(line)
        for g in two_pass:
            if (g, True) in det and (g, False) in det:
                two, fus = det[(g, False)], det[(g, True)]
                bar2 = min(two) - 3 * (max(two) - min(two))
                lines.append(f"  fused blur at detect_group {g}: two-pass / fused {np.median(two) / np.median(fus):.2f}x; fused "
                             f"median < two-pass best - 3 x two-pass spread ({bar2:.4f}): {float(np.median(fus)) < bar2}")
        for st in legs.values():
            st.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
