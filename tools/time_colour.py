"""What colour input costs: FrameStream.submit on resident colour frames
against the same stream on the equivalent resident mono8 frames, in one process, and
ops.bgr2gray_device alone.

Method (bench.py's): warm-up submits that fill the pipeline, then `--runs` timed runs of
exactly `--steps` submits each with a device synchronise on both sides, the two inputs
alternating run by run; the value is the median run.  The conversion kernel is timed the
same way over `--kernel-iters` launches per run; its bytes are (C + 1) w h per frame
(C read, 1 written), its roof 8 TB/s.  Prints one JSON line.

usage: python tools/time_colour.py [--width 1280 --height 720 --nfeatures 2000 --batch 256 --channels 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd._native import Context  # noqa: E402
from droplet_visual_odometry_amd.stream import FrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

HBM_ROOF = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256, help="pairs per submit (batch + 1 frames)")
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=0, help="warm-up submits (at least the pipeline depth)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_colour.py measures on the GPU; none is visible")
    W, H, B, C = a.width, a.height, a.batch, a.channels
    dev = torch.device("cuda", 0)
    scene = SceneStream(W, H, device=str(dev))
    gray_src = torch.cat([scene.render_batch(range(i, min(i + 8, B + 1))) for i in range(0, B + 1, 8)])
    ch = [gray_src, torch.roll(gray_src, 3, dims=2), 255 - gray_src]  # three different channels
    if C == 4:
        ch.append(torch.full_like(gray_src, 255))
    colour = torch.stack(ch, dim=-1).contiguous()
    mono = torch.empty_like(gray_src)
    ctx = Context(0)
    ops.bgr2gray_device(colour, mono, ctx=ctx)  # the equivalent mono8 frames
    torch.cuda.synchronize()

    fs = FrameStream(W, H, scene.K, nfeatures=a.nfeatures, max_frames=B + 1, ctx=ctx)
    depth = FrameStream.pipeline_depth()
    recs = [fs.new_records(B) for _ in range(depth + 1)]
    torch.cuda.synchronize()
    count = [0]

    def run(frames, steps):
        fs.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fs.submit(frames, recs[count[0] % len(recs)], wait_torch=False)
            count[0] += 1
        fs.sync()
        return time.perf_counter() - t0

    warm = max(a.warmup, depth)
    run(mono, warm)
    run(colour, warm)
    t_mono, t_col = [], []
    for _ in range(a.runs):
        t_mono.append(run(mono, a.steps))
        t_col.append(run(colour, a.steps))
    fs.drain()
    fs.sync()
    r_mono = fs.process(mono)
    fs.sync()
    r_mono = r_mono.clone()
    r_col = fs.process(colour)
    fs.sync()
    same = bool(torch.equal(r_mono, r_col))  # the same frames either way: the same records

    st = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty_like(mono)
    t_k = []
    for r in range(a.runs + 1):  # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.kernel_iters):
            ops.bgr2gray_device(colour, out, stream=st, ctx=ctx)
        torch.cuda.synchronize()
        if r:
            t_k.append((time.perf_counter() - t0) / a.kernel_iters)
    fs.close()
    frames_per_run = B * a.steps  # as bench.py counts: one frame per pair
    med = lambda ts: float(np.median(ts))  # noqa: E731
    k_bytes = (C + 1) * W * H * (B + 1)
    res = {
        "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "width": W, "height": H, "nfeatures": a.nfeatures, "batch": B, "channels": C, "steps": a.steps,
        "runs": a.runs, "streams": 1,
        "mono_frames_per_s": round(frames_per_run / med(t_mono), 1),
        "colour_frames_per_s": round(frames_per_run / med(t_col), 1),
        "mono_runs_s": [round(t, 5) for t in t_mono], "colour_runs_s": [round(t, 5) for t in t_col],
        "colour_over_mono_time": round(med(t_col) / med(t_mono), 4),
        "records_equal": same,
        "bgr2gray_us_per_frame": round(1e6 * med(t_k) / (B + 1), 3),
        "bgr2gray_bytes_per_s": round(k_bytes / med(t_k), 1),
        "bgr2gray_fraction_of_8TBs": round(k_bytes / med(t_k) / HBM_ROOF, 4),
        "note": "one machine, one run; host clock around work that ends in a device synchronise",
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
