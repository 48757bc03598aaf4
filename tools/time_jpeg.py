"""What JPEG input costs: ops.JpegDecoder alone with device, with split device
(`--split`: one leg per split_bytes, and the restart-per-row files once at the default) and with
host entropy decoding, today's route (Pillow on one core -> colour frames -> FrameStream.submit) on
the same files, and FrameStream.submit_jpeg against submit on the resident mono8 frames.

Frames: `--distinct` frames of the synthetic scene with three different channels, encoded by
Pillow at `--quality`, 4:2:0, once without restart markers and once with one per MCU row, and
repeated to `--batch` frames per call.  Method (bench.py's): one warm-up call, then `--runs` timed
runs with a device synchronise on both sides, on the host clock; the value is the median run
and every run is printed.  Needs Pillow (it makes the files).  Prints one JSON line.

`--decode-only` leaves out the stream comparisons.

usage: python tools/time_jpeg.py [--width 1280 --height 720 --nfeatures 2000 --batch 256 --quality 80]
                                 [--split 32,64,128,256,512] [--decode-only]"""
import argparse
import io
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256, help="frames per call")
    ap.add_argument("--distinct", type=int, default=32, help="different frames among them")
    ap.add_argument("--quality", type=int, default=80)
    ap.add_argument("--group", type=int, default=256, help="the decoder's group_frames")
    ap.add_argument("--steps", type=int, default=2, help="calls per timed run of the stream comparisons")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--split", default="32,64,128,256,512", help="split_bytes of the device_split legs ('' for none)")
    ap.add_argument("--decode-only", action="store_true", help="no stream comparisons")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_jpeg.py measures on the GPU; none is visible")
    from PIL import Image
    W, H, B = a.width, a.height, a.batch
    dev = torch.device("cuda", 0)
    scene = SceneStream(W, H, device=str(dev))
    g = torch.cat([scene.render_batch(range(i, min(i + 8, a.distinct))) for i in range(0, a.distinct, 8)])
    rgb = torch.stack([g, torch.roll(g, 3, dims=2), 255 - g], dim=-1).cpu().numpy()

    def encode(f, **kw):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=a.quality, subsampling=2, **kw)
        return buf.getvalue()
    rep = lambda xs: [xs[i % len(xs)] for i in range(B)]  # noqa: E731
    plain = rep([encode(f) for f in rgb])
    rows = rep([encode(f, restart_marker_rows=1) for f in rgb])

    ctx = Context(0)
    dec = ops.JpegDecoder(W, H, group_frames=a.group, ctx=ctx)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    med = lambda ts: float(np.median(ts))  # noqa: E731

    def timed(fn):
        ts = []
        for r in range(a.runs + 1):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t0)
        return ts

    t_dev = timed(lambda: dec.decode(plain, "gray", "device", out=out, stream=st))
    mono = out.clone()  # the resident mono8 frames of the stream comparison
    t_dev_rows = timed(lambda: dec.decode(rows, "gray", "device", out=out, stream=st))
    same_rows = bool(torch.equal(out, mono))
    t_host = timed(lambda: dec.decode(plain, "gray", "host", out=out, stream=st))
    same_host = bool(torch.equal(out, mono))
    split_res = {}
    same_split = True
    for sb in [int(v) for v in a.split.split(",") if v]:
        dec.split_bytes = sb
        ts = timed(lambda: dec.decode(plain, "gray", "device_split", out=out, stream=st))
        same_split = same_split and bool(torch.equal(out, mono))
        passes, segments, fallbacks = dec.split_info()
        split_res[f"decode_split_{sb}_frames_per_s"] = round(B / med(ts), 1)
        split_res[f"decode_split_{sb}_runs_s"] = [round(t, 5) for t in ts]
        split_res[f"decode_split_{sb}_max_passes"] = passes
        assert fallbacks == 0 and segments > 0
    if a.split:
        dec.split_bytes = ops.JPEG_SPLIT_BYTES_DEFAULT
        ts = timed(lambda: dec.decode(rows, "gray", "device_split", out=out, stream=st))
        same_split = same_split and bool(torch.equal(out, mono))
        split_res["decode_split_default_restart_rows_frames_per_s"] = round(B / med(ts), 1)
        split_res["decode_split_default_restart_rows_runs_s"] = [round(t, 5) for t in ts]
        split_res["split_bytes_default"] = ops.JPEG_SPLIT_BYTES_DEFAULT
        # the legs before, once more after the split ones (the legs alternate in one process)
        ts = timed(lambda: dec.decode(plain, "gray", "device", out=out, stream=st))
        split_res["decode_device_again_frames_per_s"] = round(B / med(ts), 1)
        split_res["decode_device_again_runs_s"] = [round(t, 5) for t in ts]
        ts = timed(lambda: dec.decode(rows, "gray", "device", out=out, stream=st))
        split_res["decode_device_restart_rows_again_frames_per_s"] = round(B / med(ts), 1)
        split_res["decode_device_restart_rows_again_runs_s"] = [round(t, 5) for t in ts]
        split_res["split_decodes_equal"] = same_split
    if a.decode_only:
        dec.close()
        print(json.dumps({
            "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "width": W, "height": H,
            "batch": B, "distinct": a.distinct, "quality": a.quality, "sampling": "4:2:0", "group_frames": a.group,
            "runs": a.runs, "jpeg_bytes_per_frame": round(float(np.mean([len(b) for b in plain])), 1),
            "decode_device_frames_per_s": round(B / med(t_dev), 1), "decode_device_runs_s": [round(t, 5) for t in t_dev],
            "decode_device_restart_rows_frames_per_s": round(B / med(t_dev_rows), 1),
            "decode_device_restart_rows_runs_s": [round(t, 5) for t in t_dev_rows],
            "decode_host_frames_per_s": round(B / med(t_host), 1), "decode_host_runs_s": [round(t, 5) for t in t_host],
            "decodes_equal": same_rows and same_host, **split_res,
            "note": "one machine, one run; host clock around work that ends in a device synchronise"}))
        return

    fs = FrameStream(W, H, scene.K, nfeatures=a.nfeatures, max_frames=B, ctx=ctx)
    depth = FrameStream.pipeline_depth()
    recs = [fs.new_records(B - 1) for _ in range(depth + 1)]
    torch.cuda.synchronize()
    count = [0]

    def next_rec():
        count[0] += 1
        return recs[count[0] % len(recs)]

    def pil_route():
        for _ in range(a.steps):
            col = np.stack([np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1] for b in plain])
            fs.submit(torch.from_numpy(col).to(dev), next_rec())
        fs.sync()

    def jpeg_route():
        for _ in range(a.steps):
            fs.submit_jpeg(plain, next_rec())
        fs.sync()

    def mono_route():
        for _ in range(a.steps):
            fs.submit(mono, next_rec(), wait_torch=False)
        fs.sync()

    for _ in range(depth):  # fill the pipeline
        fs.submit(mono, next_rec(), wait_torch=False)
    fs.sync()
    t_mono = timed(mono_route)
    t_jpeg = timed(jpeg_route)
    t_pil = timed(pil_route)
    fs.drain()
    r_mono = fs.process(mono)
    fs.sync()
    r_mono = r_mono.clone()
    r_jpeg = fs.process_jpeg(plain)
    fs.sync()
    same_rec = bool(torch.equal(r_mono, r_jpeg))
    fs.close()
    dec.close()

    fps = lambda ts, frames: round(frames / med(ts), 1)  # noqa: E731
    r5 = lambda ts: [round(t, 5) for t in ts]  # noqa: E731
    res = {
        "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0),
        "width": W, "height": H, "nfeatures": a.nfeatures, "batch": B, "distinct": a.distinct, "quality": a.quality,
        "sampling": "4:2:0", "group_frames": a.group, "runs": a.runs, "steps": a.steps, "streams": 1,
        "jpeg_bytes_per_frame": round(float(np.mean([len(b) for b in plain])), 1),
        "jpeg_bytes_per_frame_restart_rows": round(float(np.mean([len(b) for b in rows])), 1),
        "decode_device_frames_per_s": fps(t_dev, B), "decode_device_runs_s": r5(t_dev),
        "decode_device_restart_rows_frames_per_s": fps(t_dev_rows, B), "decode_device_restart_rows_runs_s": r5(t_dev_rows),
        "decode_host_frames_per_s": fps(t_host, B), "decode_host_runs_s": r5(t_host),
        "decodes_equal": same_rows and same_host,
        "submit_mono_frames_per_s": fps(t_mono, B * a.steps), "submit_mono_runs_s": r5(t_mono),
        "submit_jpeg_frames_per_s": fps(t_jpeg, B * a.steps), "submit_jpeg_runs_s": r5(t_jpeg),
        "pil_then_submit_frames_per_s": fps(t_pil, B * a.steps), "pil_then_submit_runs_s": r5(t_pil),
        "records_equal": same_rec, **split_res,
        "note": "one machine, one run; host clock around work that ends in a device synchronise",
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
