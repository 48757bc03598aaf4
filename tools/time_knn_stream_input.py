"""What raw input costs in the batched k-NN stream ("Raw input for the k-NN stream"):
one stream.KnnFrameStream call on colour, colour + undistort or JPEG + undistort frames (leg B)
against the operator-by-operator path into a caller-owned gray batch followed by the mono
process() (leg A: ops.bgr2gray_device, ops.Undistorter.apply, or ops.JpegDecoder.decode and
Undistorter.apply), in modes knn_sift and surf with group detection at 640x480 and 1280x720, 32 and
128 frames per call.

Method: synthetic frames with three different channels, JPEG-encoded on the host by Pillow (quality
90, 4:2:0) for the JPEG form; the camera is the scene's with the rosbot distortion, and the streams
of the undistorting forms run with the new camera matrix.  Per size, mode, form and batch the two
legs alternate run by run in one process; a run is the leg's calls on resident input ended by a
synchronise (after one warm-up run); host clock, ms per pair; the value is the median of `--runs`
runs.  Both legs' records must agree in every field before anything is timed.  The input stage's
share comes from HIP events in one extra call: the first stage figure of leg B (input + detection)
against that of a mono call on leg A's gray batch.  Every run, the spread (max - min), the slab
bytes and the library's source hash go to `--out`.  Verdict per row (DESIGN.md §1's rule): B is
faster only if its median is below A's best run minus 3 x A's spread, and not slower if it is
below A's worst run plus 3 x A's spread.

usage: python tools/time_knn_stream_input.py [--out profiles/knn_stream_input_time.txt] [--runs 5]"""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd._native import DVO_ECAP, PAIR_RECORD_DTYPE  # noqa: E402
from droplet_visual_odometry_amd.stream import KnnFrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

MODES = {"knn_sift": ("sift", "detect_group"), "surf": ("surf", "surf_group")}
FORMS = ("colour", "colour+undistort", "jpeg+undistort")
DIST = np.array([0.142541, -0.248887, -0.005254, -0.005417, 0.0])


def encode(rgb):
    from PIL import Image
    blobs = []
    for f in rgb:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    return blobs


def timed(st, call):
    st.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    st.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_stream_input_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", default="32,128")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--group", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_knn_stream_input.py measures on the GPU; none is visible")
    batches = [int(b) for b in a.batches.split(",")]
    F = max(batches)
    lines = [f"time_knn_stream_input: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs}; leg A: the operators into a caller-owned gray batch, then process(gray); leg B: the one "
             f"call; group detection {a.group}; legs alternate; ms per pair",
             "one machine, one process; host clock around call(s) + synchronise; records of both legs equal before timing"]
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = SceneStream(W, H, device="cuda")
        mono = torch.cat([scene.render_batch(range(i, min(i + 8, F))) for i in range(0, F, 8)]).contiguous()
        bgr = torch.stack([mono, torch.roll(mono, 3, dims=2), 255 - mono], -1).contiguous()
        blobs = encode(np.ascontiguousarray(bgr.cpu().numpy()[..., ::-1]))
        K = np.asarray(scene.K, np.float64)
        newK = ops.get_optimal_new_camera_matrix(K, DIST, (W, H), alpha=1.0)
        u = ops.Undistorter(K, DIST, newK, W, H)
        dec = ops.JpegDecoder(W, H, group_frames=min(F, ops.JpegDecoder.default_group_frames(W, H)))
        gray = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
        gray0 = torch.empty_like(gray)
        slab = ops.knn_stream_raw_input_bytes(W, H, F)
        jpeg_mb = sum(len(b) for b in blobs) / F / 1e6
        lines.append(f"{W}x{H}: slab {slab} bytes for {F} frames ({slab / F:.0f} per frame); JPEG files {jpeg_mb:.3f} MB each")

        def operators(form, n):
            """Leg A's input stage: `gray[:n]` on torch's stream."""
            if form == "colour":
                ops.bgr2gray_device(bgr[:n], gray[:n])
            elif form == "colour+undistort":
                u.apply(bgr[:n], gray[:n])
            else:
                dec.decode(blobs[:n], "gray", out=gray0[:n])
                u.apply(gray0[:n], gray[:n])

        for mode in a.modes.split(","):
            det, group_kw = MODES[mode]
            for form in FORMS:
                Ks = K if form == "colour" else newK
                und = None if form == "colour" else u
                # the counts that size the frame slots: one mono call on leg A's gray batch
                operators(form, F)
                room = 8192 if det == "sift" else min(8192, max(4096, W * H // 64))  # SURF: within its list capacity
                probe = KnnFrameStream(W, H, Ks, F, detector=det, feat_cap=room, **{group_kw: a.group})
                rec = probe.process(gray)
                probe.sync()
                r = probe.records_numpy(rec, F - 1)
                probe.close()
                assert not (r["status"] == DVO_ECAP).any(), "a frame has more features than the probe stream keeps"
                top = int(max(r["n_kp_prev"].max(), r["n_kp_cur"].max()))
                cap = (top + 255) // 256 * 256 + 256
                sa = KnnFrameStream(W, H, Ks, F, detector=det, feat_cap=cap, **{group_kw: a.group})
                sb = KnnFrameStream(W, H, Ks, F, detector=det, feat_cap=cap, raw_input=True, **{group_kw: a.group})
                for n in batches:
                    ra, rb = sa.new_records(n - 1), sb.new_records(n - 1)
                    torch.cuda.synchronize()

                    def leg_a():
                        operators(form, n)
                        sa.process(gray[:n], ra)

                    def leg_b():
                        if form == "jpeg+undistort":
                            sb.process_jpeg(blobs[:n], rb, undistort=und)
                        else:
                            sb.process(bgr[:n], rb, wait_torch=False, undistort=und)

                    timed(sa, leg_a)  # warm-up
                    timed(sb, leg_b)
                    na, nb = sa.records_numpy(ra, n - 1), sb.records_numpy(rb, n - 1)
                    assert na.tobytes() == nb.tobytes(), f"{W}x{H} {mode} {form} {n}: the legs' records differ"
                    assert not (na["status"] == DVO_ECAP).any()
                    ok = int((na["status"] == 0).sum())
                    ta, tb = [], []
                    for _ in range(a.runs):
                        ta.append(1e3 * timed(sa, leg_a) / (n - 1))
                        tb.append(1e3 * timed(sb, leg_b) / (n - 1))
                    for st in (sa, sb):
                        st.set_profiling(True)
                    leg_a()
                    pa = sa.stage_times()
                    leg_b()
                    pb = sb.stage_times()
                    for st in (sa, sb):
                        st.set_profiling(False)
                    tot = sum(pb.values())
                    spread = max(ta) - min(ta)
                    ma, mb = float(np.median(ta)), float(np.median(tb))
                    lines.append(f"{W}x{H} {mode} {form} {n} frames: feat_cap {cap}, {ok} of {n - 1} pairs status 0")
                    lines.append(f"  A operators + process runs {' '.join(f'{v:.3f}' for v in ta)}  median {ma:.3f}"
                                 f"  spread {spread:.3f}")
                    lines.append(f"  B one call            runs {' '.join(f'{v:.3f}' for v in tb)}  median {mb:.3f}"
                                 f"  spread {max(tb) - min(tb):.3f}  A / B {ma / mb:.3f}x; faster (median < A best - 3 x A "
                                 f"spread = {min(ta) - 3 * spread:.3f}): {mb < min(ta) - 3 * spread}; not slower (median <= A "
                                 f"worst + 3 x A spread = {max(ta) + 3 * spread:.3f}): {mb <= max(ta) + 3 * spread}")
                    lines.append(f"    B, one call, device ms: input + detection {pb['detect']:.3f}  matching + ratio "
                                 f"{pb['match']:.3f}  geometry {pb['geometry']:.3f}; mono detection {pa['detect']:.3f}: "
                                 f"input stage {pb['detect'] - pa['detect']:.3f} ms = "
                                 f"{100 * (pb['detect'] - pa['detect']) / tot:.1f} % of the call")
                sa.close()
                sb.close()
        u.close()
        dec.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
