"""What a track-PnP binding costs the ORB stream (dvo_stream_set_track_pnp).

One process: stream.FrameStream.process on device-resident frames with a Landmarks and a Tracks
bound before every call (A) against the same stream shape with a TrackPnP bound too (B: after the
track kernels the correspondence kernel and the PnP kernel, 128 hypotheses, 10 polish steps, a mask
of the stream's feature count), at the benchmark's headline shape 1280x720 / 2000 features and at
320x240 / 300 features, 64 frames per call.  Two streams of one shape alternate run by run.  A run
is one process call on the resident frames ended by a synchronise (after a warm-up call each), host
clock, ms per call, the bindings inside the timed span.  The device time of the recoverPose +
records stage (which the landmark, track and PnP kernels fall into) comes from HIP events
(dvo_stream_stage_times) in `--runs` further calls per stream, alternating in the same way; the
match stage is reported as a control.  A third stream of the shape that binds nothing runs once:
its records must be A's and B's byte for byte.

Verdict per comparison: different only if a median lies outside the other leg's best or worst run
by 3 x that leg's spread, the margin of the project's A/B notes.  The binding is opt-in, so its
cost is reported, not gated.  Not measured here: the k-NN stream, batches of thousands of pairs,
and other hypothesis counts.  Everything goes to `--out`.

usage: python tools/time_track_pnp.py [--out profiles/track_pnp_time.txt] [--runs 7 --frames 64] [--commit ID]"""
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
from droplet_visual_odometry_amd.stream import FrameStream, Landmarks, TrackPnP, Tracks  # noqa: E402
from time_tracks import frames_of, stats, verdict  # noqa: E402


def bind(fs, lm, tr, pn):
    fs.bind_landmarks(lm)
    fs.bind_tracks(tr)
    if pn is not None:
        fs.bind_pnp(pn)


def call_leg(fs, d_frames, records, lm, tr, pn):
    fs.sync()
    t0 = time.perf_counter()
    bind(fs, lm, tr, pn)
    fs.process(d_frames, records, wait_torch=False)
    fs.sync()
    return 1e3 * (time.perf_counter() - t0)


def stage_leg(fs, d_frames, records, lm, tr, pn):
    fs.set_profiling(True)
    bind(fs, lm, tr, pn)
    fs.process(d_frames, records, wait_torch=False)
    ms, _ = fs.stage_times()
    fs.set_profiling(False)
    return ms["recover_pose"], ms["match"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_pnp_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", default="1280x720x2000,320x240x300")
    ap.add_argument("--commit", default="", help="the commit the measured tree stands on (goes into the header)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_track_pnp.py measures on the GPU; none is visible")
    lines = [f"time_track_pnp: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}"
             + (f" on top of commit {a.commit}" if a.commit else ""),
             f"runs {a.runs}; one process call on {a.frames} resident frames, A a Landmarks and a Tracks bound before each "
             "call, B a TrackPnP too (128 hypotheses, 10 steps, Huber 1 px, inliers 2 px, min_points 6, a mask); "
             "legs alternate; ms per call",
             "one machine, one process; host clock around bind + call + synchronise; "
             "recoverPose + records stage and match stage from HIP events",
             "not measured: the k-NN stream, batches of thousands of pairs, other hypothesis counts"]
    for shape in a.shapes.split(","):
        W, H, NF, K, d_frames = frames_of(shape, a.frames)
        pairs = a.frames - 1
        names = ("A landmarks + tracks", "B landmarks + tracks + pnp")
        legs = {k: FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames) for k in names}
        lms = {k: Landmarks(pairs, NF, "cuda") for k in names}
        trs = {k: Tracks(pairs, NF, "cuda") for k in names}
        pns = {names[0]: None, names[1]: TrackPnP(pairs, "cuda", mask_cap=NF)}
        recs = {k: fs.new_records(pairs) for k, fs in legs.items()}
        torch.cuda.synchronize()
        for k, fs in legs.items():
            call_leg(fs, d_frames, recs[k], lms[k], trs[k], pns[k])  # warm-up (the scratch is allocated here)
        call = {k: [] for k in legs}
        pose = {k: [] for k in legs}
        match = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fs in legs.items():
                call[k].append(call_leg(fs, d_frames, recs[k], lms[k], trs[k], pns[k]))
        for _ in range(a.runs):
            for k, fs in legs.items():
                p, m = stage_leg(fs, d_frames, recs[k], lms[k], trs[k], pns[k])
                pose[k].append(p)
                match[k].append(m)
        lines.append(f"{W}x{H} nfeatures {NF}, {pairs} pairs per call, cap {NF} landmarks per pair")
        for k, fs in legs.items():
            fs.sync()
            r = FrameStream.records_numpy(recs[k], pairs)
            ok = r["status"] == 0
            sc = trs[k].scales_numpy()
            extra = ""
            if pns[k] is not None:
                po = pns[k].numpy()
                fit = po["status"] == 0
                both = fit & (sc["ratio"] > 0)  # a ratio to compare the scale with
                extra = (f"; pnp: {int(fit.sum())} status 0, {int((po['status'] == 3).sum())} without a model, "
                         f"mean n_corr {po['n_corr'][1:].mean():.1f}, mean n_best {po['n_best'][fit].mean():.1f}, "
                         f"mean inliers {po['n_inliers'][fit].mean():.1f}, mean rms {po['rms'][fit].mean():.3f} px, "
                         f"median |scale / ratio - 1| {np.median(np.abs(po['scale'][both] / sc['ratio'][both] - 1)):.3f}")
            lines.append(f"  {k}: {int(ok.sum())} pairs status 0; mean n_common {sc['n_common'][1:].mean():.1f} "
                         f"(min {int(sc['n_common'][1:].min())}, max {int(sc['n_common'][1:].max())}){extra}")
            lines.append(f"    whole call ms                  {stats(call[k])}")
            lines.append(f"    recoverPose + records stage ms {stats(pose[k])}")
            lines.append(f"    match stage ms                 {stats(match[k])}")
        ka, kb = names
        plain = FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames)
        rec0 = plain.process(d_frames, wait_torch=False)
        plain.sync()
        r0 = FrameStream.records_numpy(rec0, pairs).tobytes()
        plain.close()

        def raw(t):
            return t.cpu().numpy().tobytes()

        same = (raw(lms[ka].entries) == raw(lms[kb].entries) and raw(lms[ka].counts) == raw(lms[kb].counts)
                and raw(trs[ka].links) == raw(trs[kb].links) and raw(trs[ka].scales) == raw(trs[kb].scales))
        lines.append(f"  landmarks, links and scales of A and B byte-equal: {same}; records of A, of B and of a stream that "
                     f"binds nothing byte-equal: "
                     f"{FrameStream.records_numpy(recs[ka], pairs).tobytes() == FrameStream.records_numpy(recs[kb], pairs).tobytes() == r0}")
        lines.append(f"  B against A (median outside A's runs by 3 x A's spread): whole call {verdict(call[ka], call[kb])}"
                     f" ({np.median(call[kb]) / np.median(call[ka]):.3f}x, {np.median(call[kb]) - np.median(call[ka]):+.3f} ms),"
                     f" recoverPose + records stage {verdict(pose[ka], pose[kb])}"
                     f" ({np.median(pose[kb]) - np.median(pose[ka]):+.3f} ms),"
                     f" match stage {verdict(match[ka], match[kb])} ({np.median(match[kb]) - np.median(match[ka]):+.3f} ms)")
        for fs in legs.values():
            fs.close()
        del legs, lms, trs, pns, recs, d_frames
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
