"""What the ORB stream's ratio-test matcher costs (dvo_stream_set_ratio_test):
stream.FrameStream.process on device-resident frames with the default cross check (A) against the
same stream shape with ratio=0.75 (B: Hamming 2-NN on the matrix cores, ratio test, gather), at
1280x720 / 2000 features and 640x480 / 500 features, 64 frames per call; and the per-call
dvo_bf_knn_hamming (k = 2), unsplit and with the train stages split over workgroups (partial lists
and a merge), against dvo_bf_match_hamming (cross check off) at 2000 x 2000 and 8192 x 8192.

Method: synthetic frames; one process; the two streams alternate run by run.  A run is one process
call on the resident frames ended by a synchronise (after a warm-up call each), host clock, ms per
call.  The match stage's device time comes from HIP events (dvo_stream_stage_times) in `--runs`
further calls per stream, alternating in the same way.  Mean kept matches and RANSAC iterations per
pair come from the records of the pairs with status 0.  The per-call legs alternate too: a run is
`--calls` calls on host descriptors (upload, kernels, read-back), ms per call.  Every run, the
spread (max - min) and the library's source hash go to `--out`.  Verdict per comparison: different
only if a median lies outside the other leg's best or worst run by 3 x that leg's spread, the margin
of the project's A/B notes.

usage: python tools/time_orb_ratio.py [--out profiles/orb_ratio_time.txt] [--runs 7 --frames 64]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd.stream import FrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402


def call_leg(fs, d_frames, records):
    fs.sync()
    t0 = time.perf_counter()
    fs.process(d_frames, records, wait_torch=False)
    fs.sync()
    return 1e3 * (time.perf_counter() - t0)


def match_leg(fs, d_frames, records):
    fs.set_profiling(True)
    fs.process(d_frames, records, wait_torch=False)
    ms, _ = fs.stage_times()
    fs.set_profiling(False)
    return ms["match"]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_ratio_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=0.75)
    ap.add_argument("--shapes", default="1280x720x2000,640x480x500")
    ap.add_argument("--sets", default="2000,8192", help="descriptor counts of the per-call legs (queries = trains)")
    ap.add_argument("--calls", type=int, default=20, help="calls per run of a per-call leg")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_orb_ratio.py measures on the GPU; none is visible")
    lines = [f"time_orb_ratio: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"runs {a.runs}; stream legs: one process call on {a.frames} resident frames, A cross check (default), "
             f"B ratio={a.ratio}; legs alternate; ms per call",
             "one machine, one process; host clock around call + synchronise; match stage from HIP events"]
    for shape in a.shapes.split(","):
        W, H, NF = (int(v) for v in shape.split("x"))
        scene = SceneStream(W, H, device="cuda")
        d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, a.frames))) for i in range(0, a.frames, 8)])
        d_frames = d_frames.contiguous()
        torch.cuda.synchronize()
        legs = {"A cross check": FrameStream(W, H, scene.K, nfeatures=NF, max_frames=a.frames),
                f"B ratio {a.ratio}": FrameStream(W, H, scene.K, nfeatures=NF, max_frames=a.frames, ratio=a.ratio)}
        recs = {k: fs.new_records(a.frames - 1) for k, fs in legs.items()}
        torch.cuda.synchronize()
        for k, fs in legs.items():
            call_leg(fs, d_frames, recs[k])  # warm-up
        call = {k: [] for k in legs}
        match = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fs in legs.items():
                call[k].append(call_leg(fs, d_frames, recs[k]))
        for _ in range(a.runs):
            for k, fs in legs.items():
                match[k].append(match_leg(fs, d_frames, recs[k]))
        lines.append(f"{W}x{H} nfeatures {NF}, {a.frames - 1} pairs per call")
        for k, fs in legs.items():
            fs.sync()
            r = FrameStream.records_numpy(recs[k], a.frames - 1)
            ok = r["status"] == 0
            lines.append(f"  {k}: {int(ok.sum())} pairs status 0; per pair: mean kept matches {r['n_matches'][ok].mean():.1f}"
                         f"  mean RANSAC iterations {r['ransac_iters'][ok].mean():.1f}"
                         f"  mean hypotheses solved {r['n_hypotheses'][ok].mean():.1f}")
            lines.append(f"    whole call ms   {stats(call[k])}")
            lines.append(f"    match stage ms  {stats(match[k])}")
        ka, kb = list(legs)
        lines.append(f"  B against A (median outside A's runs by 3 x A's spread): whole call {verdict(call[ka], call[kb])}"
                     f" ({np.median(call[kb]) / np.median(call[ka]):.3f}x), match stage {verdict(match[ka], match[kb])}"
                     f" ({np.median(match[kb]) / np.median(match[ka]):.3f}x)")
        for fs in legs.values():
            fs.close()
    rng = np.random.default_rng(1)
    lines.append(f"per call, host descriptors, {a.calls} calls per run, ms per call (upload + kernels + read-back)")
    for n in (int(v) for v in a.sets.split(",")):
        q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        t = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        per = {"bf_match_hamming (no cross check)": lambda: ops.bf_match(q, t, 0),
               "bf_knn_hamming k=2 unsplit": lambda: ops.bf_knn_hamming(q, t, 2, tsplit=1),
               "bf_knn_hamming k=2 split 4 + merge": lambda: ops.bf_knn_hamming(q, t, 2, tsplit=4),
               "bf_knn_hamming k=2 split 16 + merge": lambda: ops.bf_knn_hamming(q, t, 2, tsplit=16),
               "bf_knn_hamming k=2 (the library's choice)": lambda: ops.bf_knn_hamming(q, t, 2)}
        ms = {k: [] for k in per}
        for f in per.values():
            f()
        for _ in range(a.runs):
            for k, f in per.items():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()
                ms[k].append(1e3 * (time.perf_counter() - t0) / a.calls)
        lines.append(f"{n} x {n}")
        for k in per:
            lines.append(f"  {k:42s} {stats(ms[k])}")
        ks = list(per)
        lines.append(f"  against unsplit: split 4 {verdict(ms[ks[1]], ms[ks[2]])}, split 16 {verdict(ms[ks[1]], ms[ks[3]])}; "
                     f"the library's choice against bf_match_hamming: {verdict(ms[ks[0]], ms[ks[4]])}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
