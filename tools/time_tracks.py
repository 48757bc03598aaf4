"""What a tracks binding costs the ORB stream, and whether the unbound path moved (DESIGN.md,
dvo_stream_set_tracks).

Part 1, one process: stream.FrameStream.process on device-resident frames with a Landmarks bound
before every call (A) against the same stream shape with a Landmarks and a Tracks bound (B: the
index copy after matching, then the table, link and select kernels after the landmark kernels),
at the benchmark's headline shape 1280x720 / 2000 features and at 320x240 / 300 features, 64 frames
per call.  Two streams of one shape alternate run by run.  A run is one process call on the
resident frames ended by a synchronise (after a warm-up call each), host clock, ms per call, the
bindings inside the timed span.  The device time of the recoverPose + records stage (which the
landmark and track kernels fall into) comes from HIP events (dvo_stream_stage_times) in `--runs`
further calls per stream, alternating in the same way.  The index copy is queued between the
match stage's and the RANSAC stage's events and so shows in the whole call alone; the match stage
is reported as a control.

Part 2, a fresh child process per leg (`--ab-lib`): the unbound path (no binding at all) of this
library against another build of the library, normally the parent commit's, loaded through
DVO_LIB_PATH, alternating this / other for `--rounds` rounds as tools/ab_libs.sh does.  A child
times `--runs` process calls at the first shape and reports their median.  The unbound difference
(median of the legs' medians) must stay inside the same-library spread of the session: the larger
of the two libraries' max - min over their rounds.

Verdict per comparison of part 1: different only if a median lies outside the other leg's best or
worst run by 3 x that leg's spread, the margin of the project's A/B notes.  Everything goes to `--out`.

usage: python tools/time_tracks.py [--out profiles/tracks_time.txt] [--runs 7 --frames 64]
                                   [--ab-lib PATH --ab-name parent --rounds 3] [--commit ID]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build  # noqa: E402
from droplet_visual_odometry_amd.stream import FrameStream, Landmarks  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402


def bind(fs, lm, tr):
    if lm is not None:
        fs.bind_landmarks(lm)
    if tr is not None:
        fs.bind_tracks(tr)


def call_leg(fs, d_frames, records, lm, tr):
    fs.sync()
    t0 = time.perf_counter()
    bind(fs, lm, tr)
    fs.process(d_frames, records, wait_torch=False)
    fs.sync()
    return 1e3 * (time.perf_counter() - t0)


def stage_leg(fs, d_frames, records, lm, tr):
    fs.set_profiling(True)
    bind(fs, lm, tr)
    fs.process(d_frames, records, wait_torch=False)
    ms, _ = fs.stage_times()
    fs.set_profiling(False)
    return ms["recover_pose"], ms["match"]


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


def frames_of(shape, n):
    W, H, NF = (int(v) for v in shape.split("x"))
    scene = SceneStream(W, H, device="cuda")
    d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).contiguous()
    torch.cuda.synchronize()
    return W, H, NF, scene.K, d_frames


def child(a):
    """One leg of part 2: the unbound path of whatever library DVO_LIB_PATH names; prints the median."""
    W, H, NF, K, d_frames = frames_of(a.shapes.split(",")[0], a.frames)
    fs = FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames)
    rec = fs.new_records(a.frames - 1)
    torch.cuda.synchronize()
    call_leg(fs, d_frames, rec, None, None)
    v = [call_leg(fs, d_frames, rec, None, None) for _ in range(a.runs)]
    fs.close()
    print(f"UNBOUND {np.median(v):.4f} {min(v):.4f} {max(v):.4f}")


def unbound_ab(a, lines):
    legs = {"this": "", a.ab_name: os.path.abspath(a.ab_lib)}
    med = {k: [] for k in legs}
    lines.append(f"unbound path (no binding), {a.shapes.split(',')[0]}, {a.frames} frames per call: this library against "
                 f"{a.ab_name} (build id {build.library_build_id(legs[a.ab_name])}), a fresh process per leg, alternating, "
                 f"{a.rounds} rounds; median (min max) of {a.runs} calls, ms per call")
    for rnd in range(a.rounds):
        for k, path in legs.items():
            env = dict(os.environ)
            env.pop("DVO_LIB_PATH", None)
            if path:
                env["DVO_LIB_PATH"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(a.runs), "--frames",
                                str(a.frames), "--shapes", a.shapes], env=env, capture_output=True, text=True, timeout=300)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("UNBOUND ")]
            if r.returncode != 0 or not got:
                sys.exit(f"the {k} leg failed (exit {r.returncode}):\n{r.stdout}\n{r.stderr}")
            m, lo, hi = (float(x) for x in got[0].split()[1:])
            med[k].append(m)
            lines.append(f"  round {rnd + 1} {k}: {m:.3f} ({lo:.3f} {hi:.3f})")
    spread = {k: max(v) - min(v) for k, v in med.items()}
    diff = float(np.median(med["this"]) - np.median(med[a.ab_name]))
    inside = abs(diff) <= max(spread.values())
    lines.append(f"  this - {a.ab_name}: {diff:+.3f} ms ({100 * diff / np.median(med[a.ab_name]):+.2f} %); same-library spread "
                 + ", ".join(f"{k} {s:.3f}" for k, s in spread.items())
                 + f": the difference is {'inside' if inside else 'OUTSIDE'} it")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_time.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--shapes", default="1280x720x2000,320x240x300")
    ap.add_argument("--ab-lib", default="", help="another build of the library for the unbound comparison")
    ap.add_argument("--ab-name", default="parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--commit", default="", help="the commit the measured tree stands on (goes into the header)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tracks.py measures on the GPU; none is visible")
    if a.child:
        return child(a)
    from droplet_visual_odometry_amd.stream import Tracks
    lines = [f"time_tracks: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}"
             + (f" on top of commit {a.commit}" if a.commit else ""),
             f"runs {a.runs}; one process call on {a.frames} resident frames, A a Landmarks bound before each call, "
             "B a Landmarks and a Tracks; legs alternate; ms per call",
             "one machine, one process; host clock around bind + call + synchronise; "
             "recoverPose + records stage and match stage from HIP events"]
    for shape in a.shapes.split(","):
        W, H, NF, K, d_frames = frames_of(shape, a.frames)
        pairs = a.frames - 1
        names = ("A landmarks", "B landmarks + tracks")
        legs = {k: FrameStream(W, H, K, nfeatures=NF, max_frames=a.frames) for k in names}
        lms = {k: Landmarks(pairs, NF, "cuda") for k in names}
        trs = {names[0]: None, names[1]: Tracks(pairs, NF, "cuda")}
        recs = {k: fs.new_records(pairs) for k, fs in legs.items()}
        torch.cuda.synchronize()
        for k, fs in legs.items():
            call_leg(fs, d_frames, recs[k], lms[k], trs[k])  # warm-up (the scratch is allocated here)
        call = {k: [] for k in legs}
        pose = {k: [] for k in legs}
        match = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, fs in legs.items():
                call[k].append(call_leg(fs, d_frames, recs[k], lms[k], trs[k]))
        for _ in range(a.runs):
            for k, fs in legs.items():
                p, m = stage_leg(fs, d_frames, recs[k], lms[k], trs[k])
                pose[k].append(p)
                match[k].append(m)
        lines.append(f"{W}x{H} nfeatures {NF}, {pairs} pairs per call, cap {NF} landmarks per pair")
        for k, fs in legs.items():
            fs.sync()
            r = FrameStream.records_numpy(recs[k], pairs)
            ok = r["status"] == 0
            c = lms[k].counts.cpu().numpy()
            extra = ""
            if trs[k] is not None:
                sc = trs[k].scales_numpy()
                extra = f", mean n_common {sc['n_common'][1:].mean():.1f} (min {int(sc['n_common'][1:].min())})"
            lines.append(f"  {k}: {int(ok.sum())} pairs status 0; per pair: mean matches {r['n_matches'][ok].mean():.1f}, "
                         f"mean landmarks {c[ok].mean():.1f}{extra}")
            lines.append(f"    whole call ms                  {stats(call[k])}")
            lines.append(f"    recoverPose + records stage ms {stats(pose[k])}")
            lines.append(f"    match stage ms                 {stats(match[k])}")
        ka, kb = names
        same = (FrameStream.records_numpy(recs[ka], pairs).tobytes() == FrameStream.records_numpy(recs[kb], pairs).tobytes()
                and lms[ka].entries.cpu().numpy().tobytes() == lms[kb].entries.cpu().numpy().tobytes())
        lines.append(f"  records and landmarks of A and B byte-equal: {same}")
        lines.append(f"  B against A (median outside A's runs by 3 x A's spread): whole call {verdict(call[ka], call[kb])}"
                     f" ({np.median(call[kb]) / np.median(call[ka]):.3f}x, {np.median(call[kb]) - np.median(call[ka]):+.3f} ms),"
                     f" recoverPose + records stage {verdict(pose[ka], pose[kb])}"
                     f" ({np.median(pose[kb]) - np.median(pose[ka]):+.3f} ms),"
                     f" match stage {verdict(match[ka], match[kb])} ({np.median(match[kb]) - np.median(match[ka]):+.3f} ms)")
        for fs in legs.values():
            fs.close()
        del legs, lms, trs, recs, d_frames
    if a.ab_lib:
        torch.cuda.empty_cache()
        unbound_ab(a, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
