"""What SIFT_create(nfeatures) costs and buys in the batched k-NN stream ("SIFT
nfeatures"): stream.KnnFrameStream.process on `--frames` device-resident frames in mode knn_sift
with detect_group `--group`, at nfeatures 0 (everything kept: the baseline), 500 and 2000, at
640x480 and 1280x720.  The protocol is tools/time_sift_batch.py's.

Method: synthetic frames; per size one stream per leg on one context, in one process; the legs
alternate run by run, after one warm-up call each; a run is one process call ended by a
synchronise.  The stage times are the stream's own events (dvo_knn_stream_stage_times): detection
in ms per frame, matching and geometry in ms per pair, the whole call their sum in ms per pair.
The value is the median of `--runs` runs, the spread max - min.  The nfeatures = 0 leg's slots hold
the largest count of the frames (as time_sift_batch.py sizes them); an nfeatures = N leg's hold
N + 64, room for boundary ties, which is the point of the parameter: the matcher's grids follow
feat_cap.  Before anything is timed the first `--check-pairs` records of every leg must equal
ops.KnnPairStream(nfeatures = N).pair's on the same frames (n_hypotheses aside).

Two comparisons, neither against a fixed number:
 1. `--parent-lib PATH` (a libdvo_hip.so built from the parent commit): the nfeatures = 0 leg alone,
    in fresh processes that alternate between that library and this tree's through DVO_LIB_PATH
    (tools/ab_libs.sh's way), `--reps` processes each.  The default path must not be slower: this
    tree's median must lie within the parent's worst run plus 3 x the parent's spread.
 2. The nfeatures > 0 legs against the nfeatures = 0 leg of the same process: the difference per
    stage (retain is one workgroup per frame inside detection; the descriptor stage and the matcher
    do less).  Reported, not gated.
Every run and the library's source hash go to `--out`.

usage: python tools/time_sift_nfeatures.py [--parent-lib PATH] [--out profiles/sift_nfeatures_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("detect", "match", "geometry")


def med(v):
    return float(np.median(v))


def setup(only_default):
    """The package, bound to the library DVO_LIB_PATH names.  only_default: the library may be the
    parent's, which lacks this change's entry points; the nfeatures = 0 leg calls none of them."""
    from droplet_visual_odometry_amd import _native
    if only_default:
        lib = ctypes.CDLL(_native.LIB_PATH)
        for name in [n for n in _native._SIGNATURES if not hasattr(lib, n)]:
            del _native._SIGNATURES[name]


def frames_of(W, H, n):
    import torch
    from droplet_visual_odometry_amd.synth import SceneStream
    scene = SceneStream(W, H, device="cuda")
    d = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).contiguous()
    torch.cuda.synchronize()
    return scene.K, d


def top_count(W, H, d_frames):
    from droplet_visual_odometry_amd import ops
    sb = ops.SiftBatch(W, H, 8)
    _, _, counts = sb.detect_device(d_frames, 16)
    top = int(counts[:, 0].max().item())
    sb.close()
    return top


def run(st, d_frames, records):
    st.process(d_frames, records, wait_torch=False)
    s = st.stage_times()  # waits for the call's last event
    st.sync()
    return s


def measure(W, H, n, group, nfs, runs, check_pairs):
    """{nf: dict(cap, runs per stage, records)} of one size, the legs alternating."""
    import torch
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    K, d_frames = frames_of(W, H, n)
    top = top_count(W, H, d_frames)
    res = {}
    for nf in nfs:
        cap = (top + 255) // 256 * 256 + 256 if nf == 0 else nf + 64
        kw = dict(nfeatures=nf) if nf else {}
        st = KnnFrameStream(W, H, K, n, detector="sift", feat_cap=cap, detect_group=group, **kw)
        res[nf] = dict(st=st, cap=cap, rec=st.new_records(n - 1), runs={s: [] for s in STAGES})
    torch.cuda.synchronize()
    for nf in nfs:
        r = res[nf]
        r["st"].set_profiling(True)
        run(r["st"], d_frames, r["rec"])  # warm-up
        if check_pairs:  # the records against the per-call path, before anything is timed
            got = r["st"].records_numpy(r["rec"], n - 1)
            host = d_frames[:check_pairs + 1].cpu().numpy()
            ks = ops.KnnPairStream(W, H, K, detector="sift", matcher="bf", **(dict(nfeatures=nf) if nf else {}))
            for p in range(check_pairs):
                want, _ = ks.pair(host[p], host[p + 1])
                for f in PAIR_RECORD_DTYPE.names:
                    if f != "n_hypotheses" and not np.array_equal(got[p][f], want[f]):
                        sys.exit(f"{W}x{H} nfeatures {nf}: record {p} field {f} differs from the per-call path")
            ks.close()
    for _ in range(runs):
        for nf in nfs:
            r = res[nf]
            s = run(r["st"], d_frames, r["rec"])
            r["runs"]["detect"].append(s["detect"] / n)
            r["runs"]["match"].append(s["match"] / (n - 1))
            r["runs"]["geometry"].append(s["geometry"] / (n - 1))
    for nf in nfs:
        r = res[nf]
        rec = r["st"].records_numpy(r["rec"], n - 1)
        kept = np.concatenate([rec["n_kp_prev"][:1], rec["n_kp_cur"]])
        r["kept"] = (int(kept.min()), int(np.median(kept)), int(kept.max()))
        r["ok"] = int((rec["status"] == 0).sum())
        r["call"] = [sum(x) for x in zip(*(r["runs"][s] for s in STAGES))]
        r.pop("st").close()
        r.pop("rec")
    return top, res


def child(a):
    """The nfeatures = 0 leg alone, on whatever library DVO_LIB_PATH names: one JSON line."""
    setup(only_default=True)
    out = {}
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        _, res = measure(W, H, a.frames, a.group, [0], a.runs, 0)
        out[size] = dict(detect=res[0]["runs"]["detect"], call=res[0]["call"])
    print("RESULT " + json.dumps(out), flush=True)


def ab_parent(a, lines):
    """Comparison 1: fresh processes alternating between the parent's library and this tree's."""
    from droplet_visual_odometry_amd import build
    libs = (("parent", os.path.abspath(a.parent_lib)), ("this", build.LIB))
    got = {tag: {} for tag, _ in libs}
    for rep in range(a.reps):
        for tag, lib in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--runs", str(a.runs), "--frames", str(a.frames),
                   "--group", str(a.group), "--sizes", a.sizes]
            p = subprocess.run(cmd, env=dict(os.environ, DVO_LIB_PATH=lib), capture_output=True, text=True, timeout=300)
            if p.returncode != 0:  # nothing more is started after a failing process
                sys.exit(f"{tag} library, process {rep}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for size, r in res.items():
                d = got[tag].setdefault(size, dict(detect=[], call=[]))
                d["detect"] += r["detect"]
                d["call"] += r["call"]
    lines.append(f"comparison 1: nfeatures 0 on the parent commit's library and on this tree's, {a.reps} fresh processes each, "
                 f"alternating, {a.runs} runs a process after a warm-up")
    for size in a.sizes.split(","):
        for what, unit in (("detect", "ms/frame"), ("call", "ms/pair")):
            par, cur = got["parent"][size][what], got["this"][size][what]
            bar = max(par) + 3 * (max(par) - min(par))
            for tag, v in (("parent", par), ("this  ", cur)):
                lines.append(f"  {size} {what:6s} {tag} runs {' '.join(f'{x:.4f}' for x in v)}  median {med(v):.4f}  "
                             f"spread {max(v) - min(v):.4f} {unit}")
            lines.append(f"  {size} {what:6s} this median <= parent worst + 3 x parent spread ({bar:.4f}): {med(cur) <= bar}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_nfeatures_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--group", type=int, default=16)
    ap.add_argument("--nfeatures", default="0,500,2000", help="legs; 0, the baseline, must be among them")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--check-pairs", type=int, default=8, help="records compared with the per-call path before timing")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libdvo_hip.so (comparison 1)")
    ap.add_argument("--reps", type=int, default=3, help="processes per library in comparison 1")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if a.child:
        return child(a)
    if not torch.cuda.device_count():
        sys.exit("time_sift_nfeatures.py measures on the GPU; none is visible")
    nfs = [int(v) for v in a.nfeatures.split(",")]
    if 0 not in nfs:
        sys.exit("--nfeatures must contain 0, the baseline")
    from droplet_visual_odometry_amd import build, ops
    n = a.frames
    lines = [f"knn_sift, one process call on {n} resident frames per run, detect_group {a.group}; stage events of the stream; "
             f"median of {a.runs} runs, spread max - min"]
    if a.parent_lib:
        ab_parent(a, lines)  # before this process opens the GPU itself
    else:
        lines.append("comparison 1 (the parent commit's library) was not run: no --parent-lib")
    lines.insert(0, f"time_sift_nfeatures: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}")
    setup(only_default=False)
    lines.append("comparison 2: the nfeatures legs of one process, alternating run by run; detection in ms per frame, matching, "
                 "geometry and the whole call in ms per pair")
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        top, res = measure(W, H, n, a.group, nfs, a.runs, a.check_pairs)
        lines.append(f"{W}x{H}: features per frame <= {top}; the first {a.check_pairs} records of every leg equal the per-call "
                     f"path's; retain scratch {ops.SiftBatch.retain_bytes(a.group) / 1e6:.1f} MB for the group")
        base = res[0]
        for nf in nfs:
            r = res[nf]
            lines.append(f"  nfeatures {nf:5d} feat_cap {r['cap']:5d} kept min/median/max {r['kept'][0]}/{r['kept'][1]}/{r['kept'][2]} "
                         f"pairs status 0 {r['ok']} of {n - 1}")
            for s in STAGES + ("call",):
                v = r["call"] if s == "call" else r["runs"][s]
                line = f"    {s:8s} runs {' '.join(f'{x:.4f}' for x in v)}  median {med(v):.4f}  spread {max(v) - min(v):.4f}"
                if nf:
                    b = base["call"] if s == "call" else base["runs"][s]
                    line += f"  vs nfeatures 0: {med(v) - med(b):+.4f} ({med(b) / med(v):.2f}x)"
                lines.append(line)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
