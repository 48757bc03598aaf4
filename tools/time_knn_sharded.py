"""What sharding the batched k-NN stream costs and gives (DESIGN.md §3 "Sharded k-NN stream",
dist.ShardedKnnRunner): modes knn_sift (SIFT + BFMatcher) and flann (SIFT + FLANN) at 640x480 and
1280x720 with group detection, legs
  base      stream.KnnFrameStream.process on n resident frames, one rank: the capability before
            the runner existed, and the baseline
  world 1   the runner at world size 1: one window of n - 1 pairs (detect, finish into the send
            slot, exchange, pose tail, host chain)
  world N   the runner at N = 2, 4, 8 ranks, one GPU each, where the node has that many GPUs.

Method (that of tools/time_knn_stream_flann.py): synthetic frames, resident on each rank's GPU; per
size and mode every leg's ranks are started once as fresh child processes (as bench.py --gpus N
starts its ranks) and warm up; then the legs alternate run by run, a run being one call (base) or
one window (runner) ended by a synchronise, from a fresh thread's theRNG state; host clock on rank
0 after a barrier, ms per pair; the value is the median of `--runs` runs with the spread (max -
min).  `--runs` more profiled calls and windows per leg, alternating in the same way, give the
stream's three stage events on rank 0 (detection / matching, which in the runner contains the wait
for the draws gather / geometry) and the rest of the wall time (in the runner the exchange, the
pose tail and the chain), as medians: the split of the base leg beside the runner's shows which
stage a difference lies in.  The tool asserts that every leg's records equal
the baseline's in every field.  Verdict for world 1 (DESIGN §1's rule, mirrored): its median is
compared with the baseline's best run plus 3 x the baseline's spread.  The scaling at world N is
reported as measured.  Every step of a child (start and warm-up, a run) has its own time limit;
when one runs out the tool kills its children, writes what it has and stops.

usage: python tools/time_knn_sharded.py [--out profiles/knn_sharded_time.txt] [--runs 5 --frames 128]"""
import argparse
import hashlib
import json
import os
import select
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TREES, CHECKS = 5, 50  # v3:207-212
MODES = {"knn_sift": ("sift", "bf"), "flann": ("sift", "flann")}
TAG = "@@ "  # a child's protocol lines on stdout


# ---- a rank (child process) ------------------------------------------------------------------
def worker(a):
    import numpy as np
    import torch
    import torch.distributed as dist
    from droplet_visual_odometry_amd import dist as ddist, ops
    from droplet_visual_odometry_amd._native import Context
    from droplet_visual_odometry_amd.stream import KnnFrameStream
    from droplet_visual_odometry_amd.synth import MARKER_LEN, SceneStream

    def say(**kw):
        print(TAG + json.dumps(kw), flush=True)

    world, rank, n = a.world, a.rank, a.frames
    det, matcher = MODES[a.mode]
    W, H = (int(v) for v in a.size.split("x"))
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(a.port)
    ddist.init_process_group("nccl", rank, world, device=dev, timeout_s=a.step_timeout)
    ctx = Context(rank)
    scene = SceneStream(W, H, device=dev)
    d_all = torch.cat([scene.render_batch(range(i, min(i + 8, n))) for i in range(0, n, 8)]).contiguous()
    corners = torch.from_numpy(np.stack([scene.marker_corners(i) for i in range(n)])).to(dev)
    torch.cuda.synchronize()
    gkw = dict(detect_group=a.group) if det == "sift" else dict(surf_group=a.group)
    fkw = dict(trees=TREES, checks=CHECKS) if matcher == "flann" else {}
    # every rank sizes the slots from the whole stream's counts, so all legs use one feat_cap
    probe = KnnFrameStream(W, H, scene.K, n, detector=det, feat_cap=8192 if det == "sift" else None, ctx=ctx, **gkw)
    rec = probe.process(d_all)
    probe.sync()
    rec = probe.records_numpy(rec, n - 1)
    probe.close()
    top = int(max(rec["n_kp_prev"].max(), rec["n_kp_cur"].max()))
    cap = (top + 255) // 256 * 256 + 256
    base = base_rec = None
    if world == 1:
        base = KnnFrameStream(W, H, scene.K, n, detector=det, feat_cap=cap, matcher=matcher, ctx=ctx, **gkw, **fkw)
        base_rec = base.new_records(n - 1)
    run = ddist.ShardedKnnRunner(W, H, scene.K, n - 1, world, rank, MARKER_LEN, detector=det, matcher=matcher,
                                 feat_cap=cap, ctx=ctx, **gkw, **fkw)
    p0, p1, f0, f1 = ddist.shard_window(n - 1, world, rank)
    mine, cp, cc = d_all[f0:f1], corners[f0:f1 - 1].contiguous(), corners[f0 + 1:f1].contiguous()
    torch.cuda.synchronize()

    def base_run(profile=False):
        if matcher == "flann":
            base.rng_state = ops.THE_RNG_SEED  # ordered on the stream
        base.set_profiling(profile)
        base.sync()
        t0 = time.perf_counter()
        base.process(d_all, base_rec, wait_torch=False)
        base.sync()
        t = time.perf_counter() - t0
        return t, base_rec.cpu().numpy().tobytes(), (base.stage_times() if profile else None)

    def runner_run(profile=False):
        if matcher == "flann":
            run.ks.rng_state = ops.THE_RNG_SEED
        run.reset_pose()
        run.ks.set_profiling(profile)
        run.sync()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        (recs, T_rel, T_abs), = run.step(mine, cp, cc, wait_torch=False)
        run.sync()
        t = time.perf_counter() - t0
        return t, recs.cpu().numpy().tobytes(), (run.ks.stage_times() if profile else None)

    if base is not None:
        base_run()
    runner_run()  # warm-up
    ok = int((rec["status"] == 0).sum())
    say(ready=True, top=top, cap=cap, ok=ok, device=torch.cuda.get_device_name(rank), pairs_local=p1 - p0)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        if cmd in ("base", "basesplit"):
            t, b, s = base_run(profile=cmd == "basesplit")
            say(ms=1e3 * t / (n - 1), sha=hashlib.sha1(b).hexdigest(), wall_ms=1e3 * t, stages=s)
        elif cmd in ("runner", "split"):
            t, b, s = runner_run(profile=cmd == "split")
            say(ms=1e3 * t / (n - 1), sha=hashlib.sha1(b).hexdigest(), wall_ms=1e3 * t, stages=s)
    run.close()
    if base is not None:
        base.close()
    dist.destroy_process_group()


# ---- the parent ------------------------------------------------------------------------------
class Rank:
    def __init__(self, argv, env):
        self.p = subprocess.Popen(argv, stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env)
        self.buf = b""

    def send(self, cmd):
        self.p.stdin.write((cmd + "\n").encode())
        self.p.stdin.flush()

    def read(self, timeout):
        """The next protocol line as a dict, within `timeout` seconds; TimeoutError or RuntimeError."""
        end = time.monotonic() + timeout
        fd = self.p.stdout.fileno()
        while True:
            while b"\n" in self.buf:
                line, self.buf = self.buf.split(b"\n", 1)
                if line.startswith(TAG.encode()):
                    return json.loads(line[len(TAG):])
            left = end - time.monotonic()
            if left <= 0:
                raise TimeoutError
            if select.select([fd], [], [], left)[0]:
                chunk = os.read(fd, 65536)
                if not chunk:
                    raise RuntimeError(f"a rank ended (exit status {self.p.wait()})")
                self.buf += chunk


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def gpu_count():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                       text=True, timeout=120)
    return int(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else 0


def median(v):
    s = sorted(v)
    m = len(s) // 2
    return s[m] if len(s) % 2 else 0.5 * (s[m - 1] + s[m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_sharded_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128, help="resident frames: one call, one window")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--modes", default="knn_sift,flann")
    ap.add_argument("--worlds", default="1,2,4,8")
    ap.add_argument("--group", type=int, default=16, help="frames per detection launch")
    ap.add_argument("--start-timeout", type=float, default=240.0, help="seconds for a leg's ranks to start and warm up")
    ap.add_argument("--step-timeout", type=float, default=60.0, help="seconds for one run; the collectives' timeout too")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    for name, typ in (("world", int), ("rank", int), ("port", int), ("size", str), ("mode", str)):
        ap.add_argument("--" + name, type=typ, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from droplet_visual_odometry_amd import build
    gpus = gpu_count()
    if gpus < 1:
        sys.exit("time_knn_sharded.py measures on the GPU; none is visible")
    asked = sorted({1} | {int(v) for v in a.worlds.split(",")})  # world 1 runs in the baseline's process
    worlds = [w for w in asked if w <= gpus and w < a.frames]
    skipped = [w for w in asked if w not in worlds]
    lines = [f"time_knn_sharded: source_hash {build.source_hash()}; {gpus} GPU(s) on this node; worlds measured "
             f"{worlds}" + (f", not measured (too few GPUs) {skipped}" if skipped else ""),
             f"trees {TREES} checks {CHECKS}; group {a.group}; runs {a.runs}; {a.frames} resident frames: base = one "
             f"KnnFrameStream.process call on one rank; world N = one ShardedKnnRunner window of {a.frames - 1} pairs "
             f"over N ranks (RCCL), one GPU each; legs alternate; ms per pair",
             "each rank a fresh child process; host clock on rank 0 around call / window + synchronise, after a barrier"]
    if gpus == 1:
        lines.append("this node has one GPU: the file holds the world-1 legs only")
    ranks, failed = [], None
    env = dict(os.environ)
    try:
        for size in a.sizes.split(","):
            for mode in a.modes.split(","):
                legs = {}
                for w in worlds:  # one leg's ranks at a time: start, warm up, report ready
                    port = free_port()
                    legs[w] = [Rank([sys.executable, os.path.abspath(__file__), "--worker", "--world", str(w), "--rank",
                                     str(r), "--port", str(port), "--size", size, "--mode", mode, "--frames",
                                     str(a.frames), "--group", str(a.group), "--step-timeout", str(a.step_timeout)], env)
                               for r in range(w)]
                    ranks += legs[w]
                    info = [k.read(a.start_timeout) for k in legs[w]][0]
                    if w == 1:
                        lines.append(f"{size} {mode}: features per frame <= {info['top']}, feat_cap {info['cap']}, "
                                     f"{info['ok']} of {a.frames - 1} pairs status 0; device {info['device']}")
                ms = {"base": []}
                ms.update({w: [] for w in worlds})
                sha = set()
                for _ in range(a.runs):
                    legs[1][0].send("base")
                    got = legs[1][0].read(a.step_timeout)
                    ms["base"].append(got["ms"])
                    sha.add(got["sha"])
                    for w in worlds:
                        for k in legs[w]:
                            k.send("runner")
                        got = [k.read(a.step_timeout) for k in legs[w]]
                        ms[w].append(got[0]["ms"])
                        sha.update(g["sha"] for g in got)
                same = len(sha) == 1
                b = ms["base"]
                bspread = max(b) - min(b)
                bar = min(b) + 3 * bspread
                lines.append(f"  records of all legs and ranks equal the baseline's in every field: {same}")
                lines.append(f"  base     runs {' '.join(f'{v:.3f}' for v in b)}  median {median(b):.3f}  spread {bspread:.3f}")
                # the stage split: profiled calls / windows, the legs alternating as above
                split = {"base": []}
                split.update({w: [] for w in worlds})
                for _ in range(a.runs):
                    legs[1][0].send("basesplit")
                    split["base"].append(legs[1][0].read(a.step_timeout))
                    for w in worlds:
                        for k in legs[w]:
                            k.send("split")
                        split[w].append([k.read(a.step_timeout) for k in legs[w]][0])

                def stage_line(got):
                    d, m, g = (median([x["stages"][k] for x in got]) for k in ("detect", "match", "geometry"))
                    wall = median([x["wall_ms"] for x in got])
                    rest = median([x["wall_ms"] - sum(x["stages"].values()) for x in got])
                    return (f"    profiled, rank 0, median of {len(got)}, ms: detection {d:.3f}  matching {m:.3f}  geometry "
                            f"{g:.3f}  rest of the wall time {rest:.3f}  of {wall:.3f}")

                lines.append(stage_line(split["base"]) + "  (rest: launch and synchronise)")
                for w in worlds:
                    v = ms[w]
                    text = (f"  world {w}  runs {' '.join(f'{x:.3f}' for x in v)}  median {median(v):.3f}  spread "
                            f"{max(v) - min(v):.3f}  base / world {w} {median(b) / median(v):.2f}x")
                    if w == 1:
                        text += f"; median <= base best + 3 x base spread ({bar:.3f}): {median(v) <= bar}"
                    lines.append(text)
                    lines.append(stage_line(split[w]) + "  (matching contains the wait for the draws gather; rest: "
                                 "exchange, pose tail, chain, launch gaps)")
                for k in ranks:
                    k.send("quit")
                for k in ranks:
                    k.p.wait(timeout=a.step_timeout)
                ranks = []
                if not same:
                    raise RuntimeError(f"{size} {mode}: the legs' records differ")
    except (TimeoutError, RuntimeError, subprocess.TimeoutExpired, BrokenPipeError) as e:
        failed = f"stopped: {type(e).__name__} {e} -- a step ran out of its time limit or a rank ended; nothing more was started"
        lines.append(failed)
    finally:
        for k in ranks:
            if k.p.poll() is None:
                k.p.kill()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
