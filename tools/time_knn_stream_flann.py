"""What the FLANN mode of the batched k-NN stream costs (DESIGN.md §3 "Batched FLANN",
dvo_knn_stream_set_flann): stream.KnnFrameStream(matcher="flann").process on device-resident
frames at 8, 32 and 128 frames per call, with and without group detection, against
ops.KnnPairStream(matcher="flann").pair over the same consecutive pairs (host frames, reuse_prev,
the theRNG state chained: one frame up and one record back per pair), SIFT and SURF at 640x480 and
1280x720.  The baseline is always the pair path, never the stream itself.

Method (that of tools/time_knn_stream.py): synthetic frames; per detector and size the legs
alternate run by run in one process; a run of the pair leg is a warm-up pair and then every
consecutive pair of the frames from a fresh thread's state; a run of a stream leg sets that state
and makes one process call on n resident frames ended by a synchronise (after one warm-up call per
leg); host clock, ms per pair; the value is the median of `--runs` runs.  The split of a stream
call into detection, matching (the forests, the search and the ratio test) and geometry comes from
HIP events on the stream in one extra call per leg.  The tool asserts that the records of the legs
agree in every field but n_hypotheses (the schedules differ).  It also reports the deepest kd-tree
level of the first frames' forests (ops.test_flann_batch), the figure behind the number of level
launches.  Every run, the spread (max - min) and the library's source hash go to `--out`.
Verdict per stream leg: faster only if its median is below the pair leg's best run minus 3 x that
leg's spread, the margin of the project's A/B notes.

usage: python tools/time_knn_stream_flann.py [--out profiles/knn_stream_flann_time.txt] [--runs 5 --frames 128]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from droplet_visual_odometry_amd import build, ops  # noqa: E402
from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE  # noqa: E402
from droplet_visual_odometry_amd.stream import KnnFrameStream  # noqa: E402
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

TREES, CHECKS = 5, 50  # v3:207-212


def pair_leg(ks, frames):
    """Seconds for the consecutive pairs of `frames` after a warm-up pair; their records."""
    ks.pair(frames[0], frames[1])
    recs = np.zeros(len(frames) - 1, PAIR_RECORD_DTYPE)
    state = ops.THE_RNG_SEED
    t0 = time.perf_counter()
    for i in range(len(frames) - 1):
        # the cache is valid only after a pair whose record status is 0
        reuse = i > 0 and recs[i - 1]["status"] == 0
        recs[i], state = ks.pair(None if reuse else frames[i], frames[i + 1], reuse_prev=reuse, rng_state=state)
    return time.perf_counter() - t0, recs


def stream_leg(st, d_frames, records):
    st.rng_state = ops.THE_RNG_SEED  # ordered on the stream: no synchronisation
    st.sync()
    t0 = time.perf_counter()
    st.process(d_frames, records, wait_torch=False)
    st.sync()
    return time.perf_counter() - t0


def same_records(a, b):
    return all(np.array_equal(a[n], b[n]) for n in PAIR_RECORD_DTYPE.names if n != "n_hypotheses")


def forest_depth(st, n, cap, dim):
    """The deepest tree level over the forests of the last call's first n frames."""
    desc, counts = np.zeros((n, cap, dim), np.float32), []
    for f in range(n):
        d = st.features(f)[1]
        desc[f, :len(d)] = d
        counts.append(len(d))
    return ops.test_flann_batch(desc, counts, trees=TREES, checks=CHECKS)["depth"], max(counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_stream_flann_time.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128, help="frames rendered: the pair leg's run and the largest call")
    ap.add_argument("--batches", default="8,32,128")
    ap.add_argument("--sizes", default="640x480,1280x720")
    ap.add_argument("--detectors", default="sift,surf")
    ap.add_argument("--group", type=int, default=16, help="frames per detection launch of the grouped legs")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_knn_stream_flann.py measures on the GPU; none is visible")
    batches = [min(int(b), a.frames) for b in a.batches.split(",")]
    lines = [f"time_knn_stream_flann: source_hash {build.source_hash()} device {torch.cuda.get_device_name(0)}",
             f"trees {TREES} checks {CHECKS}; runs {a.runs}; pair leg: {a.frames - 1} consecutive pairs (reuse_prev, state "
             f"chained) after a warm-up pair; stream legs: one call on n resident frames, group = frames per detection "
             f"launch (0: frame by frame); legs alternate; ms per pair",
             "one machine, one process; host clock around synchronous calls / call + synchronise"]
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        scene = SceneStream(W, H, device="cuda")
        d_frames = torch.cat([scene.render_batch(range(i, min(i + 8, a.frames))) for i in range(0, a.frames, 8)])
        d_frames = d_frames.contiguous()
        frames = d_frames.cpu().numpy()
        torch.cuda.synchronize()
        for det in a.detectors.split(","):
            ks = ops.KnnPairStream(W, H, scene.K, detector=det, matcher="flann", trees=TREES, checks=CHECKS)
            _, recs_pair = pair_leg(ks, frames)  # also the counts that size the stream's slots
            top = int(max(recs_pair["n_kp_prev"].max(), recs_pair["n_kp_cur"].max()))
            cap = (top + 255) // 256 * 256 + 256
            legs = {}
            for g in (0, a.group):
                kw = dict(detect_group=g) if det == "sift" else dict(surf_group=g)
                st = KnnFrameStream(W, H, scene.K, max(batches), detector=det, feat_cap=cap, matcher="flann",
                                    trees=TREES, checks=CHECKS, **kw)
                for n in batches:
                    legs[(g, n)] = (st, st.new_records(n - 1))
            torch.cuda.synchronize()
            for (g, n), (st, rec) in legs.items():
                stream_leg(st, d_frames[:n], rec)  # warm-up
            depth, dtop = forest_depth(legs[(0, batches[0])][0], min(8, batches[-1]), cap, 64 if det == "surf" else 128)
            ms = {"pair": []}
            ms.update({k: [] for k in legs})
            for _ in range(a.runs):
                t, recs_pair = pair_leg(ks, frames)
                ms["pair"].append(1e3 * t / (a.frames - 1))
                for (g, n), (st, rec) in legs.items():
                    ms[(g, n)].append(1e3 * stream_leg(st, d_frames[:n], rec) / (n - 1))
            same = all(same_records(st.records_numpy(rec, n - 1), recs_pair[:n - 1]) for (g, n), (st, rec) in legs.items())
            assert same, f"{W}x{H} {det}: the stream's records differ from the pair path's"
            ok = int((recs_pair["status"] == 0).sum())
            split = {}
            for (g, n), (st, rec) in legs.items():
                st.set_profiling(True)
                st.rng_state = ops.THE_RNG_SEED
                st.process(d_frames[:n], rec, wait_torch=False)
                split[(g, n)] = st.stage_times()
                st.set_profiling(False)
            p = ms["pair"]
            spread = max(p) - min(p)
            bar = min(p) - 3 * spread
            lines.append(f"{W}x{H} {det} + flann: features per frame <= {top}, feat_cap {cap}, {ok} of {a.frames - 1} pairs "
                         f"status 0; records equal (n_hypotheses aside) {same}; deepest tree level of 7 forests over <= "
                         f"{dtop} points: {depth}; forest scratch {ops.knn_stream_flann_bytes(max(batches), cap, TREES) / 2**20:.1f} MiB")
            lines.append(f"  pair path                  runs {' '.join(f'{v:.3f}' for v in p)}  median {np.median(p):.3f}"
                         f"  spread {spread:.3f}")
            for (g, n) in legs:
                v, s = ms[(g, n)], split[(g, n)]
                tot = sum(s.values())
                lines.append(f"  stream {n:3d} frames group {g:2d} runs {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}"
                             f"  spread {max(v) - min(v):.3f}  pair / stream {np.median(p) / np.median(v):.2f}x; "
                             f"median < pair best - 3 x pair spread ({bar:.3f}): {float(np.median(v)) < bar}")
                lines.append(f"    one call, device ms: detection {s['detect']:.3f}  matching {s['match']:.3f}"
                             f"  geometry {s['geometry']:.3f}  (of {tot:.3f}: "
                             f"{100 * s['detect'] / tot:.0f} / {100 * s['match'] / tot:.0f} / "
                             f"{100 * s['geometry'] / tot:.0f} %)")
            for st in {id(st): st for st, _ in legs.values()}.values():
                st.close()
            ks.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
