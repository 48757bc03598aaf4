"""FAST workload statistics of the synthetic stream (CPU, numpy): the fraction
of level-0 score pixels that pass the compass pre-test, that are FAST-9
corners, and that survive a strict 3x3 NMS on a score proxy.  These set the
per-tile list lengths of fast_strip_kernel (candidates, corners, keeps).

usage: python tools/fast_stats.py [W H frame]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from droplet_visual_odometry_amd.synth import SceneStream  # noqa: E402

CY = [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]
CX = [0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1]


def run9(m):
    m2 = np.concatenate([m, m[:8]], 0)
    r = np.zeros(m.shape[1:], bool)
    for s in range(16):
        r |= np.all(m2[s:s + 9], 0)
    return r


def stats(img, t=20, border=30):
    img = img.astype(np.int32)
    H, W = img.shape
    y0, y1, x0, x1 = border, H - border, border, W - border
    v = img[y0:y1, x0:x1]
    circ = np.stack([img[y0 + dy:y1 + dy, x0 + dx:x1 + dx] for dx, dy in zip(CX, CY)])
    c0, c4, c8, c12 = circ[0], circ[4], circ[8], circ[12]
    comp = (np.minimum(np.maximum(c0, c8), np.maximum(c4, c12)) > v + t) | \
           (np.maximum(np.minimum(c0, c8), np.minimum(c4, c12)) < v - t)
    corner = run9(circ > v + t) | run9(circ < v - t)
    score = np.zeros(v.shape, np.int32)  # proxy: largest threshold still a corner
    for tt in range(t, 255, 4):
        ok = corner & (run9(circ > v + tt) | run9(circ < v - tt))
        if not ok.any():
            break
        score[ok] = tt
    s = np.pad(score, 1)
    nb = np.max(np.stack([s[1 + dy:1 + dy + v.shape[0], 1 + dx:1 + dx + v.shape[1]]
                          for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]), 0)
    keep = corner & (score > nb)
    return comp.mean(), corner.mean(), keep.mean()


def wave_rounds(img, t=20, border=31, band_rows=32, tile_w=124):
    """Per wave and tile of fast_strip_kernel (one workgroup per strip, the batch form): the
    compass survivors n and FAST-9 corners k on the wave's score rows, binned as the kernel bins
    them.  A tile's score rows are image rows [r0 - 1, r1] in the strip's first tile and
    [r0 + 1, r1] after it (two are carried), its score columns [xs - 1, min(xe, W - 4)]; wave wid
    takes the row pairs sr_lo + 2 wid + 8 j (+ 1).  Returns arrays n, k over the wave-tiles."""
    img = img.astype(np.int32)
    H, W = img.shape
    comp = np.zeros((H, W), bool)
    corner = np.zeros((H, W), bool)
    v = img[3:H - 3, 3:W - 3]
    circ = np.stack([img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in zip(CX, CY)])
    c0, c4, c8, c12 = circ[0], circ[4], circ[8], circ[12]
    comp[3:H - 3, 3:W - 3] = (np.minimum(np.maximum(c0, c8), np.maximum(c4, c12)) > v + t) | \
                             (np.maximum(np.minimum(c0, c8), np.minimum(c4, c12)) < v - t)
    corner[3:H - 3, 3:W - 3] = run9(circ > v + t) | run9(circ < v - t)
    assert not (corner & ~comp).any()  # the compass test is necessary for a corner
    ns, ks = [], []
    for xs in range(border, W - border, tile_w):
        xe = min(xs + tile_w, W - border)
        x_lo, x_hi = xs - 1, min(xe, W - 4) + 1
        for b, r0 in enumerate(range(border, H - border, band_rows)):
            r1 = min(r0 + band_rows, H - border)
            sr_lo, nsr = (0 if b == 0 else 2), r1 - r0 + 2
            for wid in range(4):
                rows = [r0 - 1 + sr for sr in range(sr_lo, nsr) if (sr - sr_lo) % 8 in (2 * wid, 2 * wid + 1)]
                ns.append(int(comp[rows, x_lo:x_hi].sum()))
                ks.append(int(corner[rows, x_lo:x_hi].sum()))
    return np.array(ns), np.array(ks)


def print_wave_rounds(img, name):
    """Rc = ceil(n / 64) 64-lane score rounds per wave-tile (every compass survivor is scored: the
    score classifies); Rk = ceil(k / 64) is what scoring the corners alone would take, k / (64 Rk)
    the live-lane share of such a round and n / (64 Rc) that of the rounds the kernel runs."""
    n, k = wave_rounds(img)
    if not len(n):
        return
    rc, rk = -(-n // 64), -(-k // 64)
    hist = np.bincount(rc, minlength=4)
    print(f"  {name} {img.shape[1]}x{img.shape[0]}: {len(n)} wave-tiles; per wave-tile candidates {n.mean():.1f} "
          f"(p10 {np.percentile(n, 10):.0f}, p90 {np.percentile(n, 90):.0f}), corners {k.mean():.1f}; "
          f"Rc {rc.mean():.2f} (0/1/2/3+ rounds: {100 * hist[0] / len(n):.0f}/{100 * hist[1] / len(n):.0f}/"
          f"{100 * hist[2] / len(n):.0f}/{100 * hist[3:].sum() / len(n):.0f} %), Rk {rk.mean():.2f}; live lanes: "
          f"candidate rounds {100 * n.sum() / max(1, 64 * rc.sum()):.0f} %, corner rounds "
          f"{100 * k.sum() / max(1, 64 * rk.sum()):.0f} %")


if __name__ == "__main__":
    W, H, fr = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (1280, 720, 5)))
    img = SceneStream(W, H).render(fr).numpy()
    c, k, kp = stats(img)
    print(f"{W}x{H} frame {fr}: compass pass {100 * c:.2f}%  corners {100 * k:.2f}%  NMS keeps ~{100 * kp:.2f}% "
          f"(per 16x128 tile: {2048 * c:.0f} candidates, {2048 * k:.0f} corners, ~{2016 * kp:.0f} keeps)")
    # per-wave score rounds on every pyramid level (the oracle's pyramid)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle  # noqa: E402
    oracle.build()
    for l, lv in enumerate(oracle.pyramid(img)):
        print_wave_rounds(lv, f"level {l}")
