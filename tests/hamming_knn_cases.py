"""Hamming 2-NN and ratio test restated in numpy, and the descriptor sets the tests of
BFMatcher(NORM_HAMMING).knnMatch and of the ORB stream's ratio mode share.

The restatement is integer arithmetic: D = popcount(q ^ t); a stable argsort of a row is OpenCV's
batchDistance(K) order (ascending distance, the lower train index first on ties); the ratio test is
Python's `m.distance < ratio * n.distance` on floats, the kept matches in ascending queryIdx
(visual_odometry_v3.py:223-238).  tests/test_hamming_knn_host.py pins its k = 1 column to the
oracle's BFMatcher.match."""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(q, t):
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2)


def knn(q, t, k=2):
    """(train_idx int32[nq, k], dist float32[nq, k]); (-1, FLT_MAX) where fewer than k trains exist."""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), FLT_MAX, np.float32)
    if len(q) and len(t):
        D = hamming(q, t)
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        n = order.shape[1]
        idx[:, :n] = order
        dist[:, :n] = np.take_along_axis(D, order, axis=1)
    return idx, dist


def ratio_matches(q, t, ratio):
    """[(queryIdx, trainIdx, distance)] the ratio test keeps, ascending queryIdx; needs >= 2 trains."""
    idx, dist = knn(q, t, 2)
    return [(i, int(idx[i, 0]), float(dist[i, 0])) for i in range(len(idx))
            if float(dist[i, 0]) < ratio * float(dist[i, 1])]


def flip(row, bits):
    """A copy of a 32-byte row with the given bit positions (0..255) inverted."""
    r = np.array(row, np.uint8)
    for b in bits:
        r[b >> 3] ^= np.uint8(1 << (b & 7))
    return r


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def content(kind, rng, nq, nt):
    """Query and train sets: random rows; rows drawn from a pool of 4 (ties at first and second
    place at once); every row the same (the answer is trains 0 and 1 at distance 0)."""
    if kind == "random":
        return random_rows(rng, nq), random_rows(rng, nt)
    if kind == "pool4":
        pool = random_rows(rng, 4)
        return pool[rng.integers(0, 4, nq)], pool[rng.integers(0, 4, nt)]
    if kind == "same":
        row = random_rows(rng, 1)
        return np.repeat(row, nq, axis=0), np.repeat(row, nt, axis=0)
    raise ValueError(kind)


def planted(rng, nq, nt, slots):
    """Random sets in which query i's two nearest trains sit at slots[i] = (j1, j2) (disjoint
    pairs): near copies of the query, at distances (3, 5), (5, 3) or (4, 4) in turn."""
    q, t = random_rows(rng, nq), random_rows(rng, nt)
    flips = [(3, 5), (5, 3), (4, 4)]
    for i, (j1, j2) in enumerate(slots[:nq]):
        f1, f2 = flips[i % 3]
        t[j1] = flip(q[i], rng.choice(256, f1, replace=False))
        t[j2] = flip(q[i], rng.choice(256, f2, replace=False))
    return q, t


def ratio_frames(rng, counts, cap):
    """Frame slots for the batched ratio stage: frame f + 1's rows are "the rows of frame f with a
    few bits flipped, plus random rows", by query i of frame f in turn: one copy at 0..12 flips (kept
    at any ratio >= 0.75), two copies at the same distance (dropped even at ratio 1), copies at k and
    k + 1 flips, k >= 4 (kept at 1.0, dropped at 0.75), no copy (two random rows near 100: dropped
    at 0.75).  Independent random rows alone sit near 128 +- 8 and would keep nothing."""
    F = len(counts)
    desc = random_rows(rng, F * cap).reshape(F, cap, 32)
    for f in range(F - 1):
        nq, nt = counts[f], counts[f + 1]
        free = list(rng.permutation(nt))
        for i in range(nq):
            g = i % 4
            need = (1, 2, 2, 0)[g]
            if len(free) < need:
                break
            k = int(rng.integers(0, 13)) if g == 0 else int(rng.integers(4, 12))
            for s in range(need):
                kk = k + 1 if (g == 2 and s == 1) else k
                desc[f + 1, free.pop()] = flip(desc[f, i], rng.choice(256, kk, replace=False))
    return desc


def keypoints(rng, F, cap):
    from droplet_visual_odometry_amd._native import KEYPOINT_DTYPE
    k = np.zeros((F, cap), KEYPOINT_DTYPE)
    k["x"] = rng.uniform(0, 640, (F, cap)).astype(np.float32)
    k["y"] = rng.uniform(0, 480, (F, cap)).astype(np.float32)
    return k


# nq: one query, around a wave's 64 rows, around a workgroup's 256; nt: no second neighbour, inside
# one 32-column tile, around it, around a 64-train stage, past two stages
NQ = (1, 63, 64, 65, 255, 256, 257)
NT = (1, 2, 31, 32, 33, 63, 64, 65, 129)


def planted_cases(rng):
    """(q, t, name): the two nearest of a query in one lane's register (j, j + 32), in neighbouring
    lanes (j, j + 1), and on either side of every boundary between the train splits of a
    512-train set (8 stages: splits of 2, 4 and 8 workgroups cut at multiples of 64)."""
    same_lane = [(64 * b + r, 64 * b + r + 32) for b in range(3) for r in range(32)]
    adjacent = [(2 * m, 2 * m + 1) for m in range(96)]
    across = [(B - 1 - m, B + m) for B in range(64, 512, 64) for m in range(9)]
    return [planted(rng, 70, 200, same_lane) + ("same_lane",),
            planted(rng, 70, 200, adjacent) + ("adjacent",),
            planted(rng, 200, 512, across) + ("across_split",)]


# frame counts and slot size of the batched hook's cases: the degenerate counts (no train, no
# query, one query and two trains, a full slot), pairs that keep and drop, and a slot of more than
# one 256-query block
RATIO_BATCHES = (([70, 0, 1, 2, 128], 128), ([128, 100, 70, 128, 64, 40, 128], 128), ([300, 257, 300], 300))
