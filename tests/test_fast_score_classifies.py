"""The invariant fast_strip_kernel relies on (csrc/orb.hip): cornerScore<16>
classifies.  The score is max(thr, A, B) - 1, A the largest minimum of v - c
over the 16 arcs of 9 circle pixels and B the same for c - v; a pixel is a
FAST-9 corner at threshold thr (9 contiguous circle pixels all > v + thr or all
< v - thr) exactly when the score is >= thr, and every other pixel scores
exactly thr - 1.  The kernel therefore scores every compass survivor and has
no separate run-of-9 test.  numpy only."""
import numpy as np
import pytest

THRESHOLDS = [0, 1, 20, 255]


def run9(m):
    """m: bool [n, 16] -> [n]: some 9 circularly contiguous entries are all set."""
    m2 = np.concatenate([m, m[:, :8]], 1)
    r = np.zeros(len(m), bool)
    for s in range(16):
        r |= m2[:, s:s + 9].all(1)
    return r


def is_corner(v, c, thr):
    v = v[:, None]
    return run9(c > v + thr) | run9(c < v - thr)


def corner_score(v, c, thr):
    d = v[:, None] - c
    d2 = np.concatenate([d, d[:, :8]], 1)
    arcs = np.stack([d2[:, s:s + 9] for s in range(16)], 1)  # [n, 16 arcs, 9]
    A = arcs.min(2).max(1)
    B = (-arcs).min(2).max(1)
    return np.maximum(thr, np.maximum(A, B)) - 1


def random_circles(rng, n):
    """Uniform noise, and noise of a small amplitude around the centre (so that
    differences near every threshold occur)."""
    v = rng.integers(0, 256, n)
    c = rng.integers(0, 256, (n, 16))
    amp = rng.integers(1, 48, n)
    near = np.clip(v[:, None] + rng.integers(-1, 2, (n, 16)) * rng.integers(0, amp[:, None] + 1, (n, 16)), 0, 255)
    return np.concatenate([v, v]), np.concatenate([c, near])


def arc_circles(rng, thr):
    """Arcs of length 7..10 and 16 at every start, brighter and darker, whose
    pixels differ from the centre by exactly thr or thr + 1 (or more), the
    rest of the circle at a difference <= thr: lengths 8 and 9 at differences
    thr and thr + 1 are the two sides of the corner definition."""
    vs, cs = [], []
    for sign in (1, -1):
        for length in (7, 8, 9, 10, 16):
            for start in range(16):
                for diff in (thr, thr + 1, thr + 2, thr + 40):
                    for rest in (0, thr, -thr, thr // 2):
                        for v in (0, 1, 100, 128, 254, 255):
                            arc_val = v + sign * diff
                            if not 0 <= arc_val <= 255:
                                continue
                            c = np.full(16, np.clip(v + sign * rest, 0, 255))
                            c[(start + np.arange(length)) % 16] = arc_val
                            vs.append(v)
                            cs.append(c)
                            # one arc pixel pulled back to exactly thr: breaks the run there
                            c2 = c.copy()
                            c2[(start + int(rng.integers(0, length))) % 16] = np.clip(v + sign * thr, 0, 255)
                            vs.append(v)
                            cs.append(c2)
    return np.array(vs), np.array(cs)


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_score_classifies_random(thr):
    rng = np.random.default_rng(1000 + thr)
    v, c = random_circles(rng, 200000)
    corner = is_corner(v, c, thr)
    score = corner_score(v, c, thr)
    np.testing.assert_array_equal(score >= thr, corner)
    np.testing.assert_array_equal(score[~corner], thr - 1)
    if thr < 255:
        assert corner.any() and (~corner).any()
    else:
        assert not corner.any()  # no u8 difference exceeds 255


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_score_classifies_arcs(thr):
    rng = np.random.default_rng(2000 + thr)
    v, c = arc_circles(rng, thr)
    corner = is_corner(v, c, thr)
    score = corner_score(v, c, thr)
    np.testing.assert_array_equal(score >= thr, corner)
    np.testing.assert_array_equal(score[~corner], thr - 1)
    if thr < 255:
        assert corner.any() and (~corner).any()


def test_arc_edges_at_threshold_20():
    """The four edge cases by hand: an arc of 9 at difference 21 is a corner of
    score 20, at difference 20 it is not; an arc of 8 at difference 21 is not."""
    v = np.array([100, 100, 100, 100, 100, 100])
    c = np.full((6, 16), 100)
    c[0, 3:12] = 121   # 9 brighter by thr + 1
    c[1, 3:12] = 120   # 9 brighter by thr
    c[2, 3:11] = 121   # 8 brighter by thr + 1
    c[3, [14, 15, 0, 1, 2, 3, 4, 5, 6]] = 79  # 9 darker by thr + 1, wrapping
    c[4, [14, 15, 0, 1, 2, 3, 4, 5, 6]] = 80  # 9 darker by thr
    c[5, [14, 15, 0, 1, 2, 3, 4, 5]] = 79     # 8 darker by thr + 1
    np.testing.assert_array_equal(is_corner(v, c, 20), [True, False, False, True, False, False])
    np.testing.assert_array_equal(corner_score(v, c, 20), [20, 19, 19, 20, 19, 19])
