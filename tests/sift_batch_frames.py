"""Frame stacks of the group SIFT detector's tests: the random-plus-ramp recipe of
test_gpu_sift.py::test_sift_small_and_odd_sizes, another seed per frame, and one constant frame
in the middle of the stack (its neighbours' counters must not leak into it)."""
import numpy as np

CONSTANT = 2  # index of the constant frame in a stack of 5


def textured(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    img = np.clip(img.astype(np.int32) // 2 + np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 128, 0, 255)
    return np.ascontiguousarray(img.astype(np.uint8))


def stack(w, h, n=5):
    """n frames of w x h: textured(seed = w * 31 + h + 1000 f + 1), frame CONSTANT constant (90)."""
    frames = np.stack([textured(w, h, w * 31 + h + 1000 * f + 1) for f in range(n)])
    # the seeds are chosen so that the oracle finds >= 20 keypoints in every textured frame at
    # 161 x 97 (92, 81, -, 82, 65) and 97 x 61 (33, 24, -, 25, 29), and 359 or more at 333 x 211; the
    # tests assert it
    if n > CONSTANT:
        frames[CONSTANT] = 90
    return frames
