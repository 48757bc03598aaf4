"""fast_strip_kernel classifies its compass survivors by cornerScore alone
(csrc/orb.hip; the identity is pinned by test_fast_score_classifies.py).
Keypoints byte for byte and descriptors against the oracle, in both OpenCV
semantics and through both launch forms of the kernel: ops.detect_and_compute
(one frame: 8 workgroups per strip) and a 9-frame FrameStream batch (one
workgroup per strip, the bench's form).  nfeatures is the maximum and every
level is asserted to hold fewer keypoints than its quota, so no selection cut
(retainBest) can hide a FAST difference.

Sizes: 333x211 (3 strips x 5 bands of 32 rows at level 0) and 190x131 (the
smallest with two strips and three bands).  Images:
  threshold edge   3- and 5-pixel blocks of the values {79, 80, 100, 120, 121}:
                   circle differences of exactly 20 (no corner) and 21 (corner);
  candidate-dense  uniform noise: several 64-lane candidate rounds per wave;
  seams            a flat background with isolated corners on the rows and
                   columns where bands (31 + 32 k) and strips (31 + 124 k) meet:
                   the carried score rows, the carry list and the strip borders,
                   with adjacent equal-score pairs for the strict NMS."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF = 7680
SIZES = [(333, 211), (190, 131)]
SEMANTICS = ["4.x", "3.2"]
CY = [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]
CX = [0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1]


def edge_image(w, h, block, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([79, 80, 100, 120, 121], np.uint8)
    g = vals[rng.integers(0, 5, ((h + block - 1) // block, (w + block - 1) // block))]
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


def noise_image(w, h, amp, seed):
    """Uniform noise of amplitude amp around 128 (amp 128: rng.integers(0, 256))."""
    n = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.int32)
    return (128 + (n - 128) * amp // 128).astype(np.uint8)


def seam_image(w, h):
    img = np.full((h, w), 100, np.uint8)
    deltas = [21, 60, 20, 155, 22, 40]  # 20: not a corner at the default threshold
    n = [0]

    def put(y, x):
        """One pattern centred on (y, x), cycling kind and contrast."""
        if not (4 <= y < h - 5 and 4 <= x < w - 5):
            return
        k, d = n[0] % 4, deltas[n[0] % len(deltas)]
        n[0] += 1
        if k == 0:    # a bright arc of 11 circle pixels starting anywhere: the centre is the corner
            s = n[0] % 16
            for j in range(11):
                img[y + CY[(s + j) % 16], x + CX[(s + j) % 16]] = 100 + d
        elif k == 1:  # one bright pixel: all 16 circle pixels darker
            img[y, x] = 100 + d
        elif k == 2:  # 2 x 2 block: four adjacent corners of equal score, none a strict maximum
            img[y:y + 2, x:x + 2] = 100 + d
        else:         # horizontal pair of equal scores straddling x / x + 1
            img[y, x:x + 2] = 100 - min(d, 100)

    for y in range(30, h, 32):          # rows 30 + 32 k (= 62 + 32 (k - 1)) and 31 + 32 k (63 + ...)
        for x in range(8, w, 16):
            put(y, x)
            put(y + 1, x + 8)
    for x in range(30, w, 124):         # columns 30 + 124 k, 31 + 124 k (154 + 124 (k - 1), 155 + ...)
        for y in range(6, h, 32):
            put(y, x)
            put(y + 16, x + 1)
    return img


_CACHE = {}


def per_level(kp):
    return np.bincount(kp["octave"], minlength=8)


def case_images(oracle_mod, w, h):
    """The size's four images and, per semantics, the oracle's (keypoints,
    descriptors) of each: computed once, shared by every test, never modified."""
    key = (w, h)
    if key in _CACHE:
        return _CACHE[key]
    quota = np.array(oracle_mod.features_per_level(NF))
    sems = {"4.x": oracle_mod.OCV4, "3.2": oracle_mod.OCV32}

    def refs(img):
        return {s: oracle_mod.detect_and_compute(img, NF, semantics=v) for s, v in sems.items()}

    def under_quota(r):
        return all((per_level(kp) < quota).all() for kp, _ in r.values())

    imgs = [edge_image(w, h, 3, 3), edge_image(w, h, 5, 5)]
    want = [refs(i) for i in imgs]
    amp = 128  # noise: halve the amplitude until no level is full
    while True:
        img = noise_image(w, h, amp, 7)
        r = refs(img)
        if under_quota(r) or amp == 1:
            break
        amp //= 2
    imgs.append(img)
    want.append(r)
    imgs.append(seam_image(w, h))
    want.append(refs(imgs[-1]))
    for i in imgs:
        i.setflags(write=False)
    _CACHE[key] = (imgs, want, quota)
    return _CACHE[key]


@pytest.mark.parametrize("w,h", SIZES)
def test_cases_are_below_quota_and_not_empty(oracle_mod, w, h):
    """The premise of the comparisons below, from the oracle's output alone."""
    imgs, want, quota = case_images(oracle_mod, w, h)
    for k, r in enumerate(want):
        for s, (kp, _) in r.items():
            n = per_level(kp)
            print(f"{w}x{h} image {k} semantics {s}: {len(kp)} keypoints, per level {n.tolist()} (quota {quota.tolist()})")
            assert (n < quota).all(), (k, s, n, quota)
            assert n[0] > 0, (k, s, n)


def check(kg, dg, ref, what):
    ko, do = ref
    assert len(kg) == len(ko), (what, len(kg), len(ko))
    np.testing.assert_array_equal(kg.view(np.uint8), ko.view(np.uint8), err_msg=what)
    np.testing.assert_array_equal(dg, do, err_msg=what)


@pytest.mark.parametrize("opencv", SEMANTICS)
@pytest.mark.parametrize("w,h", SIZES)
def test_single_frame_launch(gpu_ctx, oracle_mod, w, h, opencv):
    from droplet_visual_odometry_amd import ops
    imgs, want, quota = case_images(oracle_mod, w, h)
    for k, img in enumerate(imgs):
        assert (per_level(want[k][opencv][0]) < quota).all()
        kg, dg = ops.detect_and_compute(img, NF, opencv=opencv, ctx=gpu_ctx)
        check(kg, dg, want[k][opencv], f"{w}x{h} image {k} semantics {opencv}")


@pytest.mark.parametrize("opencv", SEMANTICS)
@pytest.mark.parametrize("w,h", SIZES)
def test_batch_launch(gpu_ctx, oracle_mod, w, h, opencv):
    import torch
    from droplet_visual_odometry_amd.stream import FrameStream
    imgs, want, quota = case_images(oracle_mod, w, h)
    order = [k % len(imgs) for k in range(9)]
    frames = np.stack([imgs[k] for k in order])
    K = np.array([[w, 0, w / 2], [0, w, h / 2], [0, 0, 1.0]])
    fs = FrameStream(w, h, K, nfeatures=NF, max_frames=9, ctx=gpu_ctx, opencv=opencv)
    dev = torch.from_numpy(frames).cuda()
    fs.process(dev)
    fs.sync()
    for i, k in enumerate(order):
        assert (per_level(want[k][opencv][0]) < quota).all()
        kg, dg = fs.features(i)
        check(kg, dg, want[k][opencv], f"{w}x{h} frame {i} (image {k}) semantics {opencv}")
    fs.close()
    del dev
