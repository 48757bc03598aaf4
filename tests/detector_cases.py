"""Named 8-bit images that drive oracle/sift.cpp and oracle/surf.cpp (and with them csrc/sift.hip and
csrc/surf.hip) into the branches the textured and synthetic frames of the other tests never enter:
test_detector_census.py counts the branches with the oracle, test_gpu_detector_regimes.py compares
the GPU with the oracle on every case, test_detector_anchors.py pins the oracle itself on the anchor
cases.  Pure numpy, seeded, no files.  Three sizes only (w x h: 40 x 30, 96 x 96, 176 x 160), so that
the group detectors take the cases of a size as one stack."""
import numpy as np

SIZES = ((40, 30), (96, 96), (176, 160))

# the anchor image (test_detector_anchors.py): background 100, (cx, cy, std, amplitude)
ANCHOR_BG = 100.0
ANCHOR_BLOBS = ((40.3, 40.6, 3.0, 120.0), (100.5, 45.25, 5.0, -80.0), (50.0, 110.0, 8.0, 100.0), (120.7, 115.2, 2.0, 140.0))

# the orientation anchors: a blob of std 4, amplitude 70 at the centre of 96 x 96 on a ramp of 2.5 grey / px
# whose intensity increases along image angle theta (x right, y down)
RAMP_ANGLES = (0, 37, 90, 135, 200, 270, 315)
RAMP_SLOPE, RAMP_BLOB = 2.5, (48.0, 48.0, 4.0, 70.0)

TILE = 48  # side of the noise tile of the tiled cases


def _u8(f):
    return np.ascontiguousarray(np.clip(np.rint(f), 0, 255).astype(np.uint8))


def _grid(w, h):
    return np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))


def blobs(w, h, bg, spec):
    """bg plus Gaussian blobs (cx, cy, std, amplitude), as float64."""
    x, y = _grid(w, h)
    f = np.full((h, w), float(bg))
    for cx, cy, s, a in spec:
        f += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return f


def anchor():
    return _u8(blobs(176, 160, ANCHOR_BG, ANCHOR_BLOBS))


def ramp_blob(theta_deg):
    """The orientation anchor of angle theta: 128 at the centre, rising 2.5 grey / px along theta."""
    x, y = _grid(96, 96)
    t = np.deg2rad(theta_deg)
    ramp = 128.0 + RAMP_SLOPE * ((x - 48.0) * np.cos(t) + (y - 48.0) * np.sin(t))
    return _u8(ramp + blobs(96, 96, 0.0, (RAMP_BLOB,)))


def ridges():
    """Two vertical Gaussian ridges, constant along y (singular 3 x 3 systems, det <= 0), and three
    blobs beside them so that the image has keypoints."""
    x, _ = _grid(96, 96)
    f = 60.0 + 120.0 * np.exp(-((x - 30.0) ** 2) / (2 * 3.0 ** 2)) + 90.0 * np.exp(-((x - 62.5) ** 2) / (2 * 5.0 ** 2))
    return _u8(f + blobs(96, 96, 0.0, ((82.3, 20.6, 3.0, 110.0), (80.0, 50.0, 4.0, -50.0), (83.5, 78.25, 2.5, 120.0))))


def big_blob(std):
    """A centred blob of std 6 or 7 px in 40 x 30: the descriptor radius exceeds the image diagonal."""
    return _u8(blobs(40, 30, 40.0, ((19.6, 14.7, float(std), 180.0),)))


def corner_blobs(w, h):
    """Blobs within a few pixels of a corner and of the borders: orientation and descriptor windows cut."""
    spec = ((6.3, 5.6, 1.6, 150.0), (w - 7.2, 6.4, 2.2, -90.0), (7.5, h - 6.7, 2.0, 130.0), (w - 9.4, h - 8.6, 3.0, 140.0),
            (w / 2 + 0.3, 5.8, 1.8, 120.0), (w / 2 - 2.6, h - 6.1, 2.4, -80.0))
    if w >= 96:  # for SURF, which takes no maximum within 11 px of a border: blobs just inside that margin
        m = 15.3
        spec += ((m, m - 0.7, 2.6, 140.0), (w - m - 0.2, h - m + 0.2, 3.2, -100.0), (w - m - 0.6, m + 0.1, 2.8, 130.0),
                 (m - 0.6, h - m - 0.3, 3.0, -100.0), (w / 2 + 0.3, h / 2 - 0.4, 2.7, 120.0))
    return _u8(blobs(w, h, 110.0, spec))


def surf_blobs_40():
    """Four blobs in the band of 40 x 30 where SURF's two smallest middle layers can have maxima."""
    spec = [(12.2 + 5.3 * i, 12.3 if i % 2 == 0 else 17.8, 2.4, 110.0 * (-1) ** i) for i in range(4)]
    return _u8(blobs(40, 30, 125.0, spec))


def edge_blobs():
    """A sharp vertical step edge beside blobs in 40 x 30: the edge's gradients dominate the nearest
    blob's descriptor, whose largest entries exceed 255 before saturate_cast."""
    x, _ = _grid(40, 30)
    f = 128.0 + 90.0 * np.tanh((x - 12.0) / 0.5)
    return _u8(f + blobs(40, 30, 0.0, ((26.0, 16.0, 4.0, 100.0), (31.6, 5.4, 1.5, -120.0), (27.5, 7.7, 1.7, -120.0),
                                        (34.3, 24.6, 1.7, 120.0), (31.2, 23.6, 1.7, -120.0))))


def block_noise(w, h, seed):
    """Uniform noise in 2 x 2 blocks (candidates from neighbouring layers converge: duplicates)."""
    r = np.random.default_rng(seed).integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(r, np.ones((2, 2), np.uint8)))


def noise(w, h):
    return np.ascontiguousarray(np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8))


def tiled(shift=0):
    """A 48 x 48 noise tile repeated over 176 x 160 (exactly equal SURF responses and SIFT x
    coordinates from tile to tile); shift rolls the frame by that many pixels along x."""
    t = np.random.default_rng(4848).integers(0, 256, (TILE, TILE), dtype=np.uint8)
    img = np.tile(t, (4, 4))[:160, :176]
    return np.ascontiguousarray(np.roll(img, shift, axis=1))


class Case:
    """img: uint8 [h, w]; surf_thr: the SURF threshold the case names (besides 400); min_sift / min_surf:
    the least keypoints the oracle must find (SURF at surf_thr), 0 where the case is meant to have none."""

    def __init__(self, name, img, surf_thr, min_sift=4, min_surf=4):
        self.name, self.img, self.surf_thr, self.min_sift, self.min_surf = name, img, float(surf_thr), min_sift, min_surf
        self.h, self.w = img.shape
        assert (self.w, self.h) in SIZES and img.dtype == np.uint8


_CASES = None


def cases():
    """The case list (built once; the images are not to be written to)."""
    global _CASES
    if _CASES is None:
        # 40 x 30: SURF has two middle layers there and takes maxima in a band of 8 rows only, so the cases
        # made for SIFT's branches are not meant to have SURF keypoints (min_surf 0); surf_blobs_40 is
        c = [Case("big_blob_6", big_blob(6), 10.0, min_surf=0), Case("big_blob_7", big_blob(7), 10.0, min_surf=0),
             Case("corner_blobs_40", corner_blobs(40, 30), 50.0, min_surf=0),
             Case("edge_blobs", edge_blobs(), 10.0, min_surf=0), Case("block_noise_40", block_noise(40, 30, 1), 0.0, min_surf=0),
             Case("surf_blobs_40", surf_blobs_40(), 50.0),
             Case("ridges", ridges(), 100.0)]
        # the orientation anchors are meant to have exactly one keypoint, the blob's
        c += [Case(f"ramp_blob_{a}", ramp_blob(a), 100.0, min_sift=1, min_surf=1) for a in RAMP_ANGLES]
        c += [Case("corner_blobs_96", corner_blobs(96, 96), 50.0), Case("noise_96", noise(96, 96), 0.0),
              Case("corner_blobs_176", corner_blobs(176, 160), 50.0), Case("tiled", tiled(), 100.0), Case("tiled_shifted", tiled(TILE), 100.0),
              Case("noise_176", noise(176, 160), 0.0), Case("block_noise_176", block_noise(176, 160, 2), 0.0),
              # the anchor is meant to have three SURF keypoints: its std-2 blob is below SURF's smallest scale
              Case("anchor", anchor(), 100.0, min_surf=3)]
        for k in c:
            k.img.setflags(write=False)
        _CASES = c
    return _CASES


def by_size(w, h):
    return [c for c in cases() if (c.w, c.h) == (w, h)]


def overflow_neighbours():
    """Two ordinary 512 x 512 frames for either side of overflow_noise(): 60 blobs, and noise in 8 x 8 blocks
    (at threshold 0 about 300 and 3600 SURF keypoints, under the list's 4096)."""
    rng = np.random.default_rng(78)
    spec = [(rng.uniform(30, 480), rng.uniform(30, 480), rng.uniform(2.5, 9), rng.choice([-1.0, 1.0]) * rng.uniform(50, 110))
            for _ in range(60)]
    r = np.random.default_rng(77).integers(0, 256, (64, 64), dtype=np.uint8)
    return _u8(blobs(512, 512, 120.0, spec)), np.ascontiguousarray(np.kron(r, np.ones((8, 8), np.uint8)))


def overflow_noise():
    """Uniform noise at 512 x 512: at threshold 0 SURF finds more keypoints than its device lists hold."""
    return np.ascontiguousarray(np.random.default_rng(512512).integers(0, 256, (512, 512), dtype=np.uint8))
