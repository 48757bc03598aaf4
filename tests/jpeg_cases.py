"""Reader of tests/golden/jpeg_cases.npz (written by tests/golden/make_jpeg_cases.py)."""
import functools
import os
import types

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")


@functools.lru_cache(maxsize=None)
def load_cases():
    """Every case: name, kind (small / large / stream / negative), blob (bytes), rgb (Pillow's
    decode, H x W x 3, read-only; None where only hashes are stored), probe_status,
    entropy_status, sha_bgr, sha_gray."""
    z = np.load(PATH)
    out = []
    for i, name in enumerate(z["names"]):
        h, w = (int(v) for v in z["shapes"][i])
        rgb = None
        if h:
            rgb = z["rgb_data"][z["rgb_off"][i]:z["rgb_off"][i + 1]].reshape(h, w, 3)
            rgb.setflags(write=False)
        out.append(types.SimpleNamespace(
            name=str(name), kind=str(z["kinds"][i]), blob=z["blob_data"][z["blob_off"][i]:z["blob_off"][i + 1]].tobytes(),
            rgb=rgb, probe_status=int(z["probe_status"][i]), entropy_status=int(z["entropy_status"][i]),
            sha_bgr=str(z["sha_bgr"][i]), sha_gray=str(z["sha_gray"][i])))
    return tuple(out)


def by_name(name):
    return next(c for c in load_cases() if c.name == name)


def pillow_rgb(blob):
    """Pillow's decode, or None where Pillow is not installed."""
    try:
        from PIL import Image
    except ImportError:
        return None
    import io
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def gray_np(bgr):
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)
