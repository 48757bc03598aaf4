"""The many-lane Huffman decoder (csrc/jpeg_split.h, the text the split entropy kernel compiles)
on the host: ops.jpeg_entropy_split_host against ops.jpeg_entropy_host on every fixture, the
corrupt ones included, and tests/jpeg_split_check.cpp under the address and undefined-behaviour
sanitizers: every fixture, and two small files cut at every length and with every byte changed in
turn, each input and output in a heap block of exactly its size.  Equality is exact."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from jpeg_cases import by_name, load_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SPLITS = (16, 32, 128, 4096)
MUTATED = ("17x9_420_", "9x2_gray_")  # as tests/test_jpeg_entropy_host.py


def _scan(blob):
    """The entropy-coded bytes of a file without restart markers: from the end of the SOS header
    to the first marker."""
    b = np.frombuffer(blob, np.uint8)
    pos = 2
    while True:
        assert b[pos] == 0xFF
        m, n = int(b[pos + 1]), (int(b[pos + 2]) << 8) | int(b[pos + 3])
        pos += 2 + n
        if m == 0xDA:
            break
    ff = np.flatnonzero((b[pos:-1] == 0xFF) & (b[pos + 1:] != 0))
    return b[pos:pos + int(ff[0])] if ff.size else b[pos:]  # (a file cut short has no marker after its scan)


def _straddles(scan, split):
    """FF 00 pairs with the FF as a run's last byte and the 00 as the next one's first."""
    s = np.arange(split, scan.size, split)
    return int(((scan[s - 1] == 0xFF) & (scan[s] == 0)).sum())


def _parseable():
    return [c for c in load_cases() if c.probe_status == 0]


def test_fixture_facts():
    """What the other tests rely on: restart-free scans of more runs than a workgroup has lanes,
    stuffed pairs that straddle two runs, restart-free corrupt files."""
    from droplet_visual_odometry_amd import ops
    cases = _parseable()
    assert len(cases) == 202
    assert sum(ops.jpeg_entropy_host(c.blob)[0].segments == 1 for c in cases) == 156
    for i in range(4):
        scan = _scan(by_name(f"stream_{i}").blob)
        assert 27_000 < scan.size < 31_500
        assert 1024 < -(-scan.size // 16) < 2048 and 200 < -(-scan.size // 128) < 250
    checker = _scan(by_name("67x50_420_checker_q100_none").blob)
    assert int(((checker[:-1] == 0xFF) & (checker[1:] == 0)).sum()) == 535
    want = {"67x50_420_checker_q100_none": (36, 17, 8, 5), "stream_0": (8, 5, 3, 1), "stream_3": (9, 7, 5, 2)}
    for name, counts in want.items():
        scan = _scan(by_name(name).blob)
        got = tuple(_straddles(scan, s) for s in (16, 32, 64, 128))
        assert got == counts and min(got) > 0, (name, got)
    for name in ("neg_truncated", "neg_random_scan"):
        lay, _, st = ops.jpeg_entropy_host(by_name(name).blob)
        assert lay.segments == 1 and st == -8


@pytest.mark.parametrize("split", SPLITS)
def test_split_host_equals_one_lane(split):
    from droplet_visual_odometry_amd import ops
    most = (0, "", 0)
    for c in _parseable():
        lay, want, st = ops.jpeg_entropy_host(c.blob)
        got, gst, passes = ops.jpeg_entropy_split_host(c.blob, split)
        assert gst == st == c.entropy_status, c.name
        np.testing.assert_array_equal(got, want, err_msg=f"{c.name} at {split}")
        if lay.segments == 1:
            runs = -(-_scan(c.blob).size // split)
            assert passes <= max(runs, 0), (c.name, passes, runs)
            if c.kind != "negative":
                most = max(most, (passes, c.name, runs))
        else:
            assert passes <= -(-len(c.blob) // split)
    print(f"split_bytes {split}: at most {most[0]} synchronisation passes ({most[1]}, {most[2]} runs)")
    if split == 4096:
        assert most[0] <= 8  # (the longest scan has 8 runs)


def test_bad_split_bytes():
    from droplet_visual_odometry_amd import ops
    from droplet_visual_odometry_amd._native import DVOError
    blob = by_name("stream_0").blob
    for bad in (0, 8, 24, 8192, -16):
        with pytest.raises(DVOError) as e:
            ops.jpeg_entropy_split_host(blob, bad)
        assert e.value.code == -1


def test_jpeg_split_check_under_sanitizers(tmp_path):
    cases = load_cases()
    mutate = {next(c.name for c in cases if c.name.startswith(p) and "_none" in c.name) for p in MUTATED}
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<iiiI", c.probe_status, c.entropy_status, int(c.name in mutate), len(c.blob)))
            f.write(c.blob)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "jpeg_split_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "jpeg_split_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.replace(",", "").split()
    assert out[0] == "ok"
    runs, compared, split, corrupt = (int(out[i]) for i in (1, 3, 5, 7))
    assert runs > len(cases) + 600   # the mutations ran
    assert compared > 3 * len(cases)  # and many of them reached the decoders, at every setting
    assert split > compared           # on segments of several runs
    assert corrupt > 100              # many of them corrupt: the one-lane fallback and the tail rules
