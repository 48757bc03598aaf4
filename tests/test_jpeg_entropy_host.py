"""The JPEG parser and the Huffman decoder the entropy kernel compiles (csrc/jpeg_parse.cpp,
csrc/jpeg_entropy.h), on the host under the address and undefined-behaviour sanitizers
(tests/jpeg_entropy_check.cpp): every fixture and every corrupt case with its expected
statuses, and two small files cut at every length and with every byte changed in turn, each
input and output in a heap block of exactly its size."""
import os
import shutil
import struct
import subprocess

from jpeg_cases import load_cases

HERE = os.path.dirname(os.path.abspath(__file__))

MUTATED = ("17x9_420_", "9x2_gray_")  # the first case of each: two MCU rows of 4:2:0, one row of gray blocks


def test_jpeg_entropy_host(tmp_path):
    cases = load_cases()
    mutate = {next(c.name for c in cases if c.name.startswith(p) and "_none" in c.name) for p in MUTATED}
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<iiiI", c.probe_status, c.entropy_status, int(c.name in mutate), len(c.blob)))
            f.write(c.blob)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "jpeg_entropy_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "jpeg_entropy_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = r.stdout.split()
    assert out[0] == "ok"
    assert int(out[1]) > len(cases) + 600  # the mutations ran
    assert int(out[3]) > len(cases)        # and many of them reached the decoder
