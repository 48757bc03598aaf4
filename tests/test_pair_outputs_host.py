"""The owner of a stream's pair outputs (csrc/pair_outputs.h) and the scratches it
sizes (csrc/device_mem.h), checked on the host under the address and
undefined-behaviour sanitizers with a fake allocator in place of the HIP
runtime's and recording fakes of launch_landmarks and launch_tracks
(tests/pair_outputs_check.cpp): the rules of the four binding setters step by
step, the scratches' hipMalloc sizes and order for both streams' shapes, a
failure of each of those allocations, and every argument of a retiring set's
launches."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pair_outputs_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "pair_outputs_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "pair_outputs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "ok"
