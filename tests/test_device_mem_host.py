"""The library's owners of device memory (csrc/device_mem.h), checked on the host
under the address and undefined-behaviour sanitizers with a fake allocator in
place of the HIP runtime's (tests/device_mem_check.cpp): the pair sets' hipMalloc
sizes and order, every set's view, a grow that fails at each of its 18
allocations (no set and no live pointer is left, and the next ensure works), one
free per pointer, and the per-call slots' ordinals and growth."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_mem_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "device_mem_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "device_mem_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "ok"
