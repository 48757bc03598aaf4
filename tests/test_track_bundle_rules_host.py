"""The bundle binding of a stream's pair outputs (csrc/pair_outputs.h) and its scratch
(csrc/device_mem.h), checked on the host under the address and undefined-behaviour sanitizers
with a fake allocator in place of the HIP runtime's and recording fakes of launch_landmarks and
launch_tracks (tests/track_bundle_check.cpp): the fifth setter's rules and parameters, which
setters clear it and that it clears nothing else, the scratch's size and one allocation, a failure
of that allocation, and the arguments of a retiring set's launch under the four combinations of a
refine and a bundle binding."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_track_bundle_rules_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "track_bundle_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "track_bundle_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "ok"
