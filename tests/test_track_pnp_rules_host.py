"""Two stand-alone host programs under the address and undefined-behaviour sanitizers (no GPU, and
nothing loaded into Python):
  track_pnp_check.cpp  the PnP binding of a stream's pair outputs (csrc/pair_outputs.h) and its
                       scratch (csrc/device_mem.h) with a fake allocator in place of the HIP
                       runtime's and recording fakes of launch_landmarks and launch_tracks: the sixth
                       setter's rules and parameter ranges, which setters clear it and that it clears
                       nothing, the scratch's size and one allocation, a failure of that allocation,
                       and the arguments of a retiring set's launch with and without the others;
  p3p_check.cpp        csrc/p3p.h itself, the text the kernel compiles: the sample generator and the
                       solver on seeded triples, compared bit for bit with the numpy restatement."""
import os
import shutil
import subprocess

import numpy as np

import track_pnp_cases as pn

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / name)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, name + ".cpp"), "-o", exe], check=True)
    return exe


def test_track_pnp_rules_host(tmp_path):
    exe = _build(tmp_path, "track_pnp_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip() == "ok"


def test_p3p_header_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "p3p_check")
    lines, want = [], []
    for n, hyps, seed in ((3, 512, 0), (4, 128, 0), (5, 64, 7), (64, 128, 2 ** 64 - 1), (1000, 512, 0x9E3779B97F4A7C15)):
        lines.append(f"S {n} {hyps} {seed}")
        want += ["s %d %d %d" % tuple(row) for row in pn.samples(n, hyps, seed)]
    cases = pn.triples(200, 3)
    same = np.tile([[0.1, 0.2, 5.0]], (3, 1)), np.tile([[0.02, 0.04]], (3, 1)), None, None  # identical points: NaN all the way
    for Y, nunv, _, _ in cases + [same]:
        bits = np.concatenate([np.asarray(Y, np.float64).reshape(9), np.asarray(nunv, np.float64).reshape(6)]).view(np.uint64)
        lines.append("T " + " ".join("%016x" % int(b) for b in bits))
        Rs, ts = pn.p3p(Y, nunv)
        want.append("t %d" % len(Rs))
        for s in range(len(Rs)):
            out = np.concatenate([Rs[s].reshape(9), ts[s]]).view(np.uint64)
            want.append(" ".join("%016x" % int(b) for b in out))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
