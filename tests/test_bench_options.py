"""bench.py's plain run and its options.  CPU only: the argument handling and the output dump, not a run.
A plain run keeps every side leg off and times one run of --steps steps; --full restores them with
their own defaults; --dump-outputs writes float64 arrays a second build can be compared against."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_side_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.runs) == (7, 3, 1)
    assert not a.full and a.dump_outputs is None
    assert a.cpu_seconds == 0 and a.dropin_seconds == 0 and a.tail_world == 0 and a.pose_check_32 == 0
    assert a.no_ref_equivalent and a.no_host_fed and a.config_legs == "none"
    # a leg's own option does not bring it back without --full
    assert _parse(monkeypatch, "--cpu-seconds", "5").cpu_seconds == 0


def test_full_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.runs == 5 and a.cpu_seconds > 0 and a.dropin_seconds > 0 and a.tail_world > 1 and a.pose_check_32 > 0
    assert not a.no_ref_equivalent and not a.no_host_fed
    assert a.config_legs.split(",") == ["c2", "c5", "c3_ocv32"]
    b = _parse(monkeypatch, "--full", "--runs", "2", "--cpu-seconds", "0", "--config-legs", "none")
    assert b.runs == 2 and b.cpu_seconds == 0 and b.config_legs == "none"
    assert _parse(monkeypatch, "--runs", "3").runs == 3


def test_dump_outputs_writes_float64_arrays(tmp_path):
    import bench
    from droplet_visual_odometry_amd._native import PAIR_RECORD_DTYPE
    rng = np.random.default_rng(0)
    recs = np.zeros(5, PAIR_RECORD_DTYPE)
    recs["R"] = rng.standard_normal((5, 9))
    recs["n_matches"] = [1, 2, 3, 4, 5]
    recs["status"] = [0, -3, 0, 0, -6]
    T_rel, T_abs = rng.standard_normal((5, 4, 4)), rng.standard_normal((5, 4, 4))
    d = tmp_path / "out" / "run1"  # created on demand
    bench.dump_outputs(str(d), recs, T_rel, T_abs)
    names = sorted(p.name for p in d.iterdir())
    assert names == sorted([f"records_{f}.npy" for f in bench.DUMP_RECORD_FIELDS] + ["T_rel.npy", "T_abs.npy"])
    for p in d.iterdir():
        assert np.load(p).dtype == np.float64
    assert np.array_equal(np.load(d / "records_R.npy"), recs["R"])
    assert np.array_equal(np.load(d / "records_status.npy"), [0.0, -3.0, 0.0, 0.0, -6.0])
    assert np.array_equal(np.load(d / "T_abs.npy"), T_abs)
    assert set(bench.DUMP_RECORD_FIELDS) == set(PAIR_RECORD_DTYPE.names) - {"pad0", "reserved"}
