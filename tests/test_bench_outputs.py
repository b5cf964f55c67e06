"""CPU: bench.py's command line and its `--dump-outputs` writer, without a device (a stand-in handle hands back the state)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

import helpers


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(helpers.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _Handle:
    def __init__(self, P, L, O, seed=0):
        rng = np.random.default_rng(seed)
        self.poses, self.points, self.objects = rng.normal(size=(P, 6)), rng.normal(size=(L, 3)), rng.normal(size=(O, 7))

    def get_poses(self):
        return self.poses

    def get_points(self):
        return self.points

    def get_objects(self):
        return self.objects


class _Iteration:
    def __init__(self, cost):
        self.cost = cost


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_command_line_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_writes_the_state_as_float64(tmp_path):
    bench = _bench()
    ba = _Handle(20, 500, 3)
    bench.dump_outputs(str(tmp_path / "d"), ba, [_Iteration(c) for c in (9.0, 4.0, 3.5)])
    got = _load(tmp_path / "d")
    assert set(got) == {"poses", "points", "objects", "iteration_costs"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["poses"], ba.poses) and np.array_equal(got["points"], ba.points) and np.array_equal(got["objects"], ba.objects)
    assert got["iteration_costs"].tolist() == [9.0, 4.0, 3.5]


def test_dump_outputs_keeps_a_fixed_sample_of_the_features_within_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100000)
    ba = _Handle(20, 20000, 3)                                   # 480 kB of features: over the budget
    its = [_Iteration(1.0)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ba, its)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 100000 and 0 < len(a["points"]) < 20000
    rows = a["point_rows"].astype(np.int64)
    assert np.array_equal(a["point_rows"], b["point_rows"]) and np.all(np.diff(rows) > 0)       # the same rows in every run
    assert np.array_equal(a["points"], ba.points[rows]) and np.array_equal(a["poses"], ba.poses)
