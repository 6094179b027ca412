"""bench.py's command line: a plain run measures the headline leg alone,
`--full` adds the other legs, `--dump-outputs DIR` writes the last timed
step's pair records as DIR/<field>.npy."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_pkg

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("stage_ms", "from_host", "hard_workload", "latency", "roofline", "roofline_legs", "cpu_baseline")


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_fields(tmp_path):
    """One .npy per PAIR_DTYPE field: poses B x 4 x 4 float32, counts float64 (exact)."""
    pkg = load_pkg()
    recs = np.zeros(5, pkg.PAIR_DTYPE)
    recs["T12"] = np.arange(5 * 16, dtype=np.float32).reshape(5, 16)
    recs["rmse"] = np.float32(0.1) * np.arange(5, dtype=np.float32)
    recs["n_matches"] = [3, 2 ** 31 - 1, 0, 7, 11]
    _load_bench().dump_outputs(str(tmp_path / "d"), recs)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert set(got) == set(pkg.PAIR_DTYPE.names)
    assert got["T12"].dtype == np.float32 and got["T12"].shape == (5, 4, 4)
    assert np.array_equal(got["T12"].reshape(5, 16), recs["T12"])
    assert got["rmse"].dtype == np.float32 and np.array_equal(got["rmse"], recs["rmse"])
    assert got["n_matches"].dtype == np.float64 and np.array_equal(got["n_matches"], recs["n_matches"])


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    """A plain run: --steps timed steps of the headline leg, no other leg in
    the line; the dumped records are the last step's, one per pair."""
    B = 8
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                        "--seq-len", str(B), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: B frames per step
    assert d["value"] == pytest.approx(B / (d["ms_per_step"] * 1e-3), rel=2e-3)
    assert d["step_ms"]["n"] == 2  # one kNN-2 mark per timed step
    assert not any(k in d for k in FULL_ONLY)
    pkg = load_pkg()
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == set(pkg.PAIR_DTYPE.names)
    for name, a in got.items():
        assert a.shape[0] == B and a.dtype == (np.float32 if name in ("T12", "Tcw", "rmse") else np.float64), name
    assert (got["n_matches"] > 100).all() and (got["ransac_ok"] == 1).all()
    assert (got["n_inliers"] <= got["n_good"]).all() and (got["n_good"] <= got["n_matches"]).all()
    for T in (got["T12"], got["Tcw"]):
        assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (B, 1)))
        R = T[:, :3, :3].astype(np.float64)
        # rotations from float32 solvers: orthonormal to a few float32 ulps per entry
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
