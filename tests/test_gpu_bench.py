"""bench.py's plain run: exactly --steps timed steps, the headline line only, and --dump-outputs writing the same outputs
for the same arguments (seeded inputs), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--batch",
                        "65536", "--steps", "5", "--warmup", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "interactions/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - line["config"]["batch_per_gpu"] / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    for full_only in ("secondary", "cpu_baseline", "extra", "replica_check", "sweep"):
        assert full_only not in line, full_only
    assert "repeats" not in line["roofline"] and "device_copy_GBs" not in line["roofline"]
    names = ("P", "P_rows", "Q", "Q_rows", "epoch_acc")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in names)
    assert a["P"].shape == (20_000, 64) and a["Q"].shape == (5_000, 64) and a["P"].dtype == np.float32
    assert a["epoch_acc"].dtype == np.float64 and a["epoch_acc"][1] == 0 and a["epoch_acc"][0] > 0
    assert np.isfinite(a["P"]).all() and np.isfinite(a["Q"]).all()
    _plain_run(tmp_path / "b")
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in names}
    for n in ("P_rows", "Q_rows"):
        np.testing.assert_array_equal(a[n], b[n])
    for n in ("P", "Q", "epoch_acc"):           # same seeded inputs, same steps: equal up to summation order
        np.testing.assert_allclose(a[n], b[n], rtol=1e-5, atol=1e-6)
