"""bench.py's command line: a plain run times exactly --steps steps and prints the head of the record; --dump-outputs writes
what the last timed step computed; --full (every other leg) is an option of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_offers_full_and_dump_outputs():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    dump = tmp_path / "outputs"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2", "--config", "C1",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "iters/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    assert "roofline" not in line and "cpu_baseline" not in line   # (--full only)
    files = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    rows = files["sample_rows"]
    P = line["config"]["gaussians"]
    assert len(rows) == min(P, 32768) and (np.diff(rows) > 0).all()
    for k in ("loss", "xyz", "features", "opacity", "scaling", "rotation", "exp_avg_features", "exp_avg_sq_xyz", "denom"):
        assert k in files and np.isfinite(files[k]).all(), k
    assert files["xyz"].shape == (len(rows), 3) and files["features"].shape == (len(rows), 16, 3)
    assert float(files["loss"]) > 0 and np.abs(files["exp_avg_sq_xyz"]).sum() > 0
