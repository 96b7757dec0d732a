"""A plain `bench.py` run sets up, warms up, times its steps, writes --dump-outputs and prints the headline line -- nothing
measured beside it; `--full` goes on after the same timed steps with the rest (roofline, spread, lazy-schedule figures, side file)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--items", "20001", "--steps", "3", "--warmup", "2", "--age-steps", "4"]


def _run(extra, tmp, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["PXR_BENCH_EXTRAS"] = str(tmp / "side.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--dump-outputs", str(tmp / "dump"), *extra], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1 and r.stdout.rstrip().endswith(rows[0]), r.stdout[-2000:]
    return json.loads(rows[0])


def test_plain_run_prints_the_headline_and_full_adds_the_rest_after_the_same_steps(tmp_path):
    plain, full = tmp_path / "plain", tmp_path / "full"
    plain.mkdir()
    full.mkdir()
    d = _run([], plain)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "final_loss", "operands"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 2 and d["value"] > 0
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["roofline"] == {} and d["cpu_baseline"] is None and "extras" not in d and "spread_ms_per_step" not in d
    assert not (plain / "side.json").exists()

    f = _run(["--full", "--no-cpu-baseline"], full)
    assert f["roofline"]["bound"] == "mfma" and f["roofline"]["launches_per_step"] > 0 and f["operands"] == d["operands"]
    assert (full / "side.json").exists() and f["extras"]
    rec = json.load(open(full / "side.json"))
    assert rec["spread"]["blocks"] == 5 and "lazy_flush" in rec and "roofline_adamw_rows" in rec
    # the same timed steps on the same batches: the same loss and the same dumped outputs
    assert f["final_loss"] == d["final_loss"]
    names = sorted(os.listdir(plain / "dump"))
    assert names == sorted(os.listdir(full / "dump")) and "loss.npy" in names
    for n in names:
        assert np.array_equal(np.load(plain / "dump" / n), np.load(full / "dump" / n)), n
