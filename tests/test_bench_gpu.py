"""bench.py's command line on the device: a plain run times the headline only and, with
--dump-outputs, writes what its last step computed."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.gpu
def test_plain_run_line_and_dump(dev, tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`: one JSON line on stdout with
    the contract's keys, `steps` timed steps, none of --full's objects; Y.npy is a float32 row
    sample of the [1M, 128] output, at most 64 MB, finite."""
    env = {k: v for k, v in os.environ.items() if k != "GNN_BENCH_DETAIL"}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / line["config"]["nnz"] - 1) < 1e-6
    assert line["cpu_baseline"] is None and "detail" not in line
    for k in ("north_star", "cfg3", "cfg4", "train_gcn_cfg2", "cache_cold_median_step_ms",
              "gcn_layer_ms"):
        assert k not in line, k
    files = sorted((tmp_path / "out").iterdir())
    assert [f.name for f in files] == ["Y.npy"]
    assert sum(f.stat().st_size for f in files) <= 64_000_000
    y = np.load(files[0])
    assert y.dtype == np.float32 and y.ndim == 2 and y.shape[1] == 128 and y.shape[0] > 1000
    assert np.isfinite(y).all() and np.abs(y).max() > 0
