"""bench.py's plain run on the GPU box: the result line of the timed steps alone, and
``--dump-outputs``.  One small run (64 walkers of C1, 2 timed steps) in a fresh process."""

from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_line_and_dump(cuda, tmp_path):
    B, N = 64, 3
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--burn-in", "0", "--batch", str(B), "--nspins", str(N), "0", "--flux", "2",
                          "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "local-energies/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value = walkers x steps / time of the timed steps, the same time ms_per_step reports
    assert line["value"] == pytest.approx(B / (1e-3 * line["ms_per_step"]), rel=2e-3)
    # nothing beside the timed steps ran
    assert line["walker_steps_per_sec"] is None and line["components"] is None and line["roofline"] is None
    assert line["kernels"] == {} and "configs_1gpu" not in line and "cpu_baseline" not in line
    shapes = {"walkers": (B, N, 2), "e_l": (B, 2), "obs": (B, 8), "n_accept": (B,), "stats": (18,)}
    files = sorted(p.name for p in (tmp_path / "dump").iterdir())
    assert files == sorted(f"{k}.npy" for k in shapes)
    arrays = {k: np.load(tmp_path / "dump" / f"{k}.npy") for k in shapes}
    for k, a in arrays.items():
        assert a.shape == shapes[k] and a.dtype in (np.float32, np.float64), k
        assert np.isfinite(a).all(), k
    # the dumped step is the one the line reports: mean E_L of its walkers = the line's energy
    # (to the line's 5 decimals and f32 summation), accept counts within the 10 moves
    e = arrays["e_l"].astype(np.float64).mean(axis=0)
    assert abs(e[0] - line["energy"][0]) <= 2e-5 * max(1.0, abs(e[0])) and abs(e[1] - line["energy"][1]) <= 2e-5
    assert arrays["n_accept"].min() >= 0 and arrays["n_accept"].max() <= 10
    assert arrays["n_accept"].mean() / 10 == pytest.approx(line["pmove"], abs=6e-4)
