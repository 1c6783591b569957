"""Sharded MinSR across rank processes (optimizers.minsr_direction_sharded), in
the clean-parent window of test_gpu_0_multirank.py and by its pattern: no `cuda` fixture, fresh
rank processes (tests/minsr_rank_worker.py) on device 0 with gloo, at most two at once.
"""

from __future__ import annotations

import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _gpu_or_skip():
    if torch.cuda.device_count() < 1:  # counts devices without initialising HIP
        pytest.skip("no GPU")
    if torch.cuda.is_initialized():
        pytest.skip("this process already initialised the GPU: rank processes must come from a clean parent")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, out, *args):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "minsr_rank_worker.py"), str(out),
                                       *map(str, args)], env=env))
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0] * world
    return [dict(np.load(f"{out}_{r}.npz")) for r in range(world)]


def test_direction_two_ranks(tmp_path):
    """96 fixed C1 walkers, 48 per rank, against one rank holding all of them through the same
    code.  The doubled batch of 192 spans five dense tile rows (42 walkers each) and two
    128-walker row tiles.  Every entry of T has one owner, so the all-reduced, mirrored T is the
    one-rank T (and plain dh_ntk's) bit for bit, and with it A and the solution y; both ranks
    hold the same direction bit for bit; against the one-rank direction only the VJP's sum over
    walkers is split differently: 2e-5 max |delta|, the bound
    test_gpu_0_multirank.py::test_gradient_allreduce_two_ranks holds the same split to.  Measured
    on the MI355X: 7.5e-7."""
    _gpu_or_skip()
    one = _run_ranks(1, tmp_path / "d1", "direction")[0]
    two = _run_ranks(2, tmp_path / "d2", "direction")
    assert one["T"].shape == (192, 192) and np.abs(one["T"]).max() > 0
    assert np.array_equal(one["T"], one["T"].T) and np.array_equal(one["T"], one["T_all"])
    for k in ("T", "A", "y"):
        assert np.all(np.isfinite(one[k])), k
        assert np.array_equal(two[0][k], two[1][k]), k
        assert np.array_equal(two[0][k], one[k]), k
    assert np.array_equal(two[0]["delta"], two[1]["delta"])
    d1, d2 = one["delta"], two[0]["delta"]
    assert np.all(np.isfinite(d1)) and np.abs(d1).max() > 0
    err = np.abs(d2 - d1).max() / np.abs(d1).max()
    print(f"sharded MinSR direction, 2 ranks against 1: {err:.3e} of max |delta| (lambda = {float(one['lam']):.3e})")
    assert err <= 2e-5, err


def test_train_two_ranks_minsr(tmp_path):
    """train() with optimizer "minsr", sharded, on 2 ranks: 2 iterations with a checkpoint at
    every step.  Both ranks end with identical parameters; the step counter is in the
    checkpoint; one rank running the same job logs the same iteration-0 energy to f32
    rounding."""
    _gpu_or_skip()
    run2 = tmp_path / "run2"
    two = _run_ranks(2, tmp_path / "t2", "train", run2)
    assert np.array_equal(two[0]["params"], two[1]["params"])
    assert np.all(np.isfinite(two[0]["params"]))
    assert int(two[0]["step"]) == 2 and int(two[1]["step"]) == 2
    with np.load(run2 / "ckpt_000001.npz", allow_pickle=False) as f:
        assert "opt_state/step" in f.files and int(f["opt_state/step"]) >= 1
        assert np.array_equal(f["data"], np.concatenate([two[0]["data"], two[1]["data"]]))
    rows = (run2 / "train_stats.csv").read_text().splitlines()
    assert len(rows) == 3 and rows[0].startswith("step,pmove,energy")
    run1 = tmp_path / "run1"
    _run_ranks(1, tmp_path / "t1", "train", run1)
    e1 = [float(r.split(",")[2]) for r in (run1 / "train_stats.csv").read_text().splitlines()[1:]]
    e2 = [float(r.split(",")[2]) for r in rows[1:]]
    assert abs(e1[0] - e2[0]) <= 2e-4  # iteration 0: same walkers, same parameters
