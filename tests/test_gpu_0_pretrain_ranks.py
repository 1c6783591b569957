"""The fidelity loss across rank processes (pretrain.make_fidelity_residual: one all-gather of
DH_NFID doubles per rank), in the clean-parent window of test_gpu_0_multirank.py and by the
pattern of test_gpu_0_minsr_ranks.py: no `cuda` fixture, fresh rank processes
(tests/pretrain_rank_worker.py) on device 0 with gloo, at most two at once.
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


def _run_ranks(world, out):
    port = _port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "pretrain_rank_worker.py"), str(out)],
                                      env=env))
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0] * world
    return [dict(np.load(f"{out}_{r}.npz")) for r in range(world)]


def test_fidelity_loss_two_ranks(tmp_path):
    """Two ranks of 32 walkers against one rank holding the same 64.  The combined sums differ
    from the whole-batch sums in the summation order only (double): the fidelity agrees to 1e-6,
    each walker's eps to float32 rounding; both ranks report the same fidelity.  The
    rank-averaged Adam-path gradient splits the VJP's sum over walkers differently: 1e-5 of its
    largest entry.  (The IQR clip uses each rank's own quantiles; at these walkers the float64
    eps lies inside the bounds of the whole batch and of both halves, so it is inert in both
    runs.)  Measured on the MI355X: gradient 2.7e-7."""
    _gpu_or_skip()
    one = _run_ranks(1, tmp_path / "r1")[0]
    two = _run_ranks(2, tmp_path / "r2")
    f1 = float(one["fidelity"])
    assert 0.0 < f1 < 1.0
    assert float(two[0]["fidelity"]) == float(two[1]["fidelity"])
    assert abs(float(two[0]["fidelity"]) - f1) <= 1e-6
    eps2 = np.concatenate([two[0]["eps"], two[1]["eps"]])
    assert np.all(np.isfinite(one["eps"]))
    assert np.max(np.abs(eps2 - one["eps"]) / np.maximum(1.0, np.abs(one["eps"]))) <= 5e-7
    assert np.array_equal(two[0]["grad"], two[1]["grad"])
    g1, g2 = one["grad"], two[0]["grad"]
    assert np.all(np.isfinite(g1)) and np.abs(g1).max() > 0
    err = np.abs(g2 - g1).max() / np.abs(g1).max()
    print(f"fidelity loss, 2 ranks against 1: F {f1:.6f}, gradient {err:.3e} of max |g|")
    assert err <= 1e-5, err
