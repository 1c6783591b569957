"""The overlap penalty across rank processes (orthogonal.make_orthogonal_residual: one all-gather
of K x DH_NFID doubles per rank, both statistics vectors in one all-reduce), in the clean-parent
window of test_gpu_0_multirank.py and by the pattern of test_gpu_0_pretrain_ranks.py: no `cuda`
fixture, fresh rank processes (tests/orthogonal_rank_worker.py) on device 0 with gloo, at most
two at once.
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
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "orthogonal_rank_worker.py"), str(out)],
                                      env=env))
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0] * world
    return [dict(np.load(f"{out}_{r}.npz")) for r in range(world)]


def test_penalised_loss_two_ranks(tmp_path):
    """Two ranks of 32 walkers against one rank holding the same 64, two states.  The combined sums
    differ from the whole-batch sums in the summation order only (double): each F_k agrees to 1e-6
    and is the same on both ranks, each walker's R agrees to float32 rounding.  The rank-averaged
    Adam-path gradient splits the VJP's sum over walkers differently: 1e-5 of its largest entry.
    (The IQR clip and the centring use each rank's own quantiles and clipped means, averaged; the
    gate holds where the clip is inert in the whole batch and in both halves.)"""
    _gpu_or_skip()
    one = _run_ranks(1, tmp_path / "r1")[0]
    two = _run_ranks(2, tmp_path / "r2")
    f1 = one["fidelities"]
    assert f1.shape == (2,) and np.all((f1 > 0.0) & (f1 < 1.0))
    assert np.array_equal(two[0]["fidelities"], two[1]["fidelities"])
    assert np.all(np.abs(two[0]["fidelities"] - f1) <= 1e-6)
    assert float(two[0]["penalty"]) == float(two[1]["penalty"])
    r2 = np.concatenate([two[0]["r"], two[1]["r"]])
    assert np.all(np.isfinite(one["r"]))
    assert np.max(np.abs(r2 - one["r"]) / np.maximum(1.0, np.abs(one["r"]))) <= 5e-7
    assert complex(two[0]["energy"]) == complex(two[1]["energy"])
    assert abs(complex(two[0]["energy"]) - complex(one["energy"])) <= 1e-5 * abs(complex(one["energy"]))
    assert np.array_equal(two[0]["grad"], two[1]["grad"])
    g1, g2 = one["grad"], two[0]["grad"]
    assert np.all(np.isfinite(g1)) and np.abs(g1).max() > 0
    err = np.abs(g2 - g1).max() / np.abs(g1).max()
    print(f"penalised loss, 2 ranks against 1: F {f1}, gradient {err:.3e} of max |g|")
    assert err <= 1e-5, err
