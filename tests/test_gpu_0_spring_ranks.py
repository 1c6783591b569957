"""SPRING across rank processes (optimizers.minsr_direction_sharded with ``prev``, DESIGN.md
§3g), in the clean-parent window of test_gpu_0_multirank.py and by the pattern of
test_gpu_0_minsr_ranks.py: no `cuda` fixture, fresh rank processes (tests/spring_rank_worker.py)
on device 0 with gloo, at most two at once.
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
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "spring_rank_worker.py"), str(out)],
                                      env=env))
    rcs = [p.wait(timeout=240) for p in procs]
    assert rcs == [0] * world
    return [dict(np.load(f"{out}_{r}.npz")) for r in range(world)]


def test_spring_direction_two_ranks(tmp_path):
    """96 fixed C1 walkers, 48 per rank, a fixed float32 ``prev``, mu = 0.9, against one rank
    holding all of them through the same code.  jv comes complete out of every rank's
    dh_ntk_jvp(part = rank, nparts = 2), whatever the part: bit-identical between the ranks and
    against the single rank, and so are T, A and the solution y; both ranks hold the same phi bit
    for bit; against the one-rank phi only the VJP's sum over walkers is split differently: 2e-5
    of max |phi|, the bound test_gpu_0_minsr_ranks.py holds the same split to.  Measured on the
    MI355X: 7.3e-8."""
    _gpu_or_skip()
    one = _run_ranks(1, tmp_path / "s1")[0]
    two = _run_ranks(2, tmp_path / "s2")
    assert one["T"].shape == (192, 192) and one["jv"].shape == (192,)
    assert np.array_equal(one["T"], one["T_all"]) and np.abs(one["jv"]).max() > 0
    for k in ("jv", "T", "A", "y"):
        assert np.all(np.isfinite(one[k])), k
        assert np.array_equal(two[0][k], two[1][k]), k
        assert np.array_equal(two[0][k], one[k]), k
    assert np.array_equal(two[0]["phi"], two[1]["phi"])
    p1, p2 = one["phi"], two[0]["phi"]
    assert np.all(np.isfinite(p1)) and np.abs(p1).max() > 0
    err = np.abs(p2 - p1).max() / np.abs(p1).max()
    print(f"sharded SPRING direction, 2 ranks against 1: {err:.3e} of max |phi| (lambda = {float(one['lam']):.3e})")
    assert err <= 2e-5, err
