"""Rank process of tests/test_gpu_0_orthogonal_ranks.py (not a test module).

``orthogonal_rank_worker.py OUT``, every rank on device 0 with the gloo backend, writing
OUT_<rank>.npz: the penalised loss of make_loss_fn(ENERGY_GRAD, residual=...) — the Adam path —
on this rank's contiguous shard of 64 fixed walkers of (3, 0) at flux 6 against two states, the
Laughlin state and a frozen Psiformer: F_k of the whole batch, this rank's R and the
rank-averaged gradient.
"""

from __future__ import annotations

import dataclasses
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    out = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    from deephall_amd import config, make_network
    from deephall_amd.loss import LossMode, make_loss_fn
    from deephall_amd.orthogonal import frozen_psiformer, make_orthogonal_residual
    from helpers import make_walkers

    system = config.System(nspins=(3, 0), flux=6)
    network = config.Network()
    network.psiformer.num_layers, network.psiformer.num_heads, network.psiformer.heads_dim = 1, 2, 8
    model = make_network(system, network)
    trial = make_network(system, dataclasses.replace(network, type=config.NetworkType.laughlin))
    params = model.init(3, device="cuda")
    states = [trial, frozen_psiformer(model, model.init(8, device="cuda"))]
    B = 64
    per = B // world
    x = torch.tensor(make_walkers(B, 3, seed=5), device="cuda")[rank * per:(rank + 1) * per].contiguous()
    loss = make_loss_fn(model, system, LossMode.ENERGY_GRAD, residual=make_orthogonal_residual(model, states, [2.0, 0.5]))
    stats, grad = loss(params, x)
    torch.cuda.synchronize()
    np.savez(f"{out}_{rank}.npz", fidelities=stats["fidelities"].cpu().numpy(), penalty=float(stats["penalty"]),
             r=loss.last[0].cpu().numpy(), grad=grad.flat.cpu().numpy(), energy=complex(stats["energy"].item()))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
