"""Rank process of tests/test_gpu_0_spring_ranks.py (not a test module).

``spring_rank_worker.py OUT``, every rank on device 0 with the gloo backend, writing
OUT_<rank>.npz: optimizers.minsr_direction_sharded with a fixed float32 ``prev`` and momentum 0.9
on this rank's contiguous shard of minsr_rank_worker.py's 96 fixed C1 walkers and diffs (one NaN,
on the last shard), damping the mean diagonal of the centred matrix of all 96 walkers: the
per-walker Jacobian-vector products jv, the all-reduced and mirrored T, the solve matrix A, the
solution y and the direction phi.
"""

from __future__ import annotations

import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MU = 0.9


def main():
    out = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")

    from deephall_amd import config, make_network
    from deephall_amd.optimizers import minsr_direction_sharded, minsr_matrix
    from helpers import make_walkers

    system = config.System(nspins=(3, 0), flux=2)
    model = make_network(system, config.Network())
    params = model.init(3, device="cuda")
    B = 96
    per = B // world
    x_all = torch.tensor(make_walkers(B, 3, seed=5), device="cuda")
    diff_all = np.random.default_rng(29).standard_normal((B, 2)).astype(np.float32)
    diff_all[B - 7] = np.nan
    diff_all = torch.tensor(diff_all, device="cuda")
    ct = torch.zeros(2 * B, 2, device="cuda")
    ct[:B, 0] = 1.0
    ct[B:, 1] = 1.0
    T_all = model.ntk(params, torch.cat([x_all, x_all]), ct)
    lam = float(torch.diagonal(minsr_matrix(T_all, ~torch.isnan(diff_all).any(dim=1), 0.0)).mean())
    # a fixed direction in the parameters' layout (the padding of the flat buffer stays 0)
    prev = model.init(11, device="cuda")
    prev.flat.mul_(0.05)
    sl = slice(rank * per, (rank + 1) * per)
    keep = {}
    phi = minsr_direction_sharded(model, params, x_all[sl].contiguous(), diff_all[sl].contiguous(), lam, keep=keep,
                                  prev=prev, momentum=MU)
    torch.cuda.synchronize()
    np.savez(f"{out}_{rank}.npz", T=keep["T"].cpu().numpy(), A=keep["A"].cpu().numpy(), y=keep["y"].cpu().numpy(),
             jv=keep["jv"].cpu().numpy(), phi=phi.flat.cpu().numpy(), T_all=T_all.cpu().numpy(), lam=lam)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
