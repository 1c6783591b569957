"""Rank process of tests/test_gpu_0_minsr_ranks.py (not a test module).

``minsr_rank_worker.py OUT MODE [RUN_DIR]``, every rank on device 0 with the gloo backend,
writing OUT_<rank>.npz:

* ``direction``: optimizers.minsr_direction_sharded on this rank's contiguous shard of 96 fixed
  C1 walkers with random diffs (one NaN, on the last shard): the all-reduced and mirrored T,
  the solve matrix A, the solution y and the direction.  The damping is the mean diagonal of
  the centred matrix of all 96 walkers (a well-conditioned solve: condition number at most
  2 x 96 + 1), which every rank computes for itself from the whole batch.
* ``train``: train() with optimizer "minsr", ``sharded`` on, on the small network of
  multirank_worker.py's ``train`` mode: 2 iterations, a checkpoint at every step.
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


def main_direction(out, world, rank):
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
    sl = slice(rank * per, (rank + 1) * per)
    keep = {}
    delta = minsr_direction_sharded(model, params, x_all[sl].contiguous(), diff_all[sl].contiguous(), lam, keep=keep)
    torch.cuda.synchronize()
    np.savez(f"{out}_{rank}.npz", T=keep["T"].cpu().numpy(), A=keep["A"].cpu().numpy(), y=keep["y"].cpu().numpy(),
             delta=delta.flat.cpu().numpy(), T_all=T_all.cpu().numpy(), lam=lam)


def main_train(out, world, rank, run_dir):
    from deephall_amd import Config, train

    cfg = Config.from_dict({
        "batch_size": 60, "seed": 42,
        "system": {"nspins": (3, 0), "flux": 2, "interaction_strength": 0.0},
        "network": {"psiformer": {"num_layers": 1, "num_heads": 1, "heads_dim": 4}},
        "mcmc": {"burn_in": 4},
        "optim": {"iterations": 2, "optimizer": "minsr", "minsr": {"sharded": True}},
        "log": {"save_path": run_dir, "save_time_interval": 0, "save_step_interval": 1},
    })
    state = train(cfg)
    torch.cuda.synchronize()
    np.savez(f"{out}_{rank}.npz", params=state.params.flat.cpu().numpy(), data=state.data.cpu().numpy(),
             step=int(state.opt_state.step))


def main():
    out, mode = sys.argv[1], sys.argv[2]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    if mode == "direction":
        main_direction(out, world, rank)
    elif mode == "train":
        main_train(out, world, rank, sys.argv[3])
    else:
        raise SystemExit(f"unknown mode {mode}")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
