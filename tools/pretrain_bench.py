"""Cost and effect of fidelity pretraining at N = 6, 2Q = 15 (Laughlin 1/3), 4096 walkers:

  python tools/pretrain_bench.py iteration train|pretrain adam|kfac [iterations]
      wall time of one iteration (mcmc_step, the optimizer's training step, the statistics'
      host read): the energy step or the fidelity step.  The `train` mode uses nothing of
      pretrain.py, so the same file times an older tree:  python tools/pretrain_bench.py ROOT=dir ...
  python tools/pretrain_bench.py illustrate RUN_DIR [seed]
      200 KFAC iterations from scratch against 50 pretraining + 150 KFAC iterations, same seed:
      final energy (mean of the last 20 rows) and fidelity with the Laughlin state (20 batches).
"""

import sys
import time
from pathlib import Path

args = sys.argv[1:]
ROOT = Path(__file__).resolve().parents[1]
if args and args[0].startswith("ROOT="):
    ROOT = Path(args.pop(0)[5:]).resolve()
sys.path[:0] = [str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deephall_amd import Config, make_network  # noqa: E402
from deephall_amd.mcmc import update_mcmc_width  # noqa: E402
from deephall_amd.optimizers import make_optimizer_step  # noqa: E402
from deephall_amd.random import PRNGKey  # noqa: E402
from deephall_amd.train import initalize_state, setup_mcmc  # noqa: E402
from deephall_amd.types import CheckpointState  # noqa: E402


def config(optimizer, **kw):
    d = {"batch_size": 4096, "seed": 7, "system": {"nspins": (6, 0), "flux": 15}, "mcmc": {"burn_in": 50},
         "optim": {"optimizer": optimizer, "iterations": 200}}
    d["optim"].update(kw.pop("optim", {}))
    d.update(kw)
    return Config.from_dict(d)


def iteration(mode, optimizer, iterations=40):
    cfg = config(optimizer)
    model = make_network(cfg.system, cfg.network)
    _, (params, data, _, width) = initalize_state(cfg, model)
    mcmc_step, pmoves = setup_mcmc(cfg, model)
    if mode == "pretrain":
        from deephall_amd.pretrain import make_fidelity_residual, make_reference

        cfg.optim.pretrain.iterations = iterations
        init, step = make_optimizer_step(cfg, model, residual=make_fidelity_residual(model, make_reference(cfg)))
    else:
        init, step = make_optimizer_step(cfg, model)
    state = CheckpointState(params, data, init(params, None, data), width)
    key = PRNGKey(cfg.seed)
    steps = cfg.mcmc.steps
    times = []
    for t in range(10 + iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new_data, _ = mcmc_step(state.params, state.data, key, state.mcmc_width, reduce=False)
        key = key.advance(steps)
        state = state._replace(data=new_data)
        state, stats = step(state, None, n_accept=mcmc_step.last_n_accept, steps=steps)
        pmove = float(stats["pmove"])
        w, pmoves = update_mcmc_width(t, state.mcmc_width, cfg.mcmc.adapt_frequency, pmove, pmoves)
        state = state._replace(mcmc_width=w)
        torch.cuda.synchronize()
        if t >= 10:
            times.append(1000 * (time.perf_counter() - t0))
    times.sort()
    print(f"{mode} iteration, {optimizer}, N=6 2Q=15 B=4096: median {times[len(times) // 2]:.2f} ms "
          f"(min {times[0]:.2f}, max {times[-1]:.2f}; {iterations} iterations after 10) [{ROOT.name}]")


def illustrate(run_dir, seed=7):
    from deephall_amd import train
    from deephall_amd.pretrain import combine_partials, fidelity_partial, make_reference

    for name, npre, nvmc in (("scratch", 0, 200), ("pretrained", 50, 150)):
        cfg = config("kfac", seed=seed, optim={"iterations": nvmc, "pretrain": {"iterations": npre}},
                     log={"save_path": str(Path(run_dir) / name)})
        t0 = time.perf_counter()
        state = train(cfg)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        rows = (Path(run_dir) / name / "train_stats.csv").read_text().splitlines()[1:]
        e = np.array([float(r.split(",")[2]) for r in rows])
        model = make_network(cfg.system, cfg.network)
        cfg.optim.pretrain.iterations = 1
        ref = make_reference(cfg)
        mcmc_step, _ = setup_mcmc(cfg, model)
        key = PRNGKey(seed + 1000)
        data, parts = state.data, []
        for _ in range(20):
            data, _ = mcmc_step(state.params, data, key, state.mcmc_width)
            key = key.advance(cfg.mcmc.steps)
            parts.append(fidelity_partial(model.apply(state.params, data), ref.apply({}, data)))
        _, fid = combine_partials(torch.stack(parts))
        print(f"{name}: {npre} pretraining + {nvmc} KFAC iterations, seed {seed}: energy of the last 20 rows "
              f"{e[-20:].mean():.4f} +- {e[-20:].std() / np.sqrt(20):.4f}, last row {e[-1]:.4f}, "
              f"fidelity with Laughlin {float(fid):.4f} (20 x 4096 walkers), wall {wall:.1f} s")


if __name__ == "__main__":
    if args[0] == "iteration":
        iteration(args[1], args[2], int(args[3]) if len(args) > 3 else 40)
    elif args[0] == "illustrate":
        illustrate(args[1], int(args[2]) if len(args) > 2 else 7)
    else:
        raise SystemExit(__doc__)
