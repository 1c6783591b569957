"""Cost of the overlap penalty (csrc/orthogonal.hip, deephall_amd/orthogonal.py):

  python tools/ortho_bench.py kernels [calls] [repeats]
      dh_ortho_partial + dh_ortho_residual at B = 4096 and 131072 for K = 1, 4, 16 states
      (Re d_k ~ N(0, 3^2) + 500, Im d ~ U(-50, 50), 3 % invalid walkers) against K calls of the
      dh_fidelity_partial + dh_fidelity_residual pair on the same inputs, the two alternating;
      device events around `calls` back-to-back pairs, the median of `repeats`.
  python tools/ortho_bench.py iteration adam|kfac [iterations] [rounds]
      wall time of one training iteration at N = 6, 2Q = 15, B = 4096 (mcmc_step, the optimizer's
      training step, the statistics' host read, ending in a device synchronise): the plain energy
      step, one Laughlin state, one frozen Psiformer of the run's own architecture; the three
      alternate in blocks of `iterations`, `rounds` times, after 10 iterations each.
"""

import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deephall_amd import Config, _lib, make_network  # noqa: E402
from deephall_amd.networks.psiformer import ParamTree, _ptr  # noqa: E402


def median(times):
    times = sorted(times)
    return times[len(times) // 2], times[0], times[-1]


def kernels(calls=200, repeats=5):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for B in (4096, 131072):
        for K in (1, 4, 16):
            g = torch.Generator().manual_seed(K)
            lpsi = torch.stack([-20 + 5 * torch.randn(B, generator=g), 6.28 * (torch.rand(B, generator=g) - 0.5)], -1)
            d = torch.stack([500 + 3 * torch.randn(K, B, generator=g), 100 * (torch.rand(K, B, generator=g) - 0.5)], -1)
            lphi = lpsi + d
            for k in range(K):
                lphi[k, k::33, 0] = float("nan")
            lpsi, lphi = lpsi.cuda().contiguous(), lphi.cuda().contiguous()
            e_l = torch.randn(B, 2, device="cuda")
            part = torch.empty(K, _lib.DH_NFID, dtype=torch.float64, device="cuda")
            weight = torch.full((K,), 0.3, dtype=torch.float64, device="cuda")
            out = torch.empty(B, 2, device="cuda")
            resid = torch.empty(K, B, 2, device="cuda")

            def ortho():
                return (lib.dh_ortho_partial(_ptr(lpsi), _ptr(lphi), B, K, _ptr(part), st)
                        | lib.dh_ortho_residual(_ptr(lpsi), _ptr(lphi), B, K, _ptr(part), _ptr(weight), _ptr(e_l),
                                                _ptr(out), st))

            def fidelity():
                rc = 0
                for k in range(K):
                    rc |= lib.dh_fidelity_partial(_ptr(lpsi), _ptr(lphi[k]), B, _ptr(part[k]), st)
                    rc |= lib.dh_fidelity_residual(_ptr(lpsi), _ptr(lphi[k]), B, _ptr(part[k]), _ptr(resid[k]), st)
                return rc

            times = {"ortho": [], "fidelity": []}
            for fn in (ortho, fidelity):
                for _ in range(10):
                    assert fn() == 0
            torch.cuda.synchronize()
            for _ in range(repeats):
                for name, fn in (("ortho", ortho), ("fidelity", fidelity)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(calls):
                        fn()
                    t1.record()
                    torch.cuda.synchronize()
                    times[name].append(1000 * t0.elapsed_time(t1) / calls)
            (mo, lo, ho), (mf, lf, hf) = median(times["ortho"]), median(times["fidelity"])
            print(f"B={B} K={K}: dh_ortho pair {mo:.1f} us (min {lo:.1f}, max {ho:.1f}); {K} x dh_fidelity pair "
                  f"{mf:.1f} us (min {lf:.1f}, max {hf:.1f}); {repeats} x {calls} calls each, alternating")


def iteration(optimizer, iterations=40, rounds=3):
    from deephall_amd.mcmc import update_mcmc_width
    from deephall_amd.optimizers import make_optimizer_step
    from deephall_amd.orthogonal import frozen_psiformer, make_orthogonal_residual, make_states
    from deephall_amd.random import PRNGKey
    from deephall_amd.train import initalize_state, setup_mcmc
    from deephall_amd.types import CheckpointState

    cfg = Config.from_dict({"batch_size": 4096, "seed": 7, "system": {"nspins": (6, 0), "flux": 15},
                            "optim": {"optimizer": optimizer, "orthogonal": {"states": [{"type": "laughlin"}]}}})
    model = make_network(cfg.system, cfg.network)
    _, (params, data, _, width) = initalize_state(cfg, model)
    mcmc_step, _ = setup_mcmc(cfg, model)
    steps = cfg.mcmc.steps
    (laughlin,), _ = make_states(cfg)
    hooks = {"plain": None, "laughlin": make_orthogonal_residual(model, [laughlin], [1.0]),
             "frozen": make_orthogonal_residual(model, [frozen_psiformer(model, model.init(PRNGKey(99), device=data.device))],
                                                [1.0])}
    runs = {}
    for name, hook in hooks.items():
        init, step = make_optimizer_step(cfg, model, residual=hook)
        p = ParamTree.view_of(model.spec, params.flat.clone())
        runs[name] = [step, CheckpointState(p, data.clone(), init(p, None, data), width), PRNGKey(cfg.seed), [], 0,
                      np.zeros(cfg.mcmc.adapt_frequency)]

    def run(name, n, timed):
        step, state, key, times, t, pmoves = runs[name]
        for _ in range(n):
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
            t += 1
            if timed:
                times.append(1000 * (time.perf_counter() - t0))
        runs[name][1:] = [state, key, times, t, pmoves]

    for name in runs:
        run(name, 10, False)
    for _ in range(rounds):
        for name in runs:
            run(name, iterations, True)
    for name in runs:
        m, lo, hi = median(runs[name][3])
        print(f"{name} iteration, {optimizer}, N=6 2Q=15 B=4096: median {m:.2f} ms (min {lo:.2f}, max {hi:.2f}; "
              f"{rounds} x {iterations} iterations, alternating, after 10)")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "kernels":
        kernels(*(int(a) for a in args[1:3]))
    elif len(args) > 1 and args[0] == "iteration":
        iteration(args[1], *(int(a) for a in args[2:4]))
    else:
        raise SystemExit(__doc__)
