"""The Moore-Read Pfaffian state (networks/pfaffian.py, pfaffian.hip) on MI355X.

* The kernel against `MooreReadCallable`, the float64 skew elimination in torch pushed through
  the callable boundary (torch.func derivatives, hamiltonian.local_energy(callable, system)):
  log psi, E_L and every observable.  The kernel works in double and stores f32 / f64 exactly as
  laughlin.hip and cf.hip do, so the tolerances are those of test_gpu_jain.py.
* Clustered walkers (one pair 1e-3 rad apart, placed so that the pivot search must leave the
  natural order) and permuted walkers: the pivoting signs.
* Analytic pins on every walker of a batch: a lowest-Landau-level singlet (KE = N/2,
  L^2 = Lz = Lz^2 = 0).
* Cross-kernel: N = 2, p = 2 is the Laughlin state w^3 of laughlin.hip.
* MCMC, the training driver with optimizer none, and the overlap estimator's reference.
"""

from __future__ import annotations

import csv

import numpy as np
import pytest
import torch

from deephall_amd import Config, config, hamiltonian, make_network, train
from deephall_amd.networks import Laughlin, MooreRead, MooreReadCallable
from helpers import make_walkers

pytestmark = pytest.mark.gpu
KEYS = ("kinetic", "potential", "angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square")
CASES = [
    dict(nspins=(2, 0), flux=1),  # a single 2x2 block: no elimination step
    dict(nspins=(4, 0), flux=5),  # one elimination step
    dict(nspins=(6, 0), flux=9),
    dict(nspins=(3, 3), flux=9, interaction_type="harmonic"),
    dict(nspins=(8, 0), flux=13, radius=2.5),
    dict(nspins=(4, 0), flux=11, cf_flux=2),
    dict(nspins=(10, 0), flux=17),
]


def build(case):
    system = config.System(nspins=case["nspins"], flux=case["flux"], radius=case.get("radius"),
                           interaction_type=config.InteractionType(case.get("interaction_type", "coulomb")))
    net = config.Network()
    net.type = config.NetworkType.pfaffian
    net.pfaffian.cf_flux = case.get("cf_flux", 1)
    model = make_network(system, net)
    assert isinstance(model, MooreRead)
    ref = MooreReadCallable(case["nspins"], case["flux"], cf_flux=net.pfaffian.cf_flux, system=system)
    return system, model, ref


def geo_scale(x, flux):
    """Q^2 (sum 1/sin theta)^2: the size of the magnetic terms that cancel in KE and L^2."""
    st = torch.sin(x[..., 0].double().cpu())
    return np.maximum(1.0, ((flux / 2) ** 2 * (1 / st).sum(-1) ** 2).numpy())


def phase_err(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def logpsi_errors(model, ref, x, cuda):
    lp = model.apply(model.init(0, device=cuda), x).cpu().numpy()
    lp_ref = ref(None, x.cpu()).numpy()
    return (np.abs(lp.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real)), phase_err(lp.imag, lp_ref.imag))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pfaffian_vs_callable(cuda, case):
    system, model, ref = build(case)
    N = sum(case["nspins"])
    params = model.init(0, device=cuda)
    x = torch.tensor(make_walkers(8, N, seed=7, margin=0.05), device=cuda)
    err_re, err_im = logpsi_errors(model, ref, x, cuda)
    print(f"{case_id(case)}: log psi re {err_re.max():.1e} phase {err_im.max():.1e}")
    assert err_re.max() < 1e-6
    assert err_im.max() < 1e-5
    e, o = hamiltonian.local_energy(model, system)(params, x)
    e_ref, o_ref = hamiltonian.local_energy(ref, system)(ref.init(), x)
    geo = geo_scale(x, case["flux"])
    scale = lambda v: np.maximum(np.maximum(1.0, np.abs(v)), geo)  # noqa: E731
    err = np.max(np.abs(e.cpu().numpy() - e_ref.cpu().numpy()) / scale(e_ref.cpu().numpy()))
    print(f"{case_id(case)}: E_L {err:.1e}")
    assert err < 1e-5
    for k in KEYS:
        r = o_ref[k].cpu().numpy()
        err = np.max(np.abs(o[k].cpu().numpy() - r) / scale(r))
        print(f"{case_id(case)}: {k} {err:.1e}")
        assert err < 1e-5, k


@pytest.mark.parametrize("N", [6, 8])
def test_clustered_walkers(cuda, N):
    """One pair 1e-3 rad apart as electrons (0, 1), (2, 3) and (N - 2, N - 1): an entry of A of
    about 2e3 that the pivot search has to find, in and out of the natural order.  Every walker
    counts."""
    _, model, ref = build(dict(nspins=(N, 0), flux=2 * (N - 1) - 1))
    x = make_walkers(24, N, seed=13, margin=0.05)
    for w in range(24):
        i, k = ((0, 1), (2, 3), (N - 2, N - 1))[w % 3]
        x[w, k] = x[w, i] + np.float32([6e-4, 8e-4])
    x = torch.tensor(x, device=cuda)
    err_re, err_im = logpsi_errors(model, ref, x, cuda)
    print(f"clustered N={N}: log psi re {err_re.max():.1e} phase {err_im.max():.1e}")
    assert err_re.max() < 1e-6
    assert err_im.max() < 1e-5


def test_permutations(cuda):
    """psi is antisymmetric: Re log psi is unchanged and the phase moves by pi x parity."""
    _, model, _ = build(dict(nspins=(8, 0), flux=13))
    params = model.init(0, device=cuda)
    x = torch.tensor(make_walkers(512, 8, seed=17, margin=0.05), device=cuda)
    lp = model.apply(params, x).cpu().numpy()
    # a transposition, a 3-cycle, the reversal (4 transpositions), a 7-cycle, a 5-cycle times a transposition
    for perm, parity in (([1, 0, 2, 3, 4, 5, 6, 7], 1), ([1, 2, 0, 3, 4, 5, 6, 7], 0), ([7, 6, 5, 4, 3, 2, 1, 0], 0),
                         ([3, 5, 0, 7, 1, 2, 6, 4], 0), ([2, 4, 6, 3, 0, 7, 1, 5], 1)):
        inversions = sum(perm[i] > perm[k] for i in range(8) for k in range(i + 1, 8))
        assert inversions % 2 == parity
        lpp = model.apply(params, x[:, perm].contiguous()).cpu().numpy()
        assert np.max(np.abs(lpp.real - lp.real) / np.maximum(1, np.abs(lp.real))) < 1e-6, perm
        assert np.max(phase_err(lpp.imag, lp.imag + np.pi * parity)) < 1e-5, perm


@pytest.mark.parametrize("nspins,flux,p,B", [((4, 0), 5, 1, 4096), ((6, 0), 9, 1, 4096), ((4, 0), 11, 2, 4096),
                                             ((8, 0), 13, 1, 1024), ((10, 0), 17, 1, 512), ((12, 0), 21, 1, 512),
                                             ((16, 0), 29, 1, 256)])
def test_singlet_analytic_pins(cuda, nspins, flux, p, B):
    """KE = N/2, Im KE = 0, L^2 = 0, Lz = Lz^2 = 0 on every walker."""
    system, model, _ = build(dict(nspins=nspins, flux=flux, cf_flux=p))
    N = sum(nspins)
    x = torch.tensor(make_walkers(B, N, seed=3, margin=0.05), device=cuda)
    e, o = hamiltonian.local_energy(model, system)(model.init(0, device=cuda), x)
    geo = geo_scale(x, flux)
    for k, want in (("kinetic", N / 2), ("angular_momentum_square", 0.0), ("angular_momentum_z", 0.0),
                    ("angular_momentum_z_square", 0.0)):
        err = np.max(np.abs(o[k].real.cpu().numpy() - want) / geo)
        print(f"N={N} p={p} {k}: {err:.1e}")
        assert err < 1e-5, (k, err)
    assert np.max(np.abs(o["kinetic"].imag.cpu().numpy()) / geo) < 1e-5
    assert torch.isfinite(e.real).all()


def test_two_electrons_vs_laughlin_kernel(cuda):
    """N = 2, p = 2, 2Q = 3 against laughlin.hip on 512 walkers.  Here Pf = 1 / w and the pair
    part is w^4: psi = w^3, w = w_01.  Laughlin at 2Q = 3 has Q1 = 1/2, the orbitals (v, u), so
    det = v_0 u_1 - u_0 v_1 = -w, and its Jastrow over ordered pairs is w_01 w_10 = -w^2: the two
    factors -1 cancel and the constant phase between the kernels is 0."""
    system = config.System(nspins=(2, 0), flux=3)
    mr = MooreRead((2, 0), 3, cf_flux=2, system=system)
    net = config.Network()
    net.type = config.NetworkType.laughlin
    la = make_network(system, net)
    assert type(la) is Laughlin
    x = torch.tensor(make_walkers(512, 2, seed=5, margin=0.05), device=cuda)
    lpm = mr.apply(mr.init(0, device=cuda), x).cpu().numpy()
    lpl = la.apply(la.init(0, device=cuda), x).cpu().numpy()
    assert np.max(np.abs(lpm.real - lpl.real) / np.maximum(1, np.abs(lpl.real))) < 1e-6
    assert np.max(phase_err(lpm.imag + 0.0, lpl.imag)) < 1e-5
    em, om = hamiltonian.local_energy(mr, system)(mr.init(0, device=cuda), x)
    el, ol = hamiltonian.local_energy(la, system)(la.init(0, device=cuda), x)
    geo = geo_scale(x, 3)
    for k in KEYS:
        a, r = om[k].cpu().numpy(), ol[k].cpu().numpy()
        err = np.max(np.abs(a - r) / np.maximum(np.maximum(1.0, np.abs(r)), geo))
        assert err < 1e-5, (k, err)
    assert np.max(np.abs(em.cpu().numpy() - el.cpu().numpy()) / np.maximum(np.maximum(1.0, np.abs(el.cpu().numpy())), geo)) < 1e-5


def test_pfaffian_mcmc(cuda):
    from deephall_amd.mcmc import make_mcmc_step
    from deephall_amd.random import PRNGKey

    system, model, ref = build(dict(nspins=(6, 0), flux=9))
    params = model.init(0, device=cuda)
    x = torch.tensor(make_walkers(512, 6, seed=9, margin=0.05), device=cuda).contiguous()
    step = make_mcmc_step(model, batch_per_device=512, steps=5)
    x, pmove = step(params, x, PRNGKey(2), 0.3)
    pm = float(pmove)
    assert 0.05 < pm <= 1.0, pm
    assert torch.isfinite(x).all()
    assert (x[..., 0] >= 0).all() and (x[..., 0] <= np.pi).all()
    lp = model.apply(params, x).cpu().numpy()
    lp_ref = ref(None, x.cpu()).numpy()
    assert np.max(np.abs(lp.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real))) < 1e-6
    assert np.max(phase_err(lp.imag, lp_ref.imag)) < 1e-5
    # the value-only and the energy instantiation of the kernel agree on log psi
    _, obs = hamiltonian.local_energy(model, system).raw(params, x)
    obs = obs.cpu().numpy()
    assert np.max(np.abs(obs[:, 6] - lp.real) / np.maximum(1, np.abs(lp.real))) < 1e-6
    assert np.max(phase_err(obs[:, 7], lp.imag)) < 1e-5


def test_pfaffian_driver(cuda, tmp_path):
    """train with network.type pfaffian and optimizer none: MCMC and statistics on pfaffian.hip;
    every iteration logs L^2 = 0 and KE = N/2 = 3 (an exact lowest-Landau-level singlet)."""
    cfg = Config.from_dict({
        "seed": 42,
        "batch_size": 1024,
        "system": {"nspins": (6, 0), "flux": 9},
        "network": {"type": "pfaffian"},
        "mcmc": {"burn_in": 50},
        "optim": {"iterations": 20, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    with open(tmp_path / "train_stats.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 20
    e = np.array([float(r["energy"]) for r in rows])
    print("Moore-Read N=6 2Q=9 energy: mean", e.mean(), "min", e.min(), "max", e.max())
    assert np.isfinite(e).all()
    for r in rows:
        assert abs(float(r["L_square"])) < 1e-3, r
        assert abs(float(r["kinetic"]) - 3.0) < 1e-3, r


class _Adaptor:
    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg

    def call_network(self, params, x, system=None):
        return self.model.apply(params, x)


def test_overlap_reference(cuda):
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import overlap

    cfg = Config.from_dict({"system": {"nspins": (6, 0), "flux": 9}, "network": {"type": "pfaffian"}})
    model = make_network(cfg.system, cfg.network)
    est = overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([6, 0], flux=9), {"reference": "pfaffian"}, {})
    assert isinstance(est.laughlin, MooreRead)
    values, state = est.empty_val_state(3)
    x = torch.tensor(make_walkers(512, 6, seed=2), device=cuda)
    for i in range(3):
        v, state = est.evaluate(i, {}, None, x, None, state, None)
        values["ratio"][i] = v["ratio"].mean()
        values["ratio_square"][i] = v["ratio_square"].mean()
    assert abs(est.digest(values, state)["overlap"].item() - 1.0) < 1e-5
    # the default reference is still the Laughlin state of the system
    cfg3 = Config.from_dict({"system": {"nspins": (3, 0), "flux": 6}, "network": {"type": "pfaffian"}})
    est3 = overlap.OverlapEstimator(_Adaptor(None, cfg3), HallSystem([3, 0], flux=6), {}, {})
    assert type(est3.laughlin) is Laughlin
