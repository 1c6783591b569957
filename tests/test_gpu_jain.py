"""Jain composite-fermion states with two Lambda levels (networks/jain.py, cf.hip) on MI355X.

* The kernel against `JainCallable`, the float64 slogdet form of the same state pushed through
  the callable boundary (torch.func derivatives, hamiltonian.local_energy(callable, system)):
  log psi, E_L and every observable.  The kernel works in double, so the tolerances are those of
  test_gpu_laughlin.py for the quasiparticle kernel.
* Analytic pins on every walker of a batch: both levels filled is a lowest-Landau-level singlet
  (KE = N/2, L^2 = Lz = Lz^2 = 0); a single exciton keeps KE = N/2 and has Lz = 1.
* Cross-kernel: one second-level orbital on a filled level 0 is the Laughlin quasiparticle of
  laughlin.hip, a filled level 0 alone the Laughlin ground state.
* MCMC, the training driver with optimizer none, and the overlap estimator's Jain reference.
"""

from __future__ import annotations

import csv

import numpy as np
import pytest
import torch

from deephall_amd import Config, config, hamiltonian, make_network, train
from deephall_amd.networks import Jain, JainCallable, Laughlin
from helpers import make_walkers

pytestmark = pytest.mark.gpu
EXCITON = ((0, -1.5), (0, -0.5), (0, 0.5), (1, 2.5))  # N = 4, 2Q = 9
KEYS = ("kinetic", "potential", "angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square")
CASES = [
    dict(nspins=(4, 0), flux=6),  # Q1 = 0: both edge orbitals, level 0 is one column
    dict(nspins=(6, 0), flux=11),  # Q1 = 1/2
    dict(nspins=(3, 3), flux=11, interaction_type="harmonic"),
    dict(nspins=(8, 0), flux=16, radius=2.5),
    dict(nspins=(4, 0), flux=12, cf_flux=2),
    dict(nspins=(10, 0), flux=21),
    dict(nspins=(4, 0), flux=9, occupation=EXCITON),
]


def build(case):
    system = config.System(nspins=case["nspins"], flux=case["flux"], radius=case.get("radius"),
                           interaction_type=config.InteractionType(case.get("interaction_type", "coulomb")))
    net = config.Network()
    net.type = config.NetworkType.jain
    net.jain.cf_flux = case.get("cf_flux", 1)
    net.jain.occupation = case.get("occupation")
    model = make_network(system, net)
    assert isinstance(model, Jain)
    ref = JainCallable(case["nspins"], case["flux"], cf_flux=net.jain.cf_flux, occupation=net.jain.occupation,
                       system=system)
    return system, model, ref


def geo_scale(x, flux):
    """Q^2 (sum 1/sin theta)^2: the size of the magnetic terms that cancel in KE and L^2."""
    st = torch.sin(x[..., 0].double().cpu())
    return np.maximum(1.0, ((flux / 2) ** 2 * (1 / st).sum(-1) ** 2).numpy())


def phase_err(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k != "occupation") + ("-exciton" if "occupation" in c else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_jain_vs_callable(cuda, case):
    system, model, ref = build(case)
    N = sum(case["nspins"])
    params = model.init(0, device=cuda)
    x = torch.tensor(make_walkers(8, N, seed=7, margin=0.05), device=cuda)
    lp = model.apply(params, x).cpu().numpy()
    lp_ref = ref(None, x.cpu()).numpy()
    err_re = np.max(np.abs(lp.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real)))
    err_im = np.max(phase_err(lp.imag, lp_ref.imag))
    print(f"{case_id(case)}: log psi re {err_re:.1e} phase {err_im:.1e}")
    assert err_re < 1e-6
    assert err_im < 1e-5
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


@pytest.mark.parametrize("nspins,flux,p,B", [((4, 0), 6, 1, 4096), ((6, 0), 11, 1, 4096), ((4, 0), 12, 2, 4096),
                                             ((8, 0), 16, 1, 1024), ((10, 0), 21, 1, 512), ((12, 0), 26, 1, 256)])
def test_ground_state_analytic_pins(cuda, nspins, flux, p, B):
    """Both Lambda levels filled: KE = N/2, Im KE = 0, L^2 = 0, Lz = Lz^2 = 0 on every walker."""
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


def test_exciton_analytic_pins(cuda):
    """One composite fermion in the second level: KE = N/2 = 2 and Lz = 1 on every walker (a single
    exciton determinant is not an L^2 eigenstate, so L^2 is not pinned)."""
    system, model, _ = build(dict(nspins=(4, 0), flux=9, occupation=EXCITON))
    x = torch.tensor(make_walkers(1024, 4, seed=3, margin=0.05), device=cuda)
    e, o = hamiltonian.local_energy(model, system)(model.init(0, device=cuda), x)
    geo = geo_scale(x, 9)
    assert np.max(np.abs(o["kinetic"].real.cpu().numpy() - 2.0) / geo) < 1e-5
    assert np.max(np.abs(o["kinetic"].imag.cpu().numpy()) / geo) < 1e-5
    assert np.max(np.abs(o["angular_momentum_z"].cpu().numpy() - 1.0) / geo) < 1e-5


def _compare_kernels(cuda, jain, laughlin, system, N, flux):
    """cf.hip against laughlin.hip on 512 walkers.  laughlin.hip's Jastrow runs over ordered pairs,
    prod_{i != k} w_ik = prod_{i<k} (-w_ik^2): a phase pi for each of the N (N - 1) / 2 pairs on
    top of the 2 sum_{i<k} log w_ik of the Jain definition; every derivative is the same."""
    x = torch.tensor(make_walkers(512, N, seed=5, margin=0.05), device=cuda)
    lpj = jain.apply(jain.init(0, device=cuda), x).cpu().numpy()
    lpl = laughlin.apply(laughlin.init(0, device=cuda), x).cpu().numpy()
    assert np.max(np.abs(lpj.real - lpl.real) / np.maximum(1, np.abs(lpl.real))) < 1e-6
    assert np.max(phase_err(lpj.imag + np.pi * (N * (N - 1) // 2), lpl.imag)) < 1e-5
    ej, oj = hamiltonian.local_energy(jain, system)(jain.init(0, device=cuda), x)
    el, ol = hamiltonian.local_energy(laughlin, system)(laughlin.init(0, device=cuda), x)
    geo = geo_scale(x, flux)
    for k in KEYS:
        a, r = oj[k].cpu().numpy(), ol[k].cpu().numpy()
        err = np.max(np.abs(a - r) / np.maximum(np.maximum(1.0, np.abs(r)), geo))
        assert err < 1e-5, (k, err)
    assert np.max(np.abs(ej.cpu().numpy() - el.cpu().numpy()) / np.maximum(np.maximum(1.0, np.abs(el.cpu().numpy())), geo)) < 1e-5


@pytest.mark.parametrize("N,m1", [(4, -2.0), (4, 1.0), (6, 0.0), (6, 3.0)])
def test_one_second_level_orbital_vs_laughlin_quasiparticle(cuda, N, m1):
    flux = 3 * (N - 1) - 1  # N = 2 Q1 + 2
    Q1 = (N - 2) / 2
    system = config.System(nspins=(N, 0), flux=flux, lz_center=m1)
    occ = tuple((0, -Q1 + j) for j in range(N - 1)) + ((1, m1),)
    jain = Jain((N, 0), flux, occupation=occ, system=system)
    net = config.Network()
    net.type = config.NetworkType.laughlin
    laughlin = make_network(system, net)
    assert type(laughlin) is Laughlin
    _compare_kernels(cuda, jain, laughlin, system, N, flux)


def test_level_zero_alone_vs_laughlin_ground_state(cuda):
    system = config.System(nspins=(3, 0), flux=6)
    jain = Jain((3, 0), 6, occupation=((0, -1.0), (0, 0.0), (0, 1.0)), system=system)
    net = config.Network()
    net.type = config.NetworkType.laughlin
    _compare_kernels(cuda, jain, make_network(system, net), system, 3, 6)


def test_jain_mcmc(cuda):
    from deephall_amd.mcmc import make_mcmc_step
    from deephall_amd.random import PRNGKey

    system, model, ref = build(dict(nspins=(6, 0), flux=11))
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


def test_jain_driver(cuda, tmp_path):
    """train with network.type jain and optimizer none: MCMC and statistics on cf.hip; every
    iteration logs L^2 = 0 and KE = N/2 = 3 (an exact lowest-Landau-level singlet)."""
    cfg = Config.from_dict({
        "seed": 42,
        "batch_size": 1024,
        "system": {"nspins": (6, 0), "flux": 11},
        "network": {"type": "jain"},
        "mcmc": {"burn_in": 50},
        "optim": {"iterations": 20, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    with open(tmp_path / "train_stats.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 20
    e = np.array([float(r["energy"]) for r in rows])
    print("Jain N=6 2Q=11 energy: mean", e.mean(), "min", e.min(), "max", e.max())
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

    cfg = Config.from_dict({"system": {"nspins": (6, 0), "flux": 11}, "network": {"type": "jain"}})
    model = make_network(cfg.system, cfg.network)
    est = overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([6, 0], flux=11), {"reference": "jain"}, {})
    assert isinstance(est.laughlin, Jain)
    values, state = est.empty_val_state(3)
    x = torch.tensor(make_walkers(512, 6, seed=2), device=cuda)
    for i in range(3):
        v, state = est.evaluate(i, {}, None, x, None, state, None)
        values["ratio"][i] = v["ratio"].mean()
        values["ratio_square"][i] = v["ratio_square"].mean()
    assert abs(est.digest(values, state)["overlap"].item() - 1.0) < 1e-5
    # the default reference is still the Laughlin state of the system
    cfg3 = Config.from_dict({"system": {"nspins": (3, 0), "flux": 6}, "network": {"type": "jain"}})
    est3 = overlap.OverlapEstimator(_Adaptor(None, cfg3), HallSystem([3, 0], flux=6), {}, {})
    assert type(est3.laughlin) is Laughlin
    with pytest.raises(ValueError):
        overlap.OverlapEstimator(_Adaptor(None, cfg3), HallSystem([3, 0], flux=6), {"reference": "moore-read"}, {})
