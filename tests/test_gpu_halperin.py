"""Halperin (m_up, m_dn, n) states (networks/halperin.py, halperin.hip) on MI355X.

* The kernel against `HalperinCallable`, the float64 torch form pushed through the callable
  boundary (torch.func derivatives, hamiltonian.local_energy(callable, system)): log psi, E_L and
  every observable.  The kernel works in double and stores f32 exactly as the other three analytic
  kernels do, so the tolerances are those of test_gpu_jain.py and test_gpu_pfaffian.py.
* Analytic pins on every walker of a batch: a lowest-Landau-level rotational singlet (KE = N/2,
  L^2 = Lz = Lz^2 = 0).
* dh_logpsi against the log psi of dh_local_energy, bit for bit; two calls; a walker alone, in a
  partial last workgroup, and inside a larger batch.
* Cross-kernel: (3,3,3) is the Laughlin state of laughlin.hip, (3,3,0) two of them.
* MCMC, the training driver with optimizer none, and the overlap estimator's reference.
"""

from __future__ import annotations

import csv

import numpy as np
import pytest
import torch

from deephall_amd import Config, config, hamiltonian, make_network, train
from deephall_amd.networks import Halperin, HalperinCallable, Laughlin
from helpers import make_walkers

pytestmark = pytest.mark.gpu
KEYS = ("kinetic", "potential", "angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square")
CASES = [
    dict(nspins=(2, 2), exponents=(1, 1, 0), flux=1),
    dict(nspins=(2, 2), exponents=(3, 3, 2), flux=7),
    dict(nspins=(3, 3), exponents=(3, 3, 2), flux=12),
    dict(nspins=(2, 2), exponents=(3, 3, 1), flux=5),
    dict(nspins=(4, 2), exponents=(1, 3, 0), flux=3),
    dict(nspins=(3, 3), exponents=(3, 3, 2), flux=12, interaction_type="harmonic"),
    dict(nspins=(2, 2), exponents=(3, 3, 2), flux=7, radius=2.5),
    dict(nspins=(3, 3), exponents=(3, 3, 2), flux=12, poles=True),   # an electron at theta = 1e-3, one at pi - 1e-3
    dict(nspins=(3, 3), exponents=(3, 3, 2), flux=12, close=True),   # an up and a down electron 1e-3 rad apart
]


def build(case):
    system = config.System(nspins=case["nspins"], flux=case["flux"], radius=case.get("radius"),
                           interaction_type=config.InteractionType(case.get("interaction_type", "coulomb")))
    net = config.Network()
    net.type = config.NetworkType.halperin
    net.halperin.exponents = case["exponents"]
    model = make_network(system, net)
    assert isinstance(model, Halperin)
    ref = HalperinCallable(case["nspins"], case["flux"], case["exponents"], system=system)
    return system, model, ref


def walkers(case, B, seed, cuda):
    N, n_up = sum(case["nspins"]), case["nspins"][0]
    x = make_walkers(B, N, seed=seed, margin=0.05)
    if case.get("poles"):
        x[:, 0, 0] = 1e-3
        x[:, N - 1, 0] = np.pi - 1e-3
    if case.get("close"):
        x[:, n_up] = x[:, 0] + np.float32([6e-4, 8e-4])
    return torch.tensor(x, device=cuda)


def geo_scale(x, flux):
    """Q^2 (sum 1/sin theta)^2: the size of the magnetic terms that cancel in KE and L^2."""
    st = torch.sin(x[..., 0].double().cpu())
    return np.maximum(1.0, ((flux / 2) ** 2 * (1 / st).sum(-1) ** 2).numpy())


def phase_err(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_halperin_vs_callable(cuda, case):
    system, model, ref = build(case)
    params = model.init(0, device=cuda)
    x = walkers(case, 8, 7, cuda)
    lp = model.apply(params, x).cpu().numpy()
    lp_ref = ref(None, x.cpu()).numpy()
    err_re = np.abs(lp.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real))
    err_im = phase_err(lp.imag, lp_ref.imag)
    print(f"{case_id(case)}: log psi re {err_re.max():.1e} phase {err_im.max():.1e}")
    assert err_re.max() < 1e-6
    assert err_im.max() < 1e-5
    e, o = hamiltonian.local_energy(model, system)(params, x)
    # the same walkers as float64: torch.func returns derivatives in the dtype of its input, and the
    # terms of a pair 1e-3 rad apart (1 / w^2 = 4e6) cancel to KE = N/2 only in double
    e_ref, o_ref = hamiltonian.local_energy(ref, system)(ref.init(), x.double())
    geo = geo_scale(x, case["flux"])
    scale = lambda v: np.maximum(np.maximum(1.0, np.abs(v)), geo)  # noqa: E731
    errs = {"E_L": np.max(np.abs(e.cpu().numpy() - e_ref.cpu().numpy()) / scale(e_ref.cpu().numpy()))}
    for k in KEYS:
        r = o_ref[k].cpu().numpy()
        errs[k] = np.max(np.abs(o[k].cpu().numpy() - r) / scale(r))
    print(f"{case_id(case)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-5, k


@pytest.mark.parametrize("nspins,expo,flux,B", [((2, 2), (3, 3, 1), 5, 4096), ((3, 3), (3, 3, 2), 12, 1024)])
def test_singlet_analytic_pins(cuda, nspins, expo, flux, B):
    """KE = N/2, Im KE = 0, L^2 = 0, Lz = Lz^2 = 0 on every walker."""
    case = dict(nspins=nspins, exponents=expo, flux=flux)
    system, model, _ = build(case)
    N = sum(nspins)
    x = walkers(case, B, 3, cuda)
    e, o = hamiltonian.local_energy(model, system)(model.init(0, device=cuda), x)
    geo = geo_scale(x, flux)
    for k, want in (("kinetic", N / 2), ("angular_momentum_square", 0.0), ("angular_momentum_z", 0.0),
                    ("angular_momentum_z_square", 0.0)):
        err = np.max(np.abs(o[k].real.cpu().numpy() - want) / geo)
        print(f"{nspins} {expo} {k}: {err:.1e}")
        assert err < 1e-5, (k, err)
    assert np.max(np.abs(o["kinetic"].imag.cpu().numpy()) / geo) < 1e-5
    assert torch.isfinite(e.real).all()


# N = 4 and 6: 16 walkers per value workgroup; N = 10: 8; N = 20: 4
@pytest.mark.parametrize("case", [CASES[1], CASES[2], dict(nspins=(5, 5), exponents=(1, 1, 1), flux=9),
                                  dict(nspins=(10, 10), exponents=(1, 1, 1), flux=19)], ids=case_id)
def test_entry_points_agree_bit_for_bit(cuda, case):
    """dh_logpsi equals the log psi dh_local_energy reports, bit for bit; two calls give the same
    bits; B = 1 and B = 257 (a partial last workgroup of the value kernel) are the same walkers'
    values inside a larger batch."""
    system, model, _ = build(case)
    params = model.init(0, device=cuda)
    x = walkers(case, 600, 21, cuda)
    lp = torch.view_as_real(model.apply(params, x))
    assert torch.isfinite(lp).all()
    assert torch.equal(bits(lp), bits(torch.view_as_real(model.apply(params, x))))
    e, obs = hamiltonian.local_energy(model, system).raw(params, x)
    assert torch.equal(bits(obs[:, 6:8]), bits(lp))
    e2, obs2 = hamiltonian.local_energy(model, system).raw(params, x)
    assert torch.equal(bits(e), bits(e2)) and torch.equal(bits(obs), bits(obs2))
    for lo, hi in ((0, 1), (599, 600), (0, 257), (343, 600), (5, 22)):
        part = x[lo:hi].contiguous()
        assert torch.equal(bits(torch.view_as_real(model.apply(params, part))), bits(lp[lo:hi])), (lo, hi)
    e1, obs1 = hamiltonian.local_energy(model, system).raw(params, x[599:600].contiguous())
    assert torch.equal(bits(e1), bits(e[599:600])) and torch.equal(bits(obs1), bits(obs[599:600]))


def _laughlin(nspins, flux, system=None):
    net = config.Network()
    net.type = config.NetworkType.laughlin
    la = make_network(system or config.System(nspins=nspins, flux=flux), net)
    assert type(la) is Laughlin
    return la


def test_equal_exponents_vs_laughlin_kernel(cuda):
    """(3,3,3) at nspins (2,1), flux 6 against laughlin.hip on the same walkers: Re log psi, and the
    phase up to one constant multiple of pi."""
    case = dict(nspins=(2, 1), exponents=(3, 3, 3), flux=6)
    system, model, _ = build(case)
    la = _laughlin((2, 1), 6, system)
    x = walkers(case, 512, 5, cuda)
    lph = model.apply(model.init(0, device=cuda), x).cpu().numpy()
    lpl = la.apply(la.init(0, device=cuda), x).cpu().numpy()
    assert np.max(np.abs(lph.real - lpl.real) / np.maximum(1, np.abs(lpl.real))) < 1e-6
    d = lph.imag - lpl.imag
    k = np.round(d[0] / np.pi)
    assert abs(d[0] - k * np.pi) < 1e-5
    assert np.max(phase_err(lph.imag, lpl.imag + k * np.pi)) < 1e-5
    eh, oh = hamiltonian.local_energy(model, system)(model.init(0, device=cuda), x)
    el, ol = hamiltonian.local_energy(la, system)(la.init(0, device=cuda), x)
    geo = geo_scale(x, 6)
    for key in KEYS:
        a, r = oh[key].cpu().numpy(), ol[key].cpu().numpy()
        assert np.max(np.abs(a - r) / np.maximum(np.maximum(1.0, np.abs(r)), geo)) < 1e-5, key


def test_no_interspecies_exponent_vs_two_laughlin_kernels(cuda):
    """(3,3,0) at (2,2), flux 3 against two (2,0) Laughlin handles on the halves."""
    case = dict(nspins=(2, 2), exponents=(3, 3, 0), flux=3)
    system, model, _ = build(case)
    la = _laughlin((2, 0), 3)
    x = walkers(case, 512, 6, cuda)
    lph = model.apply(model.init(0, device=cuda), x).cpu().numpy()
    p = la.init(0, device=cuda)
    lpl = (la.apply(p, x[:, :2].contiguous()) + la.apply(p, x[:, 2:].contiguous())).cpu().numpy()
    assert np.max(np.abs(lph.real - lpl.real) / np.maximum(1, np.abs(lpl.real))) < 1e-6
    d = lph.imag - lpl.imag
    k = np.round(d[0] / np.pi)
    assert abs(d[0] - k * np.pi) < 1e-5
    assert np.max(phase_err(lph.imag, lpl.imag + k * np.pi)) < 1e-5


def test_halperin_mcmc(cuda):
    """10 moves on 512 walkers at (3,3)(3,3,2): some but not all accepted, the walkers finite and
    on the sphere, and the same bits from the same seed."""
    from deephall_amd.mcmc import make_mcmc_step
    from deephall_amd.random import PRNGKey

    case = CASES[2]
    system, model, ref = build(case)
    params = model.init(0, device=cuda)
    x0 = walkers(case, 512, 9, cuda).contiguous()
    step = make_mcmc_step(model, batch_per_device=512, steps=10)
    x, _ = step(params, x0.clone(), PRNGKey(2), 0.3)
    nacc = step.last_n_accept.clone()
    total = int(nacc.sum().item())
    assert 0 < total < 10 * 512, total
    assert int(nacc.min().item()) >= 0 and int(nacc.max().item()) <= 10
    assert torch.isfinite(x).all()
    assert (x[..., 0] >= 0).all() and (x[..., 0] <= np.pi).all()
    assert not torch.equal(x, x0)
    xb, _ = step(params, x0.clone(), PRNGKey(2), 0.3)
    assert torch.equal(bits(xb), bits(x)) and torch.equal(step.last_n_accept, nacc)
    lp = model.apply(params, x).cpu().numpy()
    lp_ref = ref(None, x.cpu()).numpy()
    assert np.max(np.abs(lp.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real))) < 1e-6
    assert np.max(phase_err(lp.imag, lp_ref.imag)) < 1e-5


def test_halperin_driver(cuda, tmp_path):
    """train with network.type halperin and optimizer none: MCMC and statistics on halperin.hip;
    every iteration logs L^2 = 0 and KE = N/2 = 3 (an exact lowest-Landau-level singlet)."""
    cfg = Config.from_dict({
        "seed": 42,
        "batch_size": 1024,
        "system": {"nspins": (3, 3), "flux": 12},
        "network": {"type": "halperin"},
        "mcmc": {"burn_in": 50},
        "optim": {"iterations": 20, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    with open(tmp_path / "train_stats.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 20
    e = np.array([float(r["energy"]) for r in rows])
    print("Halperin (3,3,2) N=6 2Q=12 energy: mean", e.mean(), "min", e.min(), "max", e.max())
    assert np.isfinite(e).all()
    for r in rows:  # the log's own digits: kinetic 3.000, L_square +-0.0000
        assert f"{float(r['kinetic']):.3f}" == "3.000", r
        assert r["L_square"] in ("0.0000", "-0.0000"), r


class _Adaptor:
    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg

    def call_network(self, params, x, system=None):
        return self.model.apply(params, x)


def test_overlap_reference(cuda):
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import overlap

    cfg = Config.from_dict({"system": {"nspins": (3, 3), "flux": 12}, "network": {"type": "halperin"}})
    model = make_network(cfg.system, cfg.network)
    est = overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([3, 3], flux=12), {"reference": "halperin"}, {})
    assert isinstance(est.laughlin, Halperin) and est.laughlin.exponents == (3, 3, 2)
    values, state = est.empty_val_state(3)
    x = torch.tensor(make_walkers(512, 6, seed=2), device=cuda)
    for i in range(3):
        v, state = est.evaluate(i, {}, None, x, None, state, None)
        values["ratio"][i] = v["ratio"].mean()
        values["ratio_square"][i] = v["ratio_square"].mean()
    assert abs(est.digest(values, state)["overlap"].item() - 1.0) < 1e-5
    with pytest.raises(ValueError, match="reference must be"):
        overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([3, 3], flux=12), {"reference": "halperrin"}, {})
