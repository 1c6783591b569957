"""Pinned quasiholes (networks/quasihole.py, quasihole.hip) on MI355X.

* The kernel against `QuasiholeCallable`, the float64 torch form pushed through the callable
  boundary (torch.func derivatives, hamiltonian.local_energy(callable, system)): log psi, E_L and
  every observable, on both bases, also with an electron pair 1e-3 rad apart and an electron 1e-3
  rad from a hole.  The kernel works in double and stores f32 as the other analytic kernels do, so
  the tolerances are those of test_gpu_pfaffian.py and test_gpu_jain.py.
* Analytic pins on every walker of 512: KE = N/2 (lowest Landau level), L^2 of one hole on a
  Laughlin base and of a hole that acts on one species, Lz of holes at the poles.
* Cross-kernel: a hole at the north pole against laughlin.hip's quasihole determinant; coincident
  groups of the Pfaffian base against one Abelian hole.
* Permutations, MCMC, the training driver with optimizer none, the overlap estimator's reference.
"""

from __future__ import annotations

import csv
import math

import numpy as np
import pytest
import torch

from deephall_amd import Config, config, hamiltonian, make_network, train
from deephall_amd.networks import Laughlin, Quasihole, QuasiholeCallable
from helpers import make_walkers

pytestmark = pytest.mark.gpu
KEYS = ("kinetic", "potential", "angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square")
G1, G2, G3, G4 = (0.7, 0.3), (1.9, -2.1), (2.6, 1.2), (1.1, 2.8)  # generic points
L0 = (3, 3, 0)  # Laughlin 1/3 on nspins (N, 0)
CASES = [
    dict(nspins=(3, 0), exponents=L0, flux=7, holes=(G1,)),
    dict(nspins=(4, 0), exponents=L0, flux=11, holes=((0.0, 0.0), G2)),   # one hole at exactly theta = 0
    dict(nspins=(2, 2), flux=8, holes=(G1,)),
    dict(nspins=(2, 2), flux=8, holes=(G1, G2), species=("up", "down")),
    dict(nspins=(3, 2), flux=10, holes=(G3,), species=("down",)),
    dict(nspins=(2, 2), flux=8, holes=(G1,), interaction_type="harmonic"),
    dict(nspins=(3, 0), exponents=L0, flux=7, holes=(G1,), radius=2.5),
    dict(nspins=(2, 0), base="pfaffian", flux=2, holes=(G1, G2), pairing=((0,), (1,))),   # no elimination step
    dict(nspins=(4, 0), base="pfaffian", flux=6, holes=(G1, G2), pairing=((0,), (1,))),
    dict(nspins=(4, 0), base="pfaffian", cf_flux=2, flux=12, holes=(G1, G2), pairing=((0,), (1,))),
    dict(nspins=(6, 0), base="pfaffian", flux=11, holes=(G1, G2, G3, G4), pairing=((0, 1), (2, 3))),
    dict(nspins=(6, 0), base="pfaffian", flux=11, holes=(G1, G2, G3), pairing=((0,), (2,))),  # hole 1 Abelian
    dict(nspins=(10, 0), base="pfaffian", flux=19, holes=(G1, G2, G3, G4), pairing=((0, 3), (1, 2))),
]
# an electron pair 1e-3 rad apart in and out of the natural (pivot) order, an electron 1e-3 rad from a hole
CLUSTERED = [
    dict(CASES[10], close=(0, 1)),
    dict(CASES[10], close=(2, 5)),
    dict(CASES[10], on_hole=(3, 0)),   # electron 3 at hole 0 of group A
    dict(CASES[11], on_hole=(4, 1)),   # at the Abelian hole
    dict(CASES[3], close=(0, 2)),      # an up and a down electron
    dict(CASES[3], on_hole=(0, 0)),    # an up electron at the up hole
    dict(CASES[1], on_hole=(2, 1)),
]


def build(case, lz_center=0.0):
    system = config.System(nspins=case["nspins"], flux=case["flux"], radius=case.get("radius"), lz_center=lz_center,
                           interaction_type=config.InteractionType(case.get("interaction_type", "coulomb")))
    net = config.Network()
    net.type = config.NetworkType.quasihole
    net.halperin.exponents = case.get("exponents", (3, 3, 2))
    net.pfaffian.cf_flux = case.get("cf_flux", 1)
    net.quasihole = config.QuasiholeNetwork(base=case.get("base", "halperin"), holes=case["holes"],
                                            species=case.get("species"), pairing=case.get("pairing"))
    model = make_network(system, net)
    assert isinstance(model, Quasihole)
    ref = QuasiholeCallable(case["nspins"], case["flux"], base=case.get("base", "halperin"), holes=case["holes"],
                            species=case.get("species"), pairing=case.get("pairing"),
                            exponents=case.get("exponents", (3, 3, 2)), cf_flux=case.get("cf_flux", 1), system=system)
    return system, model, ref


def walkers(case, B, seed, cuda):
    x = make_walkers(B, sum(case["nspins"]), seed=seed, margin=0.05)
    step = np.float32([6e-4, 8e-4])
    if "close" in case:
        i, k = case["close"]
        x[:, k] = x[:, i] + step
    if "on_hole" in case:
        i, a = case["on_hole"]
        x[:, i] = np.float32(case["holes"][a]) + step
    return torch.tensor(x, device=cuda)


def geo_scale(x, flux):
    """Q^2 (sum 1/sin theta)^2: the size of the magnetic terms that cancel in KE and L^2."""
    st = torch.sin(x[..., 0].double().cpu())
    return np.maximum(1.0, ((flux / 2) ** 2 * (1 / st).sum(-1) ** 2).numpy())


def phase_err(a, b):
    return np.abs(np.angle(np.exp(1j * (a - b))))


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k != "holes") + f"-h{len(c['holes'])}"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def observables(model, system, x):
    e, o = hamiltonian.local_energy(model, system)(model.init(0, device=x.device), x)
    return e.cpu().numpy(), {k: o[k].cpu().numpy() for k in KEYS}


@pytest.mark.parametrize("case", CASES + CLUSTERED, ids=case_id)
def test_quasihole_vs_callable(cuda, case):
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
    e, o = observables(model, system, x)
    # the same walkers as float64: torch.func returns derivatives in the dtype of its input, and the
    # terms of a pair 1e-3 rad apart (1 / w^2 = 4e6) cancel to KE = N/2 only in double
    e_ref, o_ref = hamiltonian.local_energy(ref, system)(ref.init(), x.double())
    geo = geo_scale(x, case["flux"])
    scale = lambda v: np.maximum(np.maximum(1.0, np.abs(v)), geo)  # noqa: E731
    errs = {"E_L": np.max(np.abs(e - e_ref.cpu().numpy()) / scale(e_ref.cpu().numpy()))}
    for k in KEYS:
        r = o_ref[k].cpu().numpy()
        errs[k] = np.max(np.abs(o[k] - r) / scale(r))
    print(f"{case_id(case)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 1e-5, k


def pin(o, key, want, geo, what):
    err = np.max(np.abs(o[key].real - want) / geo)
    print(f"{what} {key}: {err:.1e}")
    assert err < 1e-5, (what, key, err)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lowest_landau_level_pin(cuda, case):
    """KE = N/2 and Im KE = 0 on every walker of 512: every state here is an LLL polynomial.  (N/2 is
    the lowest level's N Q / (2 r^2) at the default radius sqrt(Q); the case with its own radius has
    that value.)"""
    system, model, _ = build(case)
    x = walkers(case, 512, 3, cuda)
    e, o = observables(model, system, x)
    geo = geo_scale(x, case["flux"])
    Q = case["flux"] / 2
    pin(o, "kinetic", sum(case["nspins"]) / 2 * Q / case.get("radius", math.sqrt(Q)) ** 2, geo, case_id(case))
    assert np.max(np.abs(o["kinetic"].imag) / geo) < 1e-5
    assert np.isfinite(e.real).all()


@pytest.mark.parametrize("hole", [G1, (0.0, 0.0)], ids=["generic", "pole"])
@pytest.mark.parametrize("N,flux", [(4, 10), (6, 16)])
def test_one_hole_on_a_laughlin_base(cuda, N, flux, hole):
    """One hole on Laughlin 1/3 is the highest weight of L = N/2 along the hole: L^2 = (N/2)(N/2 + 1)
    anywhere; at theta = 0 also Lz = -N/2 and Lz^2 = N^2/4."""
    case = dict(nspins=(N, 0), exponents=L0, flux=flux, holes=(hole,))
    system, model, _ = build(case)
    x = walkers(case, 512, 4, cuda)
    _, o = observables(model, system, x)
    geo = geo_scale(x, flux)
    pin(o, "angular_momentum_square", (N / 2) * (N / 2 + 1), geo, f"N{N} {hole}")
    if hole[0] == 0.0:
        pin(o, "angular_momentum_z", -N / 2, geo, f"N{N} pole")
        pin(o, "angular_momentum_z_square", N * N / 4, geo, f"N{N} pole")


@pytest.mark.parametrize("nspins,species,want", [((2, 3), "up", 2.0), ((3, 2), "down", 2.0)])
def test_one_species_hole(cuda, nspins, species, want):
    """A hole that acts on one species carries L = n/2 of that species: L^2 = (n/2)(n/2 + 1).  On
    (3,3,2) one up hole needs nspins (2, 3) (up 3 + 6 + 1 = 10 = down 6 + 4): at (2, 2) the two
    species would sit at different fluxes (8 and 7), which the flux rule refuses."""
    case = dict(nspins=nspins, flux=10, holes=(G2,), species=(species,))
    system, model, _ = build(case)
    x = walkers(case, 512, 5, cuda)
    _, o = observables(model, system, x)
    pin(o, "angular_momentum_square", want, geo_scale(x, 10), f"{nspins} {species}")
    pin(o, "kinetic", 2.5, geo_scale(x, 10), f"{nspins} {species}")


@pytest.mark.parametrize("south,want", [(True, 0.0), (False, -3.0)], ids=["north-south", "north-north"])
def test_moore_read_holes_at_the_poles(cuda, south, want):
    """Group A at the north pole: with B at the south pole every term of the numerator is u v
    (Lz = 0); with B at the north pole too every electron carries one v (Lz = -N/2)."""
    case = dict(nspins=(6, 0), base="pfaffian", flux=10, holes=((0.0, 0.0), (math.pi if south else 0.0, 0.0)),
                pairing=((0,), (1,)))
    system, model, _ = build(case)
    x = walkers(case, 512, 6, cuda)
    _, o = observables(model, system, x)
    geo = geo_scale(x, 10)
    pin(o, "angular_momentum_z", want, geo, case_id(case))
    pin(o, "kinetic", 3.0, geo, case_id(case))


@pytest.mark.parametrize("case", [
    dict(nspins=(18, 0), base="pfaffian", flux=34, holes=(G1, G2), pairing=((0,), (1,))),   # 65,696 B of LDS
    dict(nspins=(28, 0), base="pfaffian", flux=55, holes=(G1, G2, G3, G4), pairing=((0, 1), (2, 3))),  # the largest N
    dict(nspins=(32, 0), exponents=L0, flux=94, holes=(G3,)),   # 73,024 B
], ids=case_id)
def test_energy_kernel_above_64_kib_of_lds(cuda, case):
    """From N = 18 (pfaffian base) and N = 31 (halperin base) the energy kernel needs more than 64 KiB of
    LDS and the launch raises the kernel's limit first: log psi against the callable on 8 walkers,
    KE = N/2 on 64, and the two entry points' log psi bit for bit."""
    system, model, ref = build(case)
    params = model.init(0, device=cuda)
    x = walkers(case, 64, 13, cuda)
    lp = model.apply(params, x)
    lp_ref = ref(None, x[:8].cpu()).numpy()
    lpn = lp[:8].cpu().numpy()
    assert np.max(np.abs(lpn.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real))) < 1e-6
    assert np.max(phase_err(lpn.imag, lp_ref.imag)) < 1e-5
    _, obs = hamiltonian.local_energy(model, system).raw(params, x)
    assert torch.equal(bits(obs[:, 6:8]), bits(torch.view_as_real(lp)))
    _, o = observables(model, system, x)
    pin(o, "kinetic", sum(case["nspins"]) / 2, geo_scale(x, case["flux"]), case_id(case))


def close(a, r, geo, key):
    assert np.max(np.abs(a - r) / np.maximum(np.maximum(1.0, np.abs(r)), geo)) < 1e-5, key


@pytest.mark.parametrize("N,flux", [(4, 10), (6, 16)])
def test_pole_hole_vs_laughlin_kernel(cuda, N, flux):
    """A hole at theta = 0 on Laughlin 1/3 against laughlin.hip's quasihole (excitation_lz = -N/2,
    the orbital m = +Q1 dropped) on 512 walkers: log psi up to the constant of walker 0, E_L and every
    observable."""
    case = dict(nspins=(N, 0), exponents=L0, flux=flux, holes=((0.0, 0.0),))
    system, model, _ = build(case, lz_center=-N / 2)
    net = config.Network()
    net.type = config.NetworkType.laughlin
    la = make_network(system, net)
    assert type(la) is Laughlin and la.excitation_lz == -N / 2
    x = walkers(case, 512, 5, cuda)
    lpq = model.apply(model.init(0, device=cuda), x).cpu().numpy()
    lpl = la.apply(la.init(0, device=cuda), x).cpu().numpy()
    d = lpq - lpl
    assert np.max(np.abs(d.real - d.real[0]) / np.maximum(1, np.abs(lpl.real))) < 1e-6
    assert np.max(phase_err(d.imag, d.imag[0])) < 1e-5
    eq, oq = observables(model, system, x)
    el, ol = observables(la, system, x)
    geo = geo_scale(x, flux)
    close(eq, el, geo, "E_L")
    for key in KEYS:
        close(oq[key], ol[key], geo, key)


def test_coincident_groups_vs_abelian_hole(cuda):
    """A = {a}, B = {b} at one point against one Abelian hole there, both on this kernel: Re log psi
    differs by (N/2) log 2, the phase and every observable are equal."""
    N = 6
    pair = dict(nspins=(N, 0), base="pfaffian", flux=10, holes=(G2, G2), pairing=((0,), (1,)))
    abel = dict(nspins=(N, 0), base="pfaffian", flux=10, holes=(G2,))
    system, mp, _ = build(pair)
    _, ma, _ = build(abel)
    x = walkers(pair, 512, 8, cuda)
    lpp = mp.apply(mp.init(0, device=cuda), x).cpu().numpy()
    lpa = ma.apply(ma.init(0, device=cuda), x).cpu().numpy()
    assert np.max(np.abs(lpp.real - lpa.real - (N / 2) * math.log(2)) / np.maximum(1, np.abs(lpa.real))) < 1e-6
    assert np.max(phase_err(lpp.imag, lpa.imag)) < 1e-5
    ep, op = observables(mp, system, x)
    ea, oa = observables(ma, system, x)
    geo = geo_scale(x, 10)
    close(ep, ea, geo, "E_L")
    for key in KEYS:
        close(op[key], oa[key], geo, key)


def test_permutations_with_four_holes(cuda):
    """Permutations of 8 electrons with 4 holes: Re log psi unchanged, the phase moves by pi x parity."""
    case = dict(nspins=(8, 0), base="pfaffian", flux=15, holes=(G1, G2, G3, G4), pairing=((0, 2), (1, 3)))
    _, model, _ = build(case)
    params = model.init(0, device=cuda)
    x = walkers(case, 64, 12, cuda)
    lp = model.apply(params, x).cpu().numpy()
    rng = np.random.default_rng(0)
    perms = [[1, 0, 2, 3, 4, 5, 6, 7], [7, 1, 2, 3, 4, 5, 6, 0], [1, 2, 0, 3, 4, 5, 6, 7]] + \
            [list(rng.permutation(8)) for _ in range(5)]
    for perm in perms:
        parity = sum(perm[i] > perm[k] for i in range(8) for k in range(i + 1, 8)) % 2
        lpp = model.apply(params, x[:, perm].contiguous()).cpu().numpy()
        assert np.max(np.abs(lpp.real - lp.real) / np.maximum(1, np.abs(lp.real))) < 1e-6, perm
        assert np.max(phase_err(lpp.imag, lp.imag + math.pi * parity)) < 1e-5, perm


@pytest.mark.parametrize("case", [CASES[10], dict(nspins=(6, 0), exponents=L0, flux=16, holes=(G3,)),
                                  dict(nspins=(3, 3), flux=14, holes=(G1, G2))], ids=case_id)
def test_quasihole_mcmc_and_entry_points(cuda, case):
    """Five moves on 512 walkers at N = 6: acceptance in (0.05, 1], the walkers finite and on the
    sphere; dh_logpsi equals the log psi dh_local_energy reports, bit for bit."""
    from deephall_amd.mcmc import make_mcmc_step
    from deephall_amd.random import PRNGKey

    system, model, ref = build(case)
    params = model.init(0, device=cuda)
    x0 = walkers(case, 512, 9, cuda).contiguous()
    step = make_mcmc_step(model, batch_per_device=512, steps=5)
    x, pmove = step(params, x0.clone(), PRNGKey(2), 0.3)
    assert 0.05 < float(pmove) <= 1.0, float(pmove)
    nacc = step.last_n_accept
    assert int(nacc.min().item()) >= 0 and int(nacc.max().item()) <= 5
    assert torch.isfinite(x).all()
    assert (x[..., 0] >= 0).all() and (x[..., 0] <= np.pi).all()
    assert not torch.equal(x, x0)
    lp = torch.view_as_real(model.apply(params, x))
    assert torch.isfinite(lp).all()
    _, obs = hamiltonian.local_energy(model, system).raw(params, x)
    assert torch.equal(bits(obs[:, 6:8]), bits(lp))
    lp_ref = ref(None, x.cpu()).numpy()
    lpn = model.apply(params, x).cpu().numpy()
    assert np.max(np.abs(lpn.real - lp_ref.real) / np.maximum(1, np.abs(lp_ref.real))) < 1e-6
    assert np.max(phase_err(lpn.imag, lp_ref.imag)) < 1e-5


def test_quasihole_driver(cuda, tmp_path):
    """train with network.type quasihole and optimizer none: MCMC and statistics on quasihole.hip;
    every iteration logs KE = N/2 = 3 and L^2 = 3 x 4 = 12 (one hole on Laughlin 1/3, N = 6)."""
    cfg = Config.from_dict({
        "seed": 42,
        "batch_size": 1024,
        "system": {"nspins": (6, 0), "flux": 16},
        "network": {"type": "quasihole", "halperin": {"exponents": [3, 3, 0]},
                    "quasihole": {"holes": [[1.1, 2.8]]}},
        "mcmc": {"burn_in": 50},
        "optim": {"iterations": 20, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    with open(tmp_path / "train_stats.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 20
    e = np.array([float(r["energy"]) for r in rows])
    print("quasihole N=6 2Q=16 energy: mean", e.mean(), "min", e.min(), "max", e.max())
    assert np.isfinite(e).all()
    for r in rows:
        assert abs(float(r["kinetic"]) - 3.0) < 1e-3, r
        assert abs(float(r["L_square"]) - 12.0) < 1e-3, r


class _Adaptor:
    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg

    def call_network(self, params, x, system=None):
        return self.model.apply(params, x)


def test_overlap_reference(cuda):
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import overlap

    cfg = Config.from_dict({"system": {"nspins": (6, 0), "flux": 11},
                            "network": {"type": "quasihole",
                                        "quasihole": {"base": "pfaffian", "holes": [list(G1), list(G2), list(G3), list(G4)],
                                                      "pairing": [[0, 1], [2, 3]]}}})
    model = make_network(cfg.system, cfg.network)
    est = overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([6, 0], flux=11), {"reference": "quasihole"}, {})
    assert isinstance(est.laughlin, Quasihole) and est.laughlin.state == model.state
    values, state = est.empty_val_state(3)
    x = torch.tensor(make_walkers(512, 6, seed=2), device=cuda)
    for i in range(3):
        v, state = est.evaluate(i, {}, None, x, None, state, None)
        values["ratio"][i] = v["ratio"].mean()
        values["ratio_square"][i] = v["ratio_square"].mean()
    assert abs(est.digest(values, state)["overlap"].item() - 1.0) < 1e-5
    default = overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([6, 0], flux=11), {}, {})
    assert type(default.laughlin) is Laughlin  # the default reference is unchanged
    with pytest.raises(ValueError, match="reference must be"):
        overlap.OverlapEstimator(_Adaptor(model, cfg), HallSystem([6, 0], flux=11), {"reference": "quasiholes"}, {})
