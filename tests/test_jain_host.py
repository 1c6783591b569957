"""Jain composite-fermion states with two Lambda levels (networks/jain.py) on the host, float64.

`JainCallable` is the state's independent route (slogdet of the explicit columns).  Here it is
pinned by what the state must satisfy: it carries Lz = sum of the occupied m, it is
antisymmetric, the ground state with both levels filled is a lowest-Landau-level singlet
(KE = N/2, L^2 = Lz = 0 on every walker, through the reference's kinetic-energy restatement
with torch.func derivatives), a single exciton keeps KE = N/2 with Lz = 1, and with one
second-level orbital on top of a filled level 0 it is the Laughlin quasiparticle.  The native
library's validation (dh_create with DH_NETWORK_JAIN, dh_create_cf) runs without a GPU.
The kernel itself is tested in test_gpu_jain.py."""

from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from deephall_amd import Config, _lib, config, make_network
from deephall_amd.networks import Jain, JainCallable, LaughlinQuasiparticle
from deephall_amd.networks.psiformer import NetworkSpec
from oracle import reference as R

EXCITON = ((0, -1.5), (0, -0.5), (0, 0.5), (1, 2.5))  # N = 4, 2Q = 9: Q1 = 3/2, Lz = 1
GROUND = [((4, 0), 6, 1), ((6, 0), 11, 1), ((4, 0), 12, 2)]


def _walkers(N, seed, cmax=1.0):
    g = torch.Generator().manual_seed(seed)
    th = torch.arccos((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * cmax)
    ph = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    return torch.stack([th, ph], -1)


@pytest.mark.parametrize("nspins,flux,p,occ,lz", [((4, 0), 6, 1, None, 0.0), ((6, 0), 11, 1, None, 0.0),
                                                  ((4, 0), 12, 2, None, 0.0), ((4, 0), 9, 1, EXCITON, 1.0),
                                                  ((3, 1), 9, 1, ((1, -2.5), (0, 1.5), (1, 0.5), (0, -0.5)), -1.0)])
def test_lz_phase(nspins, flux, p, occ, lz):
    """A rotation of every phi by a multiplies psi by exp(i Lz a), Lz = the sum of the occupied m."""
    m = JainCallable(nspins, flux, cf_flux=p, occupation=occ)
    assert sum(mm for _, mm in m.occupation) == lz
    for seed in range(3):
        x = _walkers(sum(nspins), seed)
        a = 0.37
        xr = x.clone()
        xr[:, 1] += a
        d = m(None, xr) - m(None, x)
        assert abs(d.real.item()) < 1e-10
        assert abs(math.remainder(d.imag.item() - lz * a, 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,flux,p,occ", [((6, 0), 11, 1, None), ((4, 0), 12, 2, None), ((4, 0), 9, 1, EXCITON)])
def test_permutation_antisymmetry(nspins, flux, p, occ):
    m = JainCallable(nspins, flux, cf_flux=p, occupation=occ)
    x = _walkers(sum(nspins), 11)
    perm = list(range(sum(nspins)))
    perm[0], perm[2] = perm[2], perm[0]
    d = m(None, x[perm]) - m(None, x)
    assert abs(d.real.item()) < 1e-10 and abs(math.remainder(d.imag.item() - math.pi, 2 * math.pi)) < 1e-10


def _kinetic(m, nspins, flux, xs):
    ocfg = R.LaughlinConfig(nspins=nspins, flux=flux)  # Q and the default radius only
    ke = R.make_local_kinetic_energy(lambda params, y: m(None, y), ocfg.Q, ocfg.r)
    return [ke(None, x) for x in xs], ocfg


def _geo(Q, x):
    return (Q**2 * (1 / torch.sin(x[:, 0])).sum() ** 2).item()


@pytest.mark.parametrize("nspins,flux,p", GROUND)
def test_ground_state_is_an_lll_singlet(nspins, flux, p):
    """KE = N/2, Im KE = 0, L^2 = 0 and Lz = 0 on every walker, to 1e-10 relative to
    geo = Q^2 (sum 1/sin theta)^2, the size of the magnetic terms that cancel."""
    N = sum(nspins)
    m = JainCallable(nspins, flux, cf_flux=p)
    xs = [_walkers(N, s, cmax=0.9) for s in range(3)]
    out, ocfg = _kinetic(m, nspins, flux, xs)
    for x, (ke, o) in zip(xs, out):
        scale = max(1.0, _geo(ocfg.Q, x))
        assert abs(complex(ke) - N / 2) / scale < 1e-10
        assert abs(complex(o["angular_momentum_square"])) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z"])) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z_square"])) / scale < 1e-10


def test_exciton_kinetic_and_lz():
    """One composite fermion lifted to the second level: still in the lowest Landau level
    (KE = N/2 = 2) with Lz = Lz^2 = 1; not an L^2 eigenstate, so L^2 is not pinned."""
    m = JainCallable((4, 0), 9, occupation=EXCITON)
    xs = [_walkers(4, s, cmax=0.9) for s in range(3)]
    out, ocfg = _kinetic(m, (4, 0), 9, xs)
    for x, (ke, o) in zip(xs, out):
        scale = max(1.0, _geo(ocfg.Q, x))
        assert abs(complex(ke) - 2.0) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z"]) - 1.0) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z_square"]) - 1.0) / scale < 1e-10


@pytest.mark.parametrize("m1", [-2.0, 0.0, 1.0])
def test_one_second_level_orbital_is_the_laughlin_quasiparticle(m1):
    """N = 4, 2Q = 8 (Q1 = 1): level 0 filled plus (1, m1) has the quasiparticle's columns.  With
    N (N - 1) / 2 = 6 pairs the quasiparticle's Jastrow over ordered pairs (a factor -1 per pair)
    and the 2p sum_{i<k} log w_ik here agree, so log psi is the same number."""
    occ = ((0, -1.0), (0, 0.0), (0, 1.0), (1, m1))
    jain = JainCallable((4, 0), 8, occupation=occ)
    qp = LaughlinQuasiparticle((4, 0), 8, excitation_lz=m1)
    for seed in range(4):
        x = _walkers(4, seed)
        d = jain(None, x) - qp(None, x)
        assert abs(d.real.item()) < 1e-10 * max(1.0, abs(qp(None, x).real.item()))
        assert abs(math.remainder(d.imag.item(), 2 * math.pi)) < 1e-10
    xb = torch.stack([_walkers(4, s) for s in range(3)])
    assert torch.allclose(jain(None, xb), torch.stack([jain(None, x) for x in xb]), rtol=0, atol=1e-12)


def _create(nspins, flux, p=1, occ=None, n_occ=None):
    lib = _lib.load()
    spec = NetworkSpec(nspins=nspins, flux=flux, ndets=1, num_heads=1, heads_dim=4, num_layers=0,
                       network_type="jain", cf_flux=p)
    h = C.c_void_p()
    cfg = spec.to_c()
    if occ is None:
        rc = lib.dh_create(C.byref(cfg), C.byref(h))
    else:
        flat = [int(v) for pair in occ for v in pair]
        rc = lib.dh_create_cf(C.byref(cfg), (C.c_int * len(flat))(*flat), len(occ) if n_occ is None else n_occ,
                              C.byref(h))
    if rc == 0:
        lib.dh_destroy(h)
    return rc, lib.dh_last_error()


def test_native_validation():
    """dh_create (DH_NETWORK_JAIN) and dh_create_cf: (level, 2 m) occupations."""
    for nspins, flux, p in [((4, 0), 6, 1), ((6, 0), 11, 1), ((8, 0), 16, 1), ((10, 0), 21, 1), ((12, 0), 26, 1),
                            ((4, 0), 12, 2), ((3, 3), 11, 1)]:
        assert _create(nspins, flux, p)[0] == 0, (nspins, flux, p)
    exciton2 = [(n, int(2 * m)) for n, m in EXCITON]
    assert _create((4, 0), 9, occ=exciton2)[0] == 0
    assert _create((4, 0), 6, occ=[(0, 0), (1, -2), (1, 0), (1, 2)])[0] == 0  # the default, explicitly
    bad = {
        "no ground state at this filling": _create((6, 0), 12),
        "orbital twice": _create((4, 0), 9, occ=[(0, -3), (0, -1), (0, -1), (1, 5)]),
        "|m| too large": _create((4, 0), 9, occ=[(0, -3), (0, -1), (0, 5), (1, 5)]),
        "|m| too large, level 1": _create((4, 0), 9, occ=[(0, -3), (0, -1), (0, 1), (1, 7)]),
        "wrong parity": _create((4, 0), 9, occ=[(0, -3), (0, -1), (0, 1), (1, 4)]),
        "n_occ != N": _create((4, 0), 9, occ=exciton2[:3]),
        "level 2": _create((4, 0), 9, occ=[(0, -3), (0, -1), (0, 1), (2, 5)]),
        "Q1 < 0": _create((4, 0), 4),
        "LDS": _create((16, 0), 36),  # Q1 = 3: the energy kernel would need more than 160 KiB
        "LDS, N = 14": _create((14, 0), 31),
    }
    for why, (rc, msg) in bad.items():
        assert rc != 0, why
        assert b"Jain" in msg, (why, msg)
    assert b"LDS" in bad["LDS"][1]


def test_python_validation_and_selection():
    net = config.Network()
    net.type = config.NetworkType.jain
    model = make_network(config.System(nspins=(6, 0), flux=11), net)
    assert isinstance(model, Jain) and model.spec.network_type == "jain" and model.spec.occupation is None
    assert model.occupation == ((0, -0.5), (0, 0.5), (1, -1.5), (1, -0.5), (1, 0.5), (1, 1.5))
    assert model.init(device="cpu") == {}
    net.jain.occupation = EXCITON
    model = make_network(config.System(nspins=(4, 0), flux=9), net)
    assert model.spec.occupation == ((0, -3), (0, -1), (0, 1), (1, 5))
    hash(model.spec)
    with pytest.raises(ValueError):
        Jain((6, 0), 12)
    with pytest.raises(ValueError):
        JainCallable((4, 0), 9, occupation=EXCITON[:3])
    with pytest.raises(ValueError):
        JainCallable((4, 0), 9, occupation=((0, -1.5), (0, -0.5), (0, 0.5), (1, 2.0)))
    with pytest.raises(ValueError):
        JainCallable((4, 0), 9, occupation=((0, -1.5), (0, -0.5), (0, -0.5), (1, 2.5)))
    with pytest.raises(TypeError):
        model.vjp()


def test_config_round_trip():
    cfg = Config.from_dict({
        "system": {"nspins": (4, 0), "flux": 9},
        "network": {"type": "jain", "jain": {"cf_flux": 1, "occupation": [[0, -1.5], [0, -0.5], [0, 0.5], [1, 2.5]]}},
    })
    assert cfg.network.jain.occupation == EXCITON and cfg.network.jain.cf_flux == 1
    model = make_network(cfg.system, cfg.network)
    assert isinstance(model, Jain) and model.occupation == EXCITON
    import dataclasses

    again = Config.from_dict(dataclasses.asdict(cfg))
    assert again.network.jain == cfg.network.jain
    assert Config.from_dict({"network": {"type": "jain", "jain": {"cf_flux": 2}}}).network.jain.cf_flux == 2
    assert Config.from_dict({}).network.jain.occupation is None
