"""The Moore-Read Pfaffian state (networks/pfaffian.py) on the host, float64.

`MooreReadCallable` is the state's independent route (an out-of-place skew elimination in torch
operations).  Here it is pinned by what the state must satisfy: its Pfaffian is the explicit
expansion over perfect matchings and squares to the determinant, clustered walkers included; it
carries Lz = 0, is antisymmetric, is a lowest-Landau-level singlet (KE = N/2, L^2 = Lz = 0 on every
walker, through the reference's kinetic-energy restatement with torch.func derivatives), and at
N = 2, p = 2 it is the Laughlin state w^3.  The native library's validation (dh_create with
DH_NETWORK_PFAFFIAN) runs without a GPU.  The kernel itself is tested in test_gpu_pfaffian.py."""

from __future__ import annotations

import ctypes as C
import dataclasses
import math

import pytest
import torch

from deephall_amd import Config, _lib, config, make_network
from deephall_amd.networks import MooreRead, MooreReadCallable
from deephall_amd.networks.pfaffian import log_pfaffian
from deephall_amd.networks.psiformer import NetworkSpec
from oracle import reference as R

VALID = [((2, 0), 1, 1), ((4, 0), 5, 1), ((6, 0), 9, 1), ((8, 0), 13, 1), ((12, 0), 21, 1), ((16, 0), 29, 1),
         ((4, 0), 11, 2), ((3, 3), 9, 1)]
SINGLETS = [((4, 0), 5, 1), ((6, 0), 9, 1), ((8, 0), 13, 1), ((4, 0), 11, 2)]


def _walkers(N, seed, cmax=1.0):
    g = torch.Generator().manual_seed(seed)
    th = torch.arccos((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * cmax)
    ph = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    return torch.stack([th, ph], -1)


def _clustered(N, seed, pair):
    """Electron pair[1] 1e-3 rad from electron pair[0]: one entry of A is about 2e3."""
    x = _walkers(N, seed, cmax=0.9)
    x[pair[1]] = x[pair[0]] + torch.tensor([6e-4, 8e-4], dtype=torch.float64)
    return x


def _expand(A):
    """Pf A by the expansion along the first row: 3 terms at n = 4, 15 at n = 6."""
    n = A.shape[0]
    if n == 2:
        return A[0, 1]
    total = 0
    for j in range(1, n):
        keep = [i for i in range(1, n) if i != j]
        total = total + (-1) ** (j - 1) * A[0, j] * _expand(A[keep][:, keep])
    return total


@pytest.mark.parametrize("N", [4, 6])
def test_pfaffian_is_the_explicit_expansion(N):
    xs = [_walkers(N, s) for s in range(4)] + [_clustered(N, 5, (0, 1)), _clustered(N, 6, (2, 3))]
    for x in xs:
        A, _ = MooreReadCallable.pair_matrix(x)
        pf = torch.exp(log_pfaffian(A))
        want = _expand(A)
        if N == 4:
            want4 = A[0, 1] * A[2, 3] - A[0, 2] * A[1, 3] + A[0, 3] * A[1, 2]
            assert abs(want - want4) <= 1e-14 * abs(want4)
            want = want4
        assert abs(pf - want) <= 1e-12 * abs(want)
        det = torch.linalg.det(A)
        assert abs(pf * pf - det) <= 1e-12 * abs(det)


@pytest.mark.parametrize("nspins,flux,p", [((4, 0), 5, 1), ((6, 0), 9, 1), ((3, 3), 9, 1), ((4, 0), 11, 2), ((10, 0), 17, 1)])
def test_lz_phase(nspins, flux, p):
    """Lz = 0: a rotation of every phi by a leaves psi unchanged."""
    m = MooreReadCallable(nspins, flux, cf_flux=p)
    for seed in range(3):
        x = _walkers(sum(nspins), seed)
        xr = x.clone()
        xr[:, 1] += 0.37
        d = m(None, xr) - m(None, x)
        assert abs(d.real.item()) < 1e-10
        assert abs(math.remainder(d.imag.item(), 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,flux,p", [((2, 0), 1, 1), ((6, 0), 9, 1), ((4, 0), 11, 2), ((8, 0), 13, 1)])
def test_permutation_antisymmetry(nspins, flux, p):
    m = MooreReadCallable(nspins, flux, cf_flux=p)
    N = sum(nspins)
    x = _walkers(N, 11)
    for i, k in ((0, 1), (0, N - 1), (N // 2, N // 2 - 1)):
        perm = list(range(N))
        perm[i], perm[k] = perm[k], perm[i]
        d = m(None, x[perm]) - m(None, x)
        assert abs(d.real.item()) < 1e-10 and abs(math.remainder(d.imag.item() - math.pi, 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,flux,p", SINGLETS)
def test_state_is_an_lll_singlet(nspins, flux, p):
    """KE = N/2, Im KE = 0, L^2 = 0 and Lz = Lz^2 = 0 on every walker, to 1e-10 relative to
    max(1, geo), geo = Q^2 (sum 1/sin theta)^2, the size of the magnetic terms that cancel."""
    N = sum(nspins)
    m = MooreReadCallable(nspins, flux, cf_flux=p)
    ocfg = R.LaughlinConfig(nspins=nspins, flux=flux)  # Q and the default radius only
    ke = R.make_local_kinetic_energy(lambda params, y: m(None, y), ocfg.Q, ocfg.r)
    for seed in range(3):
        x = _walkers(N, seed, cmax=0.9)
        kin, o = ke(None, x)
        scale = max(1.0, (ocfg.Q**2 * (1 / torch.sin(x[:, 0])).sum() ** 2).item())
        assert abs(complex(kin) - N / 2) / scale < 1e-10
        assert abs(complex(kin).imag) / scale < 1e-10
        assert abs(complex(o["angular_momentum_square"])) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z"])) / scale < 1e-10
        assert abs(complex(o["angular_momentum_z_square"])) / scale < 1e-10


def test_two_electrons_are_the_laughlin_state():
    """N = 2, p = 2, 2Q = 3: Pf = 1 / w and the pair part w^4, so psi = w^3, the Laughlin state at
    filling 1/3 (its determinant is -w and its Jastrow over ordered pairs -w^2)."""
    m = MooreReadCallable((2, 0), 3, cf_flux=2)
    ocfg = R.LaughlinConfig(nspins=(2, 0), flux=3)
    for seed in range(6):
        x = _walkers(2, seed)
        d = m(None, x) - R.laughlin_logpsi(ocfg, x)
        assert abs(d.real.item()) < 1e-10
        assert abs(math.remainder(d.imag.item(), 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,flux,p", [((2, 0), 1, 1), ((6, 0), 9, 1), ((4, 0), 11, 2), ((3, 3), 9, 1)])
def test_batched_equals_per_walker(nspins, flux, p):
    m = MooreReadCallable(nspins, flux, cf_flux=p)
    N = sum(nspins)
    xb = torch.stack([_walkers(N, s) for s in range(4)] + ([_clustered(N, 9, (2, 3))] if N >= 4 else []))
    one = torch.stack([m(None, x) for x in xb])
    assert one.dtype == torch.complex128
    assert torch.allclose(m(None, xb), one, rtol=0, atol=1e-12)
    xf = xb.float()  # float32 walkers are promoted, not computed in float32
    assert torch.allclose(m(None, xf), m(None, xf.double()), rtol=0, atol=1e-12)


def _create(nspins, flux, p=1):
    lib = _lib.load()
    spec = NetworkSpec(nspins=nspins, flux=flux, ndets=1, num_heads=1, heads_dim=4, num_layers=0,
                       network_type="pfaffian", cf_flux=p)
    h = C.c_void_p()
    cfg = spec.to_c()
    assert cfg.network_type == 3 and C.sizeof(cfg) == 60
    rc = lib.dh_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        assert lib.dh_set_params(h, None, 0, None) == 0  # no parameters: count 0 is accepted
        lib.dh_destroy(h)
    return rc, lib.dh_last_error()


def test_native_validation():
    """dh_create (DH_NETWORK_PFAFFIAN): N even at flux 2 p (N - 1) - 1, within the LDS budget."""
    for nspins, flux, p in VALID + [((28, 0), 53, 1)]:
        assert _create(nspins, flux, p)[0] == 0, (nspins, flux, p)
    bad = {
        "odd N": _create((5, 0), 7),
        "odd N, two spins": _create((2, 1), 3),
        "N = 0": _create((0, 0), 1),
        "flux too large": _create((6, 0), 10),
        "flux too small": _create((6, 0), 8),
        "the flux of another p": _create((4, 0), 11, 1),
        "p = 0": _create((4, 0), 5, 0),
        "flux > 126": _create((10, 0), 143, 8),
        "LDS": _create((30, 0), 57),
        "LDS, N = 32": _create((32, 0), 61),
    }
    for why, (rc, msg) in bad.items():
        assert rc == -1, why  # DH_EINVAL
        assert b"Pfaffian" in msg, (why, msg)
    assert b"LDS" in bad["LDS"][1] and b"166624" in bad["LDS"][1]  # 16 (11 N^2 + 17 N + 4)
    assert b"LDS" in bad["LDS, N = 32"][1]


def test_python_validation_and_selection():
    net = config.Network()
    net.type = config.NetworkType.pfaffian
    model = make_network(config.System(nspins=(6, 0), flux=9), net)
    assert isinstance(model, MooreRead) and model.spec.network_type == "pfaffian" and model.spec.cf_flux == 1
    assert model.spec.to_c().network_type == 3
    assert model.init(device="cpu") == {}
    hash(model.spec)
    net.pfaffian.cf_flux = 2
    model = make_network(config.System(nspins=(2, 2), flux=11), net)
    assert model.cf_flux == 2 and model.nspins == (2, 2)
    with pytest.raises(TypeError):
        model.vjp()
    for cls in (MooreRead, MooreReadCallable):
        for nspins, flux, p in [((5, 0), 7, 1), ((6, 0), 10, 1), ((6, 0), 8, 1), ((4, 0), 5, 0), ((4, 0), 5, 2), ((0, 0), 1, 1)]:
            with pytest.raises(ValueError):
                cls(nspins, flux, cf_flux=p)
    with pytest.raises(ValueError):
        make_network(config.System(nspins=(6, 0), flux=11), net)


def test_config_round_trip():
    cfg = Config.from_dict({
        "system": {"nspins": (4, 0), "flux": 11},
        "network": {"type": "pfaffian", "pfaffian": {"cf_flux": 2}},
    })
    assert cfg.network.type == config.NetworkType.pfaffian and cfg.network.pfaffian.cf_flux == 2
    model = make_network(cfg.system, cfg.network)
    assert isinstance(model, MooreRead) and model.cf_flux == 2
    again = Config.from_dict(dataclasses.asdict(cfg))
    assert again.network.pfaffian == cfg.network.pfaffian and again.network.type == cfg.network.type
    assert Config.from_dict({}).network.pfaffian.cf_flux == 1
    assert Config.from_dict({"network": {"type": "pfaffian"}}).network.pfaffian.cf_flux == 1
