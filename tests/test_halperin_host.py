"""Halperin (m_up, m_dn, n) states (networks/halperin.py) and the total-spin estimator's
restatement (tests/spin_ref.py) on the host, float64.

`HalperinCallable` is the state's independent route.  Here it is pinned by what the state must
satisfy: a lowest-Landau-level rotational singlet (KE = N/2, L^2 = Lz = Lz^2 = 0 on every walker,
through the reference's kinetic-energy restatement with torch.func derivatives), antisymmetric
inside a species, the Laughlin state at (m, m, m) and two Laughlin states at (m, m, 0).  The
native library's validation (dh_create_halperin) runs without a GPU, as do the config, the
network selection and the estimator registry.  S^2_loc of the restatement on the callable gives
S (S + 1) on every walker of the total-spin eigenstates.  The kernels themselves are tested in
test_gpu_halperin.py and test_gpu_spin_square.py."""

from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import spin_ref as SR
from deephall_amd import Config, _lib, config, make_network
from deephall_amd.networks import Halperin, HalperinCallable
from deephall_amd.networks.psiformer import NetworkSpec
from oracle import reference as R

# nspins, exponents, flux
CASES = [((2, 2), (1, 1, 0), 1), ((2, 2), (3, 3, 2), 7), ((3, 3), (3, 3, 2), 12), ((2, 2), (3, 3, 1), 5),
         ((4, 2), (1, 3, 0), 3)]
VALID = CASES + [((3, 1), (1, 5, 1), 3), ((3, 0), (3, 1, 0), 6)]
# nspins, exponents, flux, S (S + 1)
EIGENSTATES = [((2, 2), (1, 1, 0), 1, 0.0), ((2, 2), (3, 3, 2), 7, 0.0), ((3, 3), (3, 3, 2), 12, 0.0),
               ((2, 2), (1, 1, 1), 3, 6.0), ((3, 1), (1, 1, 1), 3, 6.0), ((4, 2), (1, 3, 0), 3, 2.0),
               ((2, 1), (3, 3, 3), 6, 3.75)]


def _walkers(N, seed, cmax=1.0):
    g = torch.Generator().manual_seed(seed)
    th = torch.arccos((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * cmax)
    ph = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    return torch.stack([th, ph], -1)


def _pi_multiple(d):
    """The distance of an angle from the nearest multiple of pi."""
    return abs(math.remainder(d, math.pi))


@pytest.mark.parametrize("nspins,expo,flux", CASES)
def test_state_is_an_lll_singlet(nspins, expo, flux):
    """KE = N/2, Im KE = 0, L^2 = 0 and Lz = Lz^2 = 0 on every walker, to 1e-10 relative to
    max(1, geo), geo = Q^2 (sum 1/sin theta)^2, the size of the magnetic terms that cancel."""
    N = sum(nspins)
    m = HalperinCallable(nspins, flux, expo)
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


@pytest.mark.parametrize("nspins,expo,flux", CASES)
def test_antisymmetry_inside_a_species(nspins, expo, flux):
    """Exchanging two up electrons, or two down electrons, keeps Re log psi and moves the phase by pi."""
    m = HalperinCallable(nspins, flux, expo)
    N, n_up = sum(nspins), nspins[0]
    x = _walkers(N, 11)
    for i, k in ((0, n_up - 1), (n_up, N - 1)):
        assert i != k
        perm = list(range(N))
        perm[i], perm[k] = perm[k], perm[i]
        d = m(None, x[perm]) - m(None, x)
        assert abs(d.real.item()) < 1e-10 and abs(math.remainder(d.imag.item() - math.pi, 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,mm,flux", [((2, 1), 3, 6), ((2, 2), 3, 9), ((3, 0), 3, 6), ((1, 3), 3, 9)])
def test_equal_exponents_are_the_laughlin_state(nspins, mm, flux):
    """(m, m, m) is prod w^m whatever the species: the oracle's Laughlin state (m = 3: its Jastrow
    factor is not raised to a power) in Re, and in phase up to one constant multiple of pi per case
    (the determinant's column order, and its product over ordered pairs)."""
    m = HalperinCallable(nspins, flux, (mm, mm, mm))
    ocfg = R.LaughlinConfig(nspins=nspins, flux=flux)
    d = [m(None, x) - R.laughlin_logpsi(ocfg, x) for x in (_walkers(sum(nspins), s) for s in range(6))]
    for dk in d:
        assert abs(dk.real.item()) < 1e-10
        assert _pi_multiple(dk.imag.item()) < 1e-10
        assert abs(math.remainder((dk - d[0]).imag.item(), 2 * math.pi)) < 1e-10  # the same constant


@pytest.mark.parametrize("nspins,mm,flux", [((2, 2), 3, 3), ((3, 3), 3, 6)])
def test_no_interspecies_exponent_is_two_laughlin_states(nspins, mm, flux):
    """(m, m, 0) is the product of the two species' own Laughlin states."""
    n_up, n_dn = nspins
    m = HalperinCallable(nspins, flux, (mm, mm, 0))
    oup, odn = R.LaughlinConfig(nspins=(n_up, 0), flux=flux), R.LaughlinConfig(nspins=(n_dn, 0), flux=flux)
    d = []
    for s in range(6):
        x = _walkers(sum(nspins), s)
        d.append(m(None, x) - R.laughlin_logpsi(oup, x[:n_up]) - R.laughlin_logpsi(odn, x[n_up:]))
    for dk in d:
        assert abs(dk.real.item()) < 1e-10
        assert _pi_multiple(dk.imag.item()) < 1e-10
        assert abs(math.remainder((dk - d[0]).imag.item(), 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("nspins,expo,flux", CASES)
def test_batched_equals_per_walker(nspins, expo, flux):
    m = HalperinCallable(nspins, flux, expo)
    N = sum(nspins)
    xb = torch.stack([_walkers(N, s) for s in range(5)])
    one = torch.stack([m(None, x) for x in xb])
    assert one.dtype == torch.complex128
    assert torch.allclose(m(None, xb), one, rtol=0, atol=1e-12)
    xf = xb.float()  # float32 walkers are promoted, not computed in float32
    assert torch.allclose(m(None, xf), m(None, xf.double()), rtol=0, atol=1e-12)


def test_coincident_up_and_down_electrons_without_an_exponent():
    """At n = 0 an up and a down electron may sit on one point: log psi and its derivatives stay finite."""
    m = HalperinCallable((2, 2), 1, (1, 1, 0))
    x = _walkers(4, 3, cmax=0.9)
    x[2] = x[0]
    lp = m(None, x)
    assert torch.isfinite(lp.real) and torch.isfinite(lp.imag)
    g = torch.func.grad(lambda y: m(None, y).real)(x)
    assert torch.isfinite(g).all()


def _create(nspins, flux, expo, ntype="halperin", struct_size=None, plain=False):
    lib = _lib.load()
    spec = NetworkSpec(nspins=nspins, flux=flux, ndets=1, num_heads=1, heads_dim=4, num_layers=0, network_type=ntype,
                       halperin=tuple(expo))
    h = C.c_void_p()
    cfg = spec.to_c()
    assert C.sizeof(cfg) == 60
    if struct_size is not None:
        cfg.struct_size = struct_size
    if plain:
        rc = lib.dh_create(C.byref(cfg), C.byref(h))
    else:
        rc = lib.dh_create_halperin(C.byref(cfg), *expo, C.byref(h))
    if rc == 0:
        assert lib.dh_set_params(h, None, 0, None) == 0  # no parameters: count 0 is accepted
        lib.dh_destroy(h)
    return rc, lib.dh_last_error()


def test_native_validation():
    """dh_create_halperin: the exponents' parity and sign, both flux equations, N and the flux range."""
    assert C.sizeof(_lib.DhConfig) == 60
    assert NetworkSpec(nspins=(2, 2), flux=7, ndets=1, num_heads=1, heads_dim=4, num_layers=0,
                       network_type="halperin").to_c().network_type == 4
    for nspins, expo, flux in VALID + [((16, 16), (1, 1, 1), 31), ((32, 0), (3, 1, 0), 93)]:
        assert _create(nspins, flux, expo)[0] == 0, (nspins, expo, flux)
    bad = {
        "even m_up": _create((2, 2), 6, (2, 2, 2)),
        "even m_dn": _create((2, 1), 5, (3, 2, 2)),
        "m_up = 0": _create((1, 2), 4, (0, 1, 2)),
        "n < 0": _create((2, 2), 1, (3, 3, -1)),
        "up flux + 1": _create((2, 2), 8, (3, 3, 2)),
        "up flux - 1": _create((2, 2), 6, (3, 3, 2)),
        "down flux off by one": _create((2, 2), 7, (3, 5, 2)),   # up: 3 + 4 = 7, down: 5 + 4 = 9
        "down flux off by one, below": _create((3, 2), 8, (3, 3, 1)),  # up: 6 + 2 = 8, down: 3 + 3 = 6
        "N = 0": _create((0, 0), 1, (1, 1, 0)),
        "N = 33": _create((17, 16), 32, (1, 1, 1)),
        "flux 127": _create((2, 0), 127, (127, 1, 0)),
        "flux 0": _create((1, 0), 0, (1, 1, 0)),
        "type mismatch": _create((2, 2), 7, (3, 3, 2), ntype="pfaffian"),
        "struct_size": _create((2, 2), 7, (3, 3, 2), struct_size=56),
        "dh_create": _create((2, 2), 7, (3, 3, 2), plain=True),
    }
    for why, (rc, msg) in bad.items():
        assert rc == -1, why  # DH_EINVAL
        assert b"Halperin" in msg, (why, msg)
    assert b"dh_create_halperin" in bad["dh_create"][1]
    assert b"struct_size" in bad["struct_size"][1]
    assert b"= 7" in bad["up flux + 1"][1] and b"= 9" in bad["down flux off by one"][1]
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dh_create_halperin(None, 3, 3, 2, C.byref(h)) == -1


def test_python_validation_and_selection():
    net = config.Network()
    net.type = config.NetworkType.halperin
    model = make_network(config.System(nspins=(2, 2), flux=7), net)
    assert isinstance(model, Halperin) and model.spec.network_type == "halperin" and model.spec.halperin == (3, 3, 2)
    assert model.spec.to_c().network_type == 4
    assert model.init(device="cpu") == {}
    hash(model.spec)
    net.halperin.exponents = (1, 3, 0)
    model = make_network(config.System(nspins=(4, 2), flux=3), net)
    assert model.exponents == (1, 3, 0) and model.nspins == (4, 2)
    with pytest.raises(TypeError):
        model.vjp()
    for cls in (Halperin, HalperinCallable):
        for nspins, expo, flux in VALID:
            assert cls(nspins, flux, expo).exponents == tuple(expo)
        for nspins, expo, flux in [((2, 2), (2, 2, 2), 6), ((2, 2), (3, 3, -1), 1), ((2, 2), (3, 3, 2), 8),
                                   ((2, 2), (3, 5, 2), 7), ((0, 0), (1, 1, 0), 1), ((17, 16), (1, 1, 1), 32),
                                   ((2, 0), (127, 1, 0), 127), ((2, 2), (3, 3), 7)]:
            with pytest.raises(ValueError, match="Halperin"):
                cls(nspins, flux, expo)
    with pytest.raises(ValueError):
        make_network(config.System(nspins=(2, 2), flux=7), net)  # (1, 3, 0) does not live there


def test_config_round_trip():
    cfg = Config.from_dict({
        "system": {"nspins": (4, 2), "flux": 3},
        "network": {"type": "halperin", "halperin": {"exponents": [1, 3, 0]}},  # a list, as a config file gives it
    })
    assert cfg.network.type == config.NetworkType.halperin and cfg.network.halperin.exponents == (1, 3, 0)
    model = make_network(cfg.system, cfg.network)
    assert isinstance(model, Halperin) and model.exponents == (1, 3, 0)
    again = Config.from_dict(dataclasses.asdict(cfg))
    assert again.network.halperin == cfg.network.halperin and again.network.type == cfg.network.type
    assert Config.from_dict({}).network.halperin.exponents == (3, 3, 2)
    assert Config.from_dict({"network": {"type": "halperin"}}).network.halperin.exponents == (3, 3, 2)


def test_pretrain_reference():
    from deephall_amd import pretrain

    assert "halperin" in pretrain.REFERENCES
    cfg = Config.from_dict({
        "system": {"nspins": (3, 3), "flux": 12},
        "optim": {"optimizer": "adam", "pretrain": {"iterations": 5, "reference": "halperin"}},
    })
    ref = pretrain.make_reference(cfg)
    assert isinstance(ref, Halperin) and ref.exponents == (3, 3, 2) and ref.nspins == (3, 3)
    cfg.system.flux = 11
    with pytest.raises(ValueError, match="Halperin"):
        pretrain.make_reference(cfg)
    cfg.optim.pretrain.reference = "halperrin"
    with pytest.raises(ValueError, match="reference must be one of"):
        pretrain.make_reference(cfg)


def test_registry_lookups():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS
    from deephall_amd.netobs.observables import spin_square

    assert ESTIMATORS["spin_square"] is EXTRA_ESTIMATORS["spin_square"] is spin_square.DEFAULT
    assert spin_square.DEFAULT is spin_square.SpinSquareEstimator
    assert EXTRA_ESTIMATORS.more["spin_square"] is spin_square.DEFAULT
    assert ESTIMATORS.get("spin_square") is spin_square.DEFAULT
    assert "spin_square" not in list(ESTIMATORS) and "spin_square" not in list(EXTRA_ESTIMATORS)
    assert len(ESTIMATORS) == 4
    assert set(EXTRA_ESTIMATORS) == {"renyi2"}
    for bad in (0, -3, 2.5, True, "all"):
        with pytest.raises(ValueError, match="max_rows"):
            spin_square.spin_options({"max_rows": bad})
    assert spin_square.spin_options({}) is None and spin_square.spin_options({"max_rows": 7}) == 7


def test_spin_workspace_and_argument_checks():
    """The size, range and pointer checks of the dh_spin_* calls run before any launch: no GPU here."""
    lib = _lib.load()
    assert lib.dh_spin_workspace_bytes(257, 3, 2) >= 257 * 6 * 16 + 257 * 4
    assert lib.dh_spin_workspace_bytes(8, 4, 0) >= 8 * 4  # no pair: the valid flags only
    for B, n_up, n_dn in [(0, 2, 2), (8, -1, 2), (8, 0, 0), (8, 17, 16), (2**27, 4, 4)]:
        assert lib.dh_spin_workspace_bytes(B, n_up, n_dn) == 0, (B, n_up, n_dn)
    one = C.c_void_p(64)  # never dereferenced: every call below is refused first
    null = C.c_void_p(0)
    bad = [
        lib.dh_spin_exchange(null, 8, 4, 2, 2, 0, 4, one, None),
        lib.dh_spin_exchange(one, 8, 4, 2, 2, 0, 4, null, None),
        lib.dh_spin_exchange(one, 8, 5, 2, 2, 0, 4, one, None),     # n_up + n_dn != nelec
        lib.dh_spin_exchange(one, 8, 4, 2, 2, 0, 5, one, None),     # window past the last pair
        lib.dh_spin_exchange(one, 8, 4, 2, 2, 2, 2, one, None),     # empty window
        lib.dh_spin_exchange(one, 8, 4, 4, 0, 0, 1, one, None),     # no pair to exchange
        lib.dh_spin_exchange(one, 2**27, 8, 4, 4, 0, 1, one, None),
        lib.dh_spin_exchange(one, 8, 33, 17, 16, 0, 1, one, None),
        lib.dh_spin_ratios(one, null, 8, 2, 2, 0, 4, one, 1 << 20, None),
        lib.dh_spin_ratios(one, one, 8, 2, 2, -1, 4, one, 1 << 20, None),
        lib.dh_spin_reduce(one, 8, 2, 2, one, 1 << 20, one, null, one, one, None),  # pairs needed when P > 0
        lib.dh_spin_reduce(one, 8, 2, 2, null, 1 << 20, one, one, one, one, None),
        lib.dh_spin_reduce(one, 0, 2, 2, one, 1 << 20, one, one, one, one, None),
    ]
    assert bad == [-1] * len(bad)
    assert b"spin" in lib.dh_last_error()
    assert lib.dh_spin_ratios(one, one, 8, 2, 2, 0, 4, one, 16, None) == -3      # DH_ENOMEM
    assert lib.dh_spin_reduce(one, 8, 2, 2, one, 16, one, one, one, one, None) == -3


def test_spin_ref_exchange_order():
    x = np.arange(2 * 5 * 2, dtype=np.float32).reshape(2, 5, 2)
    xs = SR.exchange_rows(x, (3, 2))
    assert xs.shape == (6, 2, 5, 2) and SR.pair_slots((3, 2)) == [(0, 3), (0, 4), (1, 3), (1, 4), (2, 3), (2, 4)]
    assert (xs[3, 1, 1] == x[1, 4]).all() and (xs[3, 1, 4] == x[1, 1]).all() and (xs[3, 1, [0, 2, 3]] == x[1, [0, 2, 3]]).all()
    assert (SR.exchange_rows(x, (3, 2), 2, 5) == xs[2:5]).all()
    assert SR.exchange_rows(x, (5, 0)).shape == (0, 2, 5, 2)


def test_spin_ref_drops_non_finite_walkers():
    rng = np.random.default_rng(0)
    B, nspins = 6, (2, 1)
    lp = rng.normal(size=B) + 1j * rng.normal(size=B)
    lps = rng.normal(size=(2, B)) + 1j * rng.normal(size=(2, B))
    s2, pairs, total, nvalid = SR.spin_square(lp, lps, nspins)
    want = 0.25 + 1.5 - np.exp(lps - lp).sum(0)
    assert nvalid == B and np.allclose(s2, want, rtol=0, atol=1e-13) and np.isclose(total, want.sum())
    assert np.allclose(pairs[:, 0], np.exp(lps - lp).sum(1))
    lp2, lps2 = lp.copy(), lps.copy()
    lp2[1] = np.nan
    lps2[1, 4] = np.inf
    s2b, pairsb, totalb, nvalidb = SR.spin_square(lp2, lps2, nspins)
    keep = [0, 2, 3, 5]
    assert nvalidb == 4 and np.isnan(s2b[[1, 4]].real).all() and np.allclose(s2b[keep], want[keep], rtol=0, atol=1e-13)
    assert np.isclose(totalb, want[keep].sum()) and np.allclose(pairsb[:, 0], np.exp(lps - lp)[:, keep].sum(1))
    # one species empty: no pair, S^2 = (N/2)(N/2 + 1) on every walker
    s2c, pairsc, totalc, nvalidc = SR.spin_square(lp, np.zeros((0, B)), (3, 0))
    assert nvalidc == B and (s2c == 3.75).all() and pairsc.shape == (3, 0) and totalc == 3.75 * B


def _callable_fn(m):
    return lambda rows: m(None, torch.as_tensor(rows, dtype=torch.float64)).numpy()


@pytest.mark.parametrize("nspins,expo,flux,want", EIGENSTATES)
def test_total_spin_eigenstates(nspins, expo, flux, want):
    """S^2_loc = S (S + 1) on every walker, to 1e-8."""
    m = HalperinCallable(nspins, flux, expo)
    x = torch.stack([_walkers(sum(nspins), s) for s in range(16)]).numpy()
    s2, pairs, total, nvalid, _, _ = SR.spin_square_of(_callable_fn(m), x, nspins)
    assert nvalid == 16
    assert np.max(np.abs(s2 - want)) < 1e-8
    assert abs(total / nvalid - want) < 1e-8
    assert abs(pairs.sum() / nvalid - (((nspins[0] - nspins[1]) / 2) ** 2 + sum(nspins) / 2 - want)) < 1e-8


def test_331_is_no_total_spin_eigenstate():
    m = HalperinCallable((2, 2), 5, (3, 3, 1))
    x = torch.stack([_walkers(4, s) for s in range(16)]).numpy()
    s2, _, _, nvalid, _, _ = SR.spin_square_of(_callable_fn(m), x, (2, 2))
    assert nvalid == 16
    assert np.std(s2.real) > 0.1 and np.max(np.abs(s2.imag)) > 0.1
