"""Impurity potential and axis histogram without a GPU: the argument checks of dh_impurity_check,
dh_external_potential and dh_axis_histogram (validation comes before any device call), the
configuration (System.impurities, NetworkSpec.impurities, _check_system, make_local_kinetic_energy),
the estimator's options and digest, and the numpy restatement against the closed-form integrals."""

from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import impurity_ref as IR
from deephall_amd import _lib, config, hamiltonian
from deephall_amd.config import Config, Impurity, System
from deephall_amd.networks import make_network
from deephall_amd.networks.psiformer import NetworkSpec

DH_EINVAL = -1
NAN, INF = math.nan, math.inf


def _buf(n=64):
    """A host buffer standing in for a device pointer: a rejected call never touches it."""
    b = (C.c_float * n)()
    return b, C.cast(b, C.c_void_p)


def _arr(entries):
    arr = (_lib.DhImpurity * max(len(entries), 1))()
    for a, (theta, phi, strength, width, kind, species) in zip(arr, entries):
        a.theta, a.phi, a.strength, a.width, a.kind, a.species = theta, phi, strength, width, kind, species
    return arr


def _rejected(lib, rc):
    assert rc == DH_EINVAL
    assert lib.dh_last_error().startswith(b"impurity:"), lib.dh_last_error()


OK = (1.0, 2.0, 0.5, 1.5, 0, 0)  # theta, phi, strength, width, kind, species
BAD_ENTRIES = {
    "theta NaN": (NAN, 2.0, 0.5, 1.5, 0, 0), "phi inf": (1.0, INF, 0.5, 1.5, 0, 0),
    "strength NaN": (1.0, 2.0, NAN, 1.5, 0, 0), "width inf": (1.0, 2.0, 0.5, INF, 1, 0),
    "width 0": (1.0, 2.0, 0.5, 0.0, 0, 0), "width < 0, charge": (1.0, 2.0, 0.5, -1.0, 1, 0),
    "kind 2": (1.0, 2.0, 0.5, 1.5, 2, 0), "kind -1": (1.0, 2.0, 0.5, 1.5, -1, 0),
    "species 3": (1.0, 2.0, 0.5, 1.5, 0, 3), "species -1": (1.0, 2.0, 0.5, 1.5, 1, -1),
    "theta < 0": (-1e-9, 2.0, 0.5, 1.5, 0, 0), "theta > pi": (math.pi + 1e-9, 2.0, 0.5, 1.5, 0, 0),
}


def _external(lib, p, *, x=True, ext=True, B=8, n_up=2, n_dn=1, radius=1.2, entries=(OK,), n_imp=None, arr=True):
    a = _arr(entries) if arr else None
    return lib.dh_external_potential(p if x else None, B, n_up, n_dn, radius, a,
                                     len(entries) if n_imp is None else n_imp, None, p if ext else None, None)


def _hist(lib, p, *, x=True, counts=True, B=8, n_up=2, n_dn=1, theta=1.0, phi=0.5, bins=16):
    return lib.dh_axis_histogram(p if x else None, B, n_up, n_dn, theta, phi, bins, p if counts else None, None)


def test_constants_and_struct():
    assert _lib.DH_MAX_IMPURITIES == 8 == config.MAX_IMPURITIES
    assert _lib.IMPURITY_KINDS == {"gaussian": 0, "charge": 1}
    assert _lib.IMPURITY_SPECIES == {k: _lib.HOLE_KINDS[k] for k in ("both", "up", "down")}
    assert C.sizeof(_lib.DhImpurity) == 40
    for s in ("dh_impurity_check", "dh_external_potential", "dh_axis_histogram"):
        assert s in _lib.EXPORTS and hasattr(_lib.load(), s)


def test_impurity_check_accepts_good_arrays():
    lib = _lib.load()
    assert lib.dh_impurity_check(None, 0) == 0
    assert lib.dh_impurity_check(_arr([OK]), 1) == 0
    ends = [(0.0, -7.0, -2.0, 1e-3, 1, 2), (math.pi, 9.0, 0.0, 1e3, 0, 1)]
    assert lib.dh_impurity_check(_arr(ends * 4), 8) == 0


@pytest.mark.parametrize("name", sorted(BAD_ENTRIES))
def test_bad_entries_are_rejected(name):
    lib = _lib.load()
    keep, p = _buf()
    for entries in ([BAD_ENTRIES[name]], [OK, OK, BAD_ENTRIES[name]]):
        _rejected(lib, lib.dh_impurity_check(_arr(entries), len(entries)))
        _rejected(lib, _external(lib, p, entries=entries))
    del keep


def test_bad_counts_and_null_arrays_are_rejected():
    lib = _lib.load()
    keep, p = _buf()
    for n in (-1, 9, 2**31 - 1):
        _rejected(lib, lib.dh_impurity_check(_arr([OK] * 8), n))
        _rejected(lib, _external(lib, p, entries=[OK] * 8, n_imp=n))
    _rejected(lib, lib.dh_impurity_check(None, 1))
    _rejected(lib, _external(lib, p, arr=False, n_imp=1))
    del keep


@pytest.mark.parametrize("bad", [dict(x=False), dict(ext=False), dict(B=0), dict(B=-2), dict(n_up=-1), dict(n_dn=-1),
                                 dict(n_up=0, n_dn=0), dict(n_up=32, n_dn=1), dict(n_up=2**30, n_dn=2**30),
                                 dict(B=2**27, n_up=16, n_dn=0), dict(radius=0.0), dict(radius=-1.0),
                                 dict(radius=NAN), dict(radius=INF)], ids=str)
def test_external_potential_rejects_bad_arguments(bad):
    lib = _lib.load()
    keep, p = _buf()
    _rejected(lib, _external(lib, p, **bad))
    del keep


@pytest.mark.parametrize("bad", [dict(x=False), dict(counts=False), dict(B=0), dict(n_up=-1), dict(n_up=0, n_dn=0),
                                 dict(n_up=20, n_dn=13), dict(B=2**27, n_up=8, n_dn=8), dict(theta=NAN),
                                 dict(phi=INF), dict(theta=-0.1), dict(theta=3.2), dict(bins=0), dict(bins=-4),
                                 dict(bins=4097)], ids=str)
def test_axis_histogram_rejects_bad_arguments(bad):
    lib = _lib.load()
    keep, p = _buf()
    _rejected(lib, _hist(lib, p, **bad))
    del keep


def test_wrappers_refuse_cpu_tensors():
    from deephall_amd.netobs import _native

    x = torch.zeros(4, 3, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        _native.axis_histogram(x, (2, 1), (1.0, 0.0), 8)
    with pytest.raises(RuntimeError, match="GPU"):
        hamiltonian.make_external_potential([(1.0, 0.0, 1.0)], (2, 1), 1.0)(x)
    with pytest.raises(RuntimeError, match="impurity:"):  # checked when the function is made
        hamiltonian.make_external_potential([(4.0, 0.0, 1.0)], (2, 1), 1.0)


# ---- configuration ------------------------------------------------------------------------------------

AS_LISTS = [[1.1, 2.8, 0.5], [0.3, -1.0, -0.25, "charge", 0.7, "up"]]
AS_DICTS = [{"theta": 1.1, "phi": 2.8, "strength": 0.5},
            {"theta": 0.3, "phi": -1.0, "strength": -0.25, "kind": "charge", "width": 0.7, "species": "up"}]
WANT = (Impurity(1.1, 2.8, 0.5, "gaussian", 1.0, "both"), Impurity(0.3, -1.0, -0.25, "charge", 0.7, "up"))


@pytest.mark.parametrize("entries", [AS_LISTS, AS_DICTS, list(WANT)], ids=["lists", "dicts", "objects"])
def test_config_from_dict_with_impurities(entries):
    cfg = Config.from_dict({"system": {"nspins": (3, 0), "flux": 7, "impurities": entries}})
    assert cfg.system.impurities == WANT and isinstance(cfg.system.impurities, tuple)
    assert hash(cfg.system.impurities) == hash(WANT)
    # the round trip through the saved config's plain form (log.py)
    from deephall_amd.log import _plain

    plain = _plain(cfg)
    assert plain["system"]["impurities"][1] == AS_DICTS[1]
    import yaml

    again = Config.from_dict(yaml.safe_load(yaml.safe_dump(plain)))
    assert again.system.impurities == WANT


def test_config_default_and_refusals():
    assert System().impurities == () and Config().system.impurities == ()
    assert "impurities" in [f.name for f in dataclasses.fields(System)]
    for bad in ([[1.0, 0.0, 1.0, "square"]], [[1.0, 0.0, 1.0, "gaussian", 0.0]], [[1.0, 0.0, 1.0, "charge", -1.0]],
                [[1.0, 0.0, 1.0, "gaussian", 1.0, "left"]], [[1.0, 0.0, 1.0]] * 9):
        with pytest.raises(ValueError, match="impurity"):
            System(impurities=bad)


NETWORKS = {
    "psiformer": dict(system=dict(nspins=(3, 0), flux=2), network={}),
    "laughlin": dict(system=dict(nspins=(3, 0), flux=6), network={"type": "laughlin"}),
    "jain": dict(system=dict(nspins=(4, 0), flux=6), network={"type": "jain"}),
    "pfaffian": dict(system=dict(nspins=(4, 0), flux=5), network={"type": "pfaffian"}),
    "halperin": dict(system=dict(nspins=(2, 2), flux=7), network={"type": "halperin"}),
    "quasihole": dict(system=dict(nspins=(3, 0), flux=7),
                      network={"type": "quasihole", "halperin": {"exponents": [3, 3, 0]},
                               "quasihole": {"holes": [[1.1, 2.8]]}}),
}


def _build(kind, impurities=()):
    case = NETWORKS[kind]
    cfg = Config.from_dict({"system": {**case["system"], "impurities": list(impurities)}, "network": case["network"]})
    return cfg.system, make_network(cfg.system, cfg.network)


@pytest.mark.parametrize("kind", sorted(NETWORKS))
def test_every_builder_carries_the_impurities(kind):
    system0, plain = _build(kind)
    system1, model = _build(kind, AS_LISTS)
    assert plain.spec.impurities == () and model.spec.impurities == WANT
    # nothing else moves: the spec without impurities is the parent's plus the default field
    assert dataclasses.replace(model.spec, impurities=()) == plain.spec
    assert hash(dataclasses.replace(model.spec, impurities=())) == hash(plain.spec)
    hamiltonian._check_system(model, system1)
    hamiltonian._check_system(plain, system0)
    for net, system in ((model, system0), (plain, system1)):
        with pytest.raises(ValueError, match="differs from the network"):
            hamiltonian._check_system(net, system)
    other = dataclasses.replace(system1, impurities=AS_LISTS[:1])
    with pytest.raises(ValueError, match="differs from the network"):
        hamiltonian._check_system(model, other)
    # with_system keeps them; to_c does not see them
    moved = model.with_system(radius=2.0, interaction_strength=0.5)
    assert moved.spec.impurities == WANT and moved.spec.radius == 2.0
    assert bytes(model.spec.to_c()) == bytes(plain.spec.to_c())


def test_networkspec_default_field():
    kw = dict(nspins=(3, 0), flux=2, ndets=1, num_heads=4, heads_dim=64, num_layers=2)
    a, b = NetworkSpec(**kw), NetworkSpec(**kw, impurities=())
    assert a == b and hash(a) == hash(b) and a.impurities == ()
    assert a != NetworkSpec(**kw, impurities=WANT)
    assert [f.name for f in dataclasses.fields(NetworkSpec)][-1] == "impurities"


def test_kinetic_energy_drops_the_impurities(monkeypatch):
    system, model = _build("psiformer", AS_LISTS)
    seen = []
    monkeypatch.setattr(hamiltonian, "_run_local_energy", lambda net, *a, **k: seen.append(net.spec) or (None, None))
    monkeypatch.setattr(hamiltonian, "_observables", lambda e_l, obs: (None, dict.fromkeys(
        ("kinetic", "angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square"))))
    for r in (1.0, 2.5):  # the default radius sqrt(Q) = 1 and another one
        hamiltonian.make_local_kinetic_energy(model, 1.0, r)(None, None)
    assert [s.impurities for s in seen] == [(), ()]
    assert model.spec.impurities == WANT


# ---- the estimator's registration, options and digest ----------------------------------------------------

def test_axis_density_is_registered_apart_from_the_pinned_names():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS
    from deephall_amd.netobs.observables import axis_density

    cls = axis_density.AxisDensityEstimator
    assert ESTIMATORS["axis_density"] is EXTRA_ESTIMATORS["axis_density"] is axis_density.DEFAULT is cls
    assert EXTRA_ESTIMATORS.more["axis_density"] is cls
    assert list(ESTIMATORS) == ["density", "pair_corr", "overlap", "one_rdm"] and list(EXTRA_ESTIMATORS) == ["renyi2"]


class _Adaptor:
    def __init__(self, cfg):
        self.cfg = cfg


def test_axis_density_reads_its_options():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables.axis_density import AxisDensityEstimator as Est

    sys_ = HallSystem(spins=[2, 1], flux=3)
    est = Est(None, sys_, {"axis": [1.0, 2.0]}, {})
    assert (est.axis, est.bins, est.nspins) == ((1.0, 2.0), 50, (2, 1)) and est.observable.shape == (50,)
    assert est.empty_val_state(4) == ({}, {"counts": None, "walkers": 0})
    cfg = Config.from_dict({"system": {"nspins": (2, 1), "flux": 3, "impurities": AS_LISTS}})
    est = Est(_Adaptor(cfg), sys_, {"impurity": 1, "bins": 16}, {})
    assert (est.axis, est.bins) == ((0.3, -1.0), 16)
    for bad in ({}, {"axis": [1.0, 2.0], "impurity": 0}, {"impurity": 2}, {"impurity": -1}, {"impurity": 0.5},
                {"axis": [1.0]}, {"axis": [4.0, 0.0]}, {"axis": [1.0, NAN]}, {"axis": [1.0, 2.0], "bins": 0},
                {"axis": [1.0, 2.0], "bins": 4097}, {"axis": [1.0, 2.0], "bins": 2.5}):
        with pytest.raises(ValueError, match="axis_density"):
            Est(_Adaptor(cfg), sys_, bad, {})
    with pytest.raises(ValueError, match="axis_density"):
        Est(None, sys_, {"impurity": 0}, {})  # no config to take it from


def test_digest_on_hand_made_counts():
    from deephall_amd.netobs.observables.axis_density import digest_counts

    W, nspins, bins = 10, (2, 1), 4
    counts = torch.tensor([[2, 8, 6, 4], [1, 3, 2, 4]])  # rows sum to W n_up, W n_dn
    out = digest_counts(counts, W, nspins)
    both = torch.tensor([3.0, 11.0, 8.0, 8.0], dtype=torch.float64)
    assert torch.allclose(out["theta"], torch.acos(torch.tensor([0.75, 0.25, -0.25, -0.75], dtype=torch.float64)))
    assert torch.allclose(out["theta_edge"], torch.acos(torch.tensor([0.5, 0.0, -0.5, -1.0], dtype=torch.float64)))
    assert out["density"].shape == (3, 4) and torch.allclose(out["density"][2], both * 4 / 30)
    assert torch.allclose(out["density"][0], counts[0].double() * 4 / 30)
    assert abs(out["density"][2].mean().item() - 1.0) < 1e-15  # the uniform density is the unit
    assert torch.allclose(out["excess"], (both / W - 3 / 4).cumsum(0)) and out["excess"][-1].item() == 0.0
    cum = both.cumsum(0)
    assert torch.allclose(out["excess_err"], (cum * (1 - cum / 30)).sqrt() / W) and out["excess_err"][-1].item() == 0.0
    assert torch.allclose(out["density_err"][2], (both * (1 - both / 30)).sqrt() * 4 / 30)


# ---- the restatement ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,width", [("gaussian", 0.3), ("gaussian", 1.0), ("gaussian", 4.0), ("charge", 0.2),
                                        ("charge", 1.0), ("charge", 5.0)])
@pytest.mark.parametrize("radius", [1.0, math.sqrt(8.0)])
def test_restatement_against_the_closed_forms(kind, width, radius):
    s = -0.7
    closed, quad = IR.integral_closed(s, kind, width, radius), IR.integral_quadrature(s, kind, width, radius)
    print(f"{kind} w = {width} R = {radius:.3f}: closed {closed:.12f} quadrature {quad:.12f}")
    assert abs(quad - closed) < 1e-9 * abs(closed)


def test_restatement_special_points():
    R = 1.7
    x = np.array([[[0.0, 0.3], [math.pi, 1.0], [1.1, 2.8]]])
    # chord 0: U = s, respectively s / h; the antipode: chord 2 R
    for kind, at0, far in (("gaussian", 0.5, 0.5 * math.exp(-2 * R * R / 0.49)), ("charge", 0.5 / 0.7, 0.5 / math.hypot(2 * R, 0.7))):
        U = IR.per_electron(x, (3, 0), R, [(0.0, 0.0, 0.5, kind, 0.7, "both")])[0]
        assert abs(U[0] - at0) < 1e-15 and abs(U[1] - far) < 1e-15
        U = IR.per_electron(x, (3, 0), R, [(1.1, 2.8, 0.5, kind, 0.7, "both")])[0]
        assert abs(U[2] - at0) < 1e-15
    # species: up is the slots below n_up
    U = IR.per_electron(x, (2, 1), R, [(1.0, 0.0, 1.0, "gaussian", 1.0, "up")])[0]
    D = IR.per_electron(x, (2, 1), R, [(1.0, 0.0, 1.0, "gaussian", 1.0, "down")])[0]
    assert U[2] == 0.0 and (U[:2] > 0).all() and (D[:2] == 0).all() and D[2] > 0
    bad = x.copy()
    bad[0, 1, 1] = np.inf
    assert np.isnan(IR.external(bad, (3, 0), R, IR.MIXED)[0])


def test_restatement_histogram():
    x = IR.walkers(500, 5, seed=3)
    counts, flagged = IR.histogram(x, (3, 2), (0.0, 0.0), 64)
    assert flagged == 0 and counts[0].sum() == 1500 and counts[1].sum() == 1000
    # about the north pole u = cos theta: numpy's own histogram, the edges ascending in u
    for row, sl in ((0, slice(0, 3)), (1, slice(3, 5))):
        want, _ = np.histogram(np.cos(x[:, sl, 0].astype(np.float64)), bins=64, range=(-1.0, 1.0))
        assert (counts[row] == want[::-1]).all()
    edge = np.array([[[math.acos(0.5), 0.0], [0.0, 0.0], [math.pi, 0.0], [np.nan, 0.0]]])
    counts, flagged = IR.histogram(edge, (4, 0), (0.0, 0.0), 4)
    assert flagged == 3 and counts[0].sum() == 3 and counts[0][0] >= 1 and counts[0][3] == 1
