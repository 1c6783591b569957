"""Pinned quasiholes (networks/quasihole.py) on the host, float64.

`QuasiholeCallable` is the state's independent route.  Here it is pinned by identities the state
must satisfy: a hole at a pole of a Laughlin base is the reference's Laughlin quasihole (a
determinant with one orbital dropped); two coincident groups of the Pfaffian base are one Abelian
hole times 2^(N/2); the three pairings of four holes span a two-dimensional space; the state stays
antisymmetric with holes present and is a lowest-Landau-level state (KE = N/2).  The native
library's validation (dh_create_quasihole) runs without a GPU, as do the config and the network
selection.  The kernels themselves are tested in test_gpu_quasihole.py."""

from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from deephall_amd import Config, _lib, config, make_network
from deephall_amd.networks import Quasihole, QuasiholeCallable
from deephall_amd.networks.psiformer import NetworkSpec
from oracle import reference as R

HOLES4 = ((0.7, 0.3), (1.9, -2.1), (2.6, 1.2), (1.1, 2.8))


def _walkers(N, seed, cmax=1.0):
    g = torch.Generator().manual_seed(seed)
    th = torch.arccos((torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * cmax)
    ph = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    return torch.stack([th, ph], -1)


@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("theta,sign", [(0.0, -1), (math.pi, +1)])
def test_pole_hole_is_the_laughlin_quasihole(N, theta, sign):
    """One hole at theta = 0 on Laughlin 1/3 is prod v_i x the ground state: the reference's quasihole
    determinant with excitation_lz = -N/2 (the orbital m = +Q1 dropped), up to one constant; a hole
    at theta = pi is excitation_lz = +N/2."""
    flux = 3 * (N - 1) + 1
    m = QuasiholeCallable((N, 0), flux, holes=((theta, 0.4),), exponents=(3, 3, 0))
    ocfg = R.LaughlinConfig(nspins=(N, 0), flux=flux, excitation_lz=sign * N / 2)
    assert ocfg.kind() == "quasihole"
    d = torch.stack([m(None, x) - R.laughlin_logpsi(ocfg, x) for x in (_walkers(N, s) for s in range(8))])
    spread_re = (d.real - d.real[0]).abs().max().item()
    spread_im = max(abs(math.remainder(v, 2 * math.pi)) for v in (d.imag - d.imag[0]).tolist())
    print(f"N = {N} theta = {theta}: spread re {spread_re:.1e} im {spread_im:.1e}")
    assert spread_re < 1e-11 and spread_im < 1e-11


@pytest.mark.parametrize("N,p", [(6, 1), (4, 2)])
def test_coincident_groups_are_an_abelian_hole(N, p):
    """A = {a}, B = {b} at one point: F = G = s, A_ik = 2 s_i s_k / w_ik, Pf = 2^(N/2) prod s x Pf(1 / w)."""
    flux = 2 * p * (N - 1) - 1 + 1
    pt = (1.3, 0.6)
    pair = QuasiholeCallable((N, 0), flux, base="pfaffian", holes=(pt, pt), pairing=((0,), (1,)), cf_flux=p)
    abel = QuasiholeCallable((N, 0), flux, base="pfaffian", holes=(pt,), cf_flux=p)
    for s in range(6):
        x = _walkers(N, s)
        ratio = torch.exp(pair(None, x) - abel(None, x))
        assert abs(ratio.real.item() - 2.0 ** (N / 2)) < 1e-10 * 2.0 ** (N / 2), ratio
        assert abs(ratio.imag.item()) < 1e-10 * 2.0 ** (N / 2)


def test_four_hole_pairings_span_two_dimensions():
    """The three pairings of four holes at generic points, N = 6, on 16 walkers: the 16 x 3 matrix of
    amplitudes (columns scaled to unit max) has rank 2."""
    N, flux = 6, 2 * 5 - 1 + 2
    x = torch.stack([_walkers(N, s) for s in range(16)])
    cols = []
    for pairing in (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2))):
        m = QuasiholeCallable((N, 0), flux, base="pfaffian", holes=HOLES4, pairing=pairing)
        lp = m(None, x)
        cols.append(torch.exp(lp - lp.real.max()))
    sv = torch.linalg.svdvals(torch.stack(cols, dim=1))
    print("singular values", sv.tolist())
    assert (sv[2] / sv[0]).item() < 1e-10
    assert (sv[1] / sv[0]).item() > 0.1


CASES = [
    dict(nspins=(4, 0), flux=11, holes=((0.0, 0.0), (1.2, 0.5)), exponents=(3, 3, 0)),
    dict(nspins=(2, 2), flux=8, holes=((0.9, -1.0), (2.0, 2.2)), species=("up", "down")),
    dict(nspins=(3, 2), flux=10, holes=((1.4, 0.2),), species=("down",)),
    dict(nspins=(6, 0), flux=11, base="pfaffian", holes=HOLES4, pairing=((0, 2), (1, 3))),
    dict(nspins=(6, 0), flux=11, base="pfaffian", holes=((0.5, 1.0), (2.2, -0.4), (1.5, 2.9)), pairing=((0,), (2,))),
    dict(nspins=(2, 0), flux=2, base="pfaffian", holes=((0.5, 1.0), (2.2, -0.4)), pairing=((0,), (1,))),
]


def _make(case, cls=QuasiholeCallable):
    kw = {k: v for k, v in case.items() if k not in ("nspins", "flux")}
    return cls(case["nspins"], case["flux"], **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.get('base', 'halperin')}-{c['nspins']}-{c['flux']}")
def test_antisymmetry_with_holes(case):
    """Exchanging two electrons of one species keeps Re log psi and moves the phase by pi."""
    m = _make(case)
    N, n_up = sum(case["nspins"]), case["nspins"][0]
    pfaffian = case.get("base") == "pfaffian"
    x = _walkers(N, 11)
    swaps = [(0, N - 1)] if pfaffian else [(i, k) for i, k in ((0, n_up - 1), (n_up, N - 1)) if i < k]
    assert swaps
    for i, k in swaps:
        perm = list(range(N))
        perm[i], perm[k] = perm[k], perm[i]
        d = m(None, x[perm]) - m(None, x)
        assert abs(d.real.item()) < 1e-10 and abs(math.remainder(d.imag.item() - math.pi, 2 * math.pi)) < 1e-10


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c.get('base', 'halperin')}-{c['nspins']}-{c['flux']}")
def test_state_is_in_the_lowest_landau_level(case):
    """KE = N/2 and Im KE = 0 on every walker, to 1e-9 relative to max(1, geo): every electron has
    degree flux in (u, v)."""
    m = _make(case)
    N = sum(case["nspins"])
    ocfg = R.LaughlinConfig(nspins=case["nspins"], flux=case["flux"])  # Q and the default radius only
    ke = R.make_local_kinetic_energy(lambda params, y: m(None, y), ocfg.Q, ocfg.r)
    for seed in range(2):
        x = _walkers(N, seed, cmax=0.9)
        kin, _ = ke(None, x)
        scale = max(1.0, (ocfg.Q**2 * (1 / torch.sin(x[:, 0])).sum() ** 2).item())
        assert abs(complex(kin) - N / 2) / scale < 1e-9


def test_batched_equals_per_walker():
    for case in CASES:
        m = _make(case)
        xb = torch.stack([_walkers(sum(case["nspins"]), s) for s in range(4)])
        one = torch.stack([m(None, x) for x in xb])
        assert one.dtype == torch.complex128
        d = m(None, xb) - one
        assert d.real.abs().max() < 1e-11
        assert max(abs(math.remainder(v, 2 * math.pi)) for v in d.imag.tolist()) < 1e-11


def test_electron_on_a_hole_is_a_node():
    m = QuasiholeCallable((3, 0), 7, holes=((1.0, 0.5),), exponents=(3, 3, 0))
    x = _walkers(3, 2)
    x[1] = torch.tensor([1.0, 0.5], dtype=torch.float64)
    assert m(None, x).real.item() < -30.0


KINDS = {"both": 0, "up": 1, "down": 2, "A": 3, "B": 4}


def _create(nspins, flux, base=0, expo=(3, 3, 2), p=1, holes=((1.0, 0.5),), kinds=None, ntype="quasihole",
            struct_size=None, q_size=None, plain=False, n_holes=None):
    lib = _lib.load()
    spec = NetworkSpec(nspins=nspins, flux=flux, ndets=1, num_heads=1, heads_dim=4, num_layers=0, network_type=ntype)
    cfg = spec.to_c()
    assert C.sizeof(cfg) == 60
    if struct_size is not None:
        cfg.struct_size = struct_size
    q = _lib.DhQuasihole()
    q.base = base
    q.m_up, q.m_dn, q.n_inter, q.p = *expo, p
    q.n_holes = len(holes) if n_holes is None else n_holes
    for a, (t, ph) in enumerate(holes):
        q.holes[a][0], q.holes[a][1] = t, ph
        q.kind[a] = KINDS[kinds[a]] if kinds is not None and isinstance(kinds[a], str) else (kinds[a] if kinds else 0)
    if q_size is not None:
        q.struct_size = q_size
    h = C.c_void_p()
    rc = lib.dh_create(C.byref(cfg), C.byref(h)) if plain else lib.dh_create_quasihole(C.byref(cfg), C.byref(q), C.byref(h))
    if rc == 0:
        assert lib.dh_set_params(h, None, 0, None) == 0  # no parameters: count 0 is accepted
        lib.dh_destroy(h)
    return rc, lib.dh_last_error()


def test_native_validation():
    """dh_create_quasihole: the flux rules of both bases, equal groups, N even, kinds per base, the
    angles, the hole count, the struct sizes; dh_create refuses the type."""
    assert C.sizeof(_lib.DhConfig) == 60 and C.sizeof(_lib.DhQuasihole) == 192
    assert NetworkSpec(nspins=(3, 0), flux=7, ndets=1, num_heads=1, heads_dim=4, num_layers=0,
                       network_type="quasihole").to_c().network_type == 5
    two = ((1.0, 0.5), (2.0, -1.0))
    good = [
        _create((3, 0), 7, expo=(3, 3, 0)),
        _create((4, 0), 11, expo=(3, 1, 0), holes=((0.0, 0.0), (math.pi, 7.0))),
        _create((2, 2), 8),
        _create((2, 2), 8, holes=two, kinds=("up", "down")),
        _create((3, 2), 10, kinds=("down",)),
        _create((32, 0), 94, expo=(3, 3, 0)),
        _create((2, 0), 2, base=1, holes=two, kinds=("A", "B")),
        _create((4, 0), 12, base=1, p=2, holes=two, kinds=("A", "B")),
        _create((6, 0), 11, base=1, holes=HOLES4, kinds=("A", "B", "B", "A")),
        _create((6, 0), 11, base=1, holes=two + ((0.3, 0.3),), kinds=("A", "B", "both")),
        _create((6, 0), 10, base=1, holes=((0.3, 0.3),), kinds=("both",)),
        _create((28, 0), 54, base=1, holes=two, kinds=("A", "B")),
        _create((4, 0), 17, expo=(3, 3, 0), holes=tuple((1.0, 0.1 * a) for a in range(8))),
    ]
    for rc, msg in good:
        assert rc == 0, msg
    bad = {
        "flux + 1": _create((3, 0), 8, expo=(3, 3, 0)),
        "flux of the ground state": _create((3, 0), 6, expo=(3, 3, 0)),
        "down flux": _create((2, 2), 8, kinds=("up",)),          # up 3 + 4 + 1 = 8, down 3 + 4 + 0 = 7
        "up flux": _create((3, 2), 10, kinds=("both",)),         # up 6 + 4 + 1 = 11
        "even m_up": _create((3, 0), 5, expo=(2, 3, 0)),
        "n < 0": _create((2, 2), 8, expo=(3, 3, -1)),
        "group on the halperin base": _create((3, 0), 7, expo=(3, 3, 0), kinds=("A",)),
        "species on the pfaffian base": _create((6, 0), 10, base=1, kinds=("up",)),
        "kind 5": _create((3, 0), 7, expo=(3, 3, 0), kinds=(5,)),
        "kind -1": _create((3, 0), 7, expo=(3, 3, 0), kinds=(-1,)),
        "unequal groups": _create((6, 0), 11, base=1, holes=two, kinds=("A", "A")),
        "one group only": _create((6, 0), 10, base=1, kinds=("A",)),
        "odd N": _create((5, 0), 8, base=1, holes=two, kinds=("A", "B")),
        "pfaffian flux": _create((6, 0), 11, base=1, holes=two, kinds=("A", "B")),
        "pfaffian p = 0": _create((6, 0), 10, base=1, p=0, holes=two, kinds=("A", "B")),
        "pfaffian N = 30": _create((30, 0), 58, base=1, holes=two, kinds=("A", "B")),
        "no holes, halperin": _create((3, 0), 6, expo=(3, 3, 0), holes=()),
        "no holes, pfaffian": _create((6, 0), 9, base=1, holes=()),
        "nine holes": _create((4, 0), 18, expo=(3, 3, 0), n_holes=9),
        "nan theta": _create((3, 0), 7, expo=(3, 3, 0), holes=((float("nan"), 0.0),)),
        "inf phi": _create((3, 0), 7, expo=(3, 3, 0), holes=((1.0, float("inf")),)),
        "theta < 0": _create((3, 0), 7, expo=(3, 3, 0), holes=((-0.1, 0.0),)),
        "theta > pi": _create((3, 0), 7, expo=(3, 3, 0), holes=((3.2, 0.0),)),
        "base 2": _create((3, 0), 7, base=2, expo=(3, 3, 0)),
        "N = 33": _create((33, 0), 97, expo=(3, 3, 0)),
        "flux 127": _create((2, 0), 127, expo=(125, 1, 0), holes=two),
        "type mismatch": _create((3, 0), 7, expo=(3, 3, 0), ntype="halperin"),
        "struct_size": _create((3, 0), 7, expo=(3, 3, 0), struct_size=56),
        "dh_quasihole size": _create((3, 0), 7, expo=(3, 3, 0), q_size=188),
        "dh_create": _create((3, 0), 7, expo=(3, 3, 0), plain=True),
    }
    for why, (rc, msg) in bad.items():
        assert rc == -1, why  # DH_EINVAL
        assert msg.startswith(b"Quasihole"), (why, msg)
    assert b"dh_create_quasihole" in bad["dh_create"][1]
    assert b"pfaffian" in bad["no holes, pfaffian"][1]
    assert b"= 7" in bad["flux + 1"][1] and b"= 10" in bad["pfaffian flux"][1]
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dh_create_quasihole(None, None, C.byref(h)) == -1


def test_python_validation_and_selection():
    net = config.Network()
    net.type = config.NetworkType.quasihole
    net.halperin.exponents = (3, 3, 0)
    net.quasihole.holes = ((1.0, 0.5),)
    model = make_network(config.System(nspins=(3, 0), flux=7), net)
    assert isinstance(model, Quasihole) and model.spec.network_type == "quasihole"
    assert model.spec.quasihole == ("halperin", (3, 3, 0), 1, ((1.0, 0.5, "both"),))
    assert model.spec.to_c().network_type == 5
    assert model.init(device="cpu") == {}
    hash(model.spec)
    with pytest.raises(TypeError):
        model.vjp()
    net.quasihole = config.QuasiholeNetwork(base="pfaffian", holes=HOLES4, pairing=((0, 3), (1, 2)))
    model = make_network(config.System(nspins=(6, 0), flux=11), net)
    assert model.base == "pfaffian" and [h[2] for h in model.holes] == ["A", "B", "B", "A"] and model.cf_flux == 1
    two = ((1.0, 0.5), (2.0, -1.0))
    for cls in (Quasihole, QuasiholeCallable):
        for case in CASES:
            assert _make(case, cls).flux == case["flux"]
        bad = [
            dict(nspins=(3, 0), flux=8, holes=two[:1], exponents=(3, 3, 0)),
            dict(nspins=(2, 2), flux=8, holes=two[:1], species=("up",)),
            dict(nspins=(3, 0), flux=5, holes=two[:1], exponents=(2, 3, 0)),
            dict(nspins=(3, 0), flux=7, holes=two[:1], exponents=(3, 3, 0), species=("A",)),
            dict(nspins=(3, 0), flux=7, holes=two[:1], exponents=(3, 3, 0), pairing=((0,), ())),
            dict(nspins=(3, 0), flux=8, holes=two, exponents=(3, 3, 0), species=("both",)),
            dict(nspins=(6, 0), flux=10, base="pfaffian", holes=two[:1], species=("up",)),
            dict(nspins=(6, 0), flux=11, base="pfaffian", holes=two, pairing=((0, 1), ())),
            dict(nspins=(6, 0), flux=10, base="pfaffian", holes=two, pairing=((0,), (0,))),
            dict(nspins=(6, 0), flux=10, base="pfaffian", holes=two, pairing=((0,), (2,))),
            dict(nspins=(5, 0), flux=8, base="pfaffian", holes=two, pairing=((0,), (1,))),
            dict(nspins=(6, 0), flux=11, base="pfaffian", holes=two, pairing=((0,), (1,))),
            dict(nspins=(30, 0), flux=58, base="pfaffian", holes=two, pairing=((0,), (1,))),
            dict(nspins=(6, 0), flux=9, base="pfaffian", holes=()),
            dict(nspins=(3, 0), flux=6, holes=(), exponents=(3, 3, 0)),
            dict(nspins=(4, 0), flux=18, holes=tuple((1.0, 0.1 * a) for a in range(9)), exponents=(3, 3, 0)),
            dict(nspins=(3, 0), flux=7, holes=((float("nan"), 0.0),), exponents=(3, 3, 0)),
            dict(nspins=(3, 0), flux=7, holes=((3.2, 0.0),), exponents=(3, 3, 0)),
            dict(nspins=(3, 0), flux=7, holes=((-0.1, 0.0),), exponents=(3, 3, 0)),
            dict(nspins=(3, 0), flux=7, base="laughlin", holes=two[:1], exponents=(3, 3, 0)),
            dict(nspins=(33, 0), flux=97, holes=two[:1], exponents=(3, 3, 0)),
        ]
        for case in bad:
            with pytest.raises(ValueError, match="Quasihole"):
                _make(case, cls)


def test_config_round_trip():
    cfg = Config.from_dict({
        "system": {"nspins": (6, 0), "flux": 11},
        "network": {"type": "quasihole",  # lists, as a config file gives them
                    "quasihole": {"base": "pfaffian", "holes": [[0.5, 1.0], [2.2, -0.4], [1.5, 2.9]],
                                  "pairing": [[0], [2]]}},
    })
    q = cfg.network.quasihole
    assert cfg.network.type == config.NetworkType.quasihole
    assert q.holes == ((0.5, 1.0), (2.2, -0.4), (1.5, 2.9)) and q.pairing == ((0,), (2,)) and q.species is None
    model = make_network(cfg.system, cfg.network)
    assert isinstance(model, Quasihole) and [h[2] for h in model.holes] == ["A", "both", "B"]
    again = Config.from_dict(dataclasses.asdict(cfg))
    assert again.network.quasihole == q and again.network.type == cfg.network.type
    cfg = Config.from_dict({"system": {"nspins": (2, 2), "flux": 8},
                            "network": {"type": "quasihole",
                                        "quasihole": {"holes": [[0.9, -1.0], [2.0, 2.2]], "species": ["up", "down"]}}})
    assert cfg.network.quasihole.species == ("up", "down") and cfg.network.quasihole.base == "halperin"
    assert make_network(cfg.system, cfg.network).exponents == (3, 3, 2)
    assert Config.from_dict({}).network.quasihole == config.QuasiholeNetwork()
    assert Config.from_dict({}).network.quasihole.holes == ()


def test_pretrain_and_overlap_references():
    from deephall_amd import pretrain

    assert "quasihole" in pretrain.REFERENCES
    cfg = Config.from_dict({
        "system": {"nspins": (6, 0), "flux": 16},
        "network": {"quasihole": {"holes": [[1.0, 0.5]]}},
        "optim": {"optimizer": "adam", "pretrain": {"iterations": 5, "reference": "quasihole"}},
    })
    ref = pretrain.make_reference(cfg)
    assert isinstance(ref, Quasihole) and ref.holes == ((1.0, 0.5, "both"),) and ref.exponents == (3, 3, 2)
    cfg.system.flux = 15
    with pytest.raises(ValueError, match="Quasihole"):
        pretrain.make_reference(cfg)
    assert Config.from_dict({}).optim.pretrain.reference == "laughlin"
