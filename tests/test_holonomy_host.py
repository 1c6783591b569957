"""Quasihole overlaps and holonomies on the host, float64: netobs/holonomy.py, the validation and
the table of dh_hole_table (no device call), the hole_overlap estimator's options.

The exact answer the GPU tests compare with is pinned here first: one hole on n electrons of a
Laughlin state is a spin-n/2 coherent state, O(eta, eta') = (conj(U) U' + conj(V) V')^n, against an
exact quadrature of `QuasiholeCallable`.  The kernels are tested in test_gpu_holonomy.py."""

from __future__ import annotations

import cmath
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import holonomy_ref as HR
from deephall_amd import Config, _lib
from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS, holonomy as H
from deephall_amd.netobs._native import hole_configs, hole_table
from deephall_amd.netobs.observables import hole_overlap
from deephall_amd.networks.psiformer import NetworkSpec


def test_coherent_overlap_is_the_quadrature():
    """N = 2, m = 1 (flux 2: 18 points per electron): the formula to 1e-14, its conjugate off by > 0.1."""
    for eta, eta2 in (((1.0, 0.0), (1.3, 0.7)), ((0.8, -0.5), (1.5, 0.9)), ((1.0, 0.0), (1.0, 0.6))):
        q = HR.coherent_quadrature(eta, eta2, 2, 1)
        e = H.coherent_overlap(eta, eta2, 2)
        print(eta, eta2, q, e, abs(q - e))
        assert abs(q - e) < 1e-14
        assert abs(q - e.conjugate()) > 0.1
    assert H.coherent_overlap((0.3, 1.0), (0.3, 1.0), 5) == pytest.approx(1.0, abs=1e-15)


def exact_gram(points, n):
    return torch.tensor([[H.coherent_overlap(a, b, n) for b in points] for a in points], dtype=torch.complex128)


def test_wilson_loop_on_a_latitude():
    """Exact coherent-state Gram blocks on the latitude theta = 1, n = 4: gamma is -arg of the exact
    discrete product to 1e-12 at T = 12, and at T = 96 within 1 / T of n pi (1 - cos theta) mod 2 pi:
    a link's phase is n (d/2) cos theta + O(d^3) with d = 2 pi / T, and the closing link carries the
    spinor's sign (-1)^n, so the T links miss the limit by O(1 / T^2) < 1 / T."""
    n, theta = 4, 1.0
    for T in (12, 96):
        path = H.latitude_path(theta, T)
        assert len(path) == T and path[0] == (theta, 0.0) and path[1][1] == pytest.approx(2 * math.pi / T)
        W = H.wilson_loop(exact_gram(path, n), T)
        assert W.shape == (1, 1)
        gamma = H.berry_angle(W)
        prod = 1.0 + 0.0j
        for t in range(T):
            prod *= H.coherent_overlap(path[t], path[(t + 1) % T], n)
        assert abs(math.remainder(gamma + cmath.phase(prod), 2 * math.pi)) < 1e-12
        # the same from the link blocks
        G = exact_gram(path, n)
        links = [G[[t, (t + 1) % T]][:, [t, (t + 1) % T]] for t in range(T)]
        assert abs(H.berry_angle(H.wilson_loop(links, T)) - gamma) < 1e-12
        limit = n * math.pi * (1 - math.cos(theta))
        print(f"T = {T}: gamma {gamma:.6f}, off the limit by {math.remainder(gamma - limit, 2 * math.pi):.2e}")
    assert abs(math.remainder(gamma - limit, 2 * math.pi)) < 1.0 / 96
    # an open path: one link fewer
    open_w = H.wilson_loop(exact_gram(path[:4], n), 4, closed=False)
    want = -sum(cmath.phase(H.coherent_overlap(path[t], path[t + 1], n)) for t in range(3))
    assert abs(H.berry_angle(open_w) - want) < 1e-12
    with pytest.raises(ValueError, match="wilson_loop"):
        H.wilson_loop(exact_gram(path[:4], n), 3)
    with pytest.raises(ValueError, match="wilson_loop"):
        H.wilson_loop(exact_gram(path[:1], n), 1, closed=False)


def test_holonomy_is_unitary_and_scale_invariant():
    """T = 5 steps of M = 2 orthonormal states of one two-dimensional space (a random unitary frame per
    step): every link and the holonomy are unitary to 1e-12; rescaling a state of a later step by a
    complex constant leaves W, rescaling one of step 0 conjugates it (the eigenvalues stay)."""
    rng = np.random.default_rng(5)
    T, M, D = 5, 2, 6
    space = np.linalg.qr(rng.normal(size=(D, M)) + 1j * rng.normal(size=(D, M)))[0]
    frames = [space @ np.linalg.qr(rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M)))[0] for _ in range(T)]
    states = np.concatenate(frames, axis=1)  # [D, T M]
    G = states.conj().T @ states
    W = H.wilson_loop(G, T)
    assert (W @ W.conj().T - torch.eye(M)).abs().max() < 1e-12
    # the frames are bases of one space: the loop closes on the identity
    assert (W - torch.eye(M)).abs().max() < 1e-12
    # non-orthogonal, unnormalised states of the steps: the same holonomy up to the frame of step 0
    mix = [rng.normal(size=(M, M)) + 1j * rng.normal(size=(M, M)) + 2 * np.eye(M) for _ in range(T)]
    mixed = np.concatenate([f @ m for f, m in zip(frames, mix)], axis=1)
    W2 = H.wilson_loop(mixed.conj().T @ mixed, T)
    assert (W2 @ W2.conj().T - torch.eye(M)).abs().max() < 1e-12
    scaled = mixed.copy()
    scaled[:, 2 * M + 1] *= 0.3 - 1.7j
    W3 = H.wilson_loop(scaled.conj().T @ scaled, T)
    assert (W3 - W2).abs().max() < 1e-12
    scaled[:, 0] *= -2.0 + 0.5j
    W4 = H.wilson_loop(scaled.conj().T @ scaled, T)
    ev = lambda w: np.sort_complex(np.linalg.eigvals(w.numpy()))  # noqa: E731
    assert np.abs(ev(W4) - ev(W2)).max() < 1e-12
    # M = 1: any rescaling drops out of the closed loop
    path = H.latitude_path(1.0, 6)
    G1 = exact_gram(path, 3)
    c = torch.tensor([1.0, 2.0 - 1.0j, 0.5j, -3.0, 1.0 + 1.0j, 0.1], dtype=torch.complex128)
    assert (H.wilson_loop(c.conj()[:, None] * G1 * c[None, :], 6) - H.wilson_loop(G1, 6)).abs().max() < 1e-12
    O = H.overlap_matrix(c.conj()[:, None] * G1 * c[None, :])
    assert (torch.diagonal(O) - 1).abs().max() < 1e-15 and (O.abs() - G1.abs()).abs().max() < 1e-15


KINDS = _lib.HOLE_KINDS
TWO = ((1.0, 0.5), (2.0, -1.0))
HOLES4 = ((0.7, 0.3), (1.9, -2.1), (2.6, 1.2), (1.1, 2.8))


def _table(nspins, flux, configs, base=0, expo=(3, 3, 2), p=1, kinds=None, n_configs=None, n_holes=None, ntype="quasihole",
           struct_size=None, hc_size=None, null=None, bytes_=None):
    """(rc, message, table bytes) of dh_hole_table; configs: one tuple of (theta, phi) per configuration,
    kinds: one tuple of names or ints per configuration (default all 'both')."""
    lib = _lib.load()
    cfg = NetworkSpec(nspins=nspins, flux=flux, ndets=1, num_heads=1, heads_dim=4, num_layers=0, network_type=ntype).to_c()
    if struct_size is not None:
        cfg.struct_size = struct_size
    hc = _lib.DhHoleConfigs()
    hc.base = base
    hc.m_up, hc.m_dn, hc.n_inter, hc.p = *expo, p
    hc.n_configs = len(configs) if n_configs is None else n_configs
    hc.n_holes = (len(configs[0]) if configs else 1) if n_holes is None else n_holes
    for c, holes in enumerate(configs[:_lib.DH_HOLE_MAX_CONFIGS]):
        for a, (t, ph) in enumerate(holes):
            hc.holes[c][a][0], hc.holes[c][a][1] = t, ph
            k = kinds[c][a] if kinds is not None else 0
            hc.kind[c][a] = KINDS[k] if isinstance(k, str) else k
    if hc_size is not None:
        hc.struct_size = hc_size
    nbytes = int(lib.dh_hole_table_bytes()) if bytes_ is None else bytes_
    buf = (C.c_uint8 * max(nbytes, 1))()
    rc = lib.dh_hole_table(None if null == "cfg" else C.byref(cfg), None if null == "configs" else C.byref(hc),
                           None if null == "table" else C.cast(buf, C.c_void_p), nbytes)
    return rc, lib.dh_last_error(), bytes(buf)


def test_hole_table_validation():
    """dh_hole_table: the struct sizes, 1 <= K <= 16, every configuration checked as dh_create_quasihole
    checks one (so all at the system's flux), the pointers, the table size; messages start "Holes:"."""
    lib = _lib.load()
    assert C.sizeof(_lib.DhHoleConfigs) == 2592 and lib.dh_hole_table_bytes() == 16 * 8 * (32 + 4) == 4608
    one = ((1.0, 0.5),)
    good = [
        _table((3, 0), 7, [one], expo=(3, 3, 0)),
        _table((3, 0), 7, [one, ((2.0, 0.1),), ((0.0, 0.0),)], expo=(3, 3, 0)),
        _table((2, 2), 8, [TWO, TWO[::-1]], kinds=[("up", "down"), ("down", "up")]),
        _table((2, 2), 8, [one, ((0.3, 0.3),)]),  # a hole on both species
        _table((3, 2), 10, [one], kinds=[("down",)]),
        _table((6, 0), 11, [HOLES4] * 3, base=1, kinds=[("A", "A", "B", "B"), ("A", "B", "A", "B"), ("A", "B", "B", "A")]),
        _table((6, 0), 11, [TWO + ((0.3, 0.3),)] * 2, base=1, kinds=[("A", "B", "both"), ("both", "A", "B")]),
        _table((28, 0), 54, [TWO], base=1, kinds=[("A", "B")]),
        _table((32, 0), 101, [tuple((1.0, 0.1 * a) for a in range(8))] * 16, expo=(3, 3, 0)),
    ]
    for rc, msg, _ in good:
        assert rc == 0, msg
    bad = {
        "K = 0": _table((3, 0), 7, [], expo=(3, 3, 0)),
        "K = 17": _table((3, 0), 7, [one] * 17, expo=(3, 3, 0), n_configs=17),
        "K = -1": _table((3, 0), 7, [one], expo=(3, 3, 0), n_configs=-1),
        "another flux": _table((2, 2), 8, [one, one], kinds=[("both",), ("up",)]),  # down 3 + 4 + 0 = 7
        "unequal groups": _table((6, 0), 11, [HOLES4] * 2, base=1, kinds=[("A", "A", "B", "B"), ("A", "A", "A", "B")]),
        "groups to Abelian holes": _table((6, 0), 11, [HOLES4] * 2, base=1, kinds=[("A", "A", "B", "B"), ("A", "B", "both", "both")]),
        "nan angle": _table((3, 0), 7, [one, ((float("nan"), 0.0),)], expo=(3, 3, 0)),
        "inf angle": _table((3, 0), 7, [((1.0, float("inf")),)], expo=(3, 3, 0)),
        "theta > pi": _table((3, 0), 7, [one, ((3.2, 0.0),)], expo=(3, 3, 0)),
        "kind of the other base": _table((3, 0), 7, [one, one], expo=(3, 3, 0), kinds=[("both",), ("A",)]),
        "kind 5": _table((3, 0), 7, [one], expo=(3, 3, 0), kinds=[(5,)]),
        "no holes": _table((3, 0), 6, [one], expo=(3, 3, 0), n_holes=0),
        "nine holes": _table((4, 0), 18, [one], expo=(3, 3, 0), n_holes=9),
        "base 2": _table((3, 0), 7, [one], base=2, expo=(3, 3, 0)),
        "even m_up": _table((3, 0), 5, [one], expo=(2, 3, 0)),
        "pfaffian N = 30": _table((30, 0), 58, [TWO], base=1, kinds=[("A", "B")]),
        "N = 33": _table((33, 0), 97, [one], expo=(3, 3, 0)),
        "type mismatch": _table((3, 0), 7, [one], expo=(3, 3, 0), ntype="halperin"),
        "dh_config size": _table((3, 0), 7, [one], expo=(3, 3, 0), struct_size=56),
        "dh_hole_configs size": _table((3, 0), 7, [one], expo=(3, 3, 0), hc_size=2588),
        "null cfg": _table((3, 0), 7, [one], expo=(3, 3, 0), null="cfg"),
        "null configs": _table((3, 0), 7, [one], expo=(3, 3, 0), null="configs"),
        "null table": _table((3, 0), 7, [one], expo=(3, 3, 0), null="table"),
        "short table": _table((3, 0), 7, [one], expo=(3, 3, 0), bytes_=4607),
    }
    for why, (rc, msg, _) in bad.items():
        assert rc == -1, why  # DH_EINVAL
        assert msg.startswith(b"Holes:"), (why, msg)
    assert b"configuration 1" in bad["another flux"][1] and b"= 7" in bad["another flux"][1]
    assert b"configuration 1" in bad["unequal groups"][1] and b"configuration 1" in bad["nan angle"][1]
    assert b"struct_size" in bad["dh_hole_configs size"][1] and b"2592" in bad["dh_hole_configs size"][1]
    # the device calls check the same before any launch: no GPU here
    one_f, null = C.c_void_p(64), C.c_void_p(0)
    cfg = NetworkSpec(nspins=(3, 0), flux=7, ndets=1, num_heads=1, heads_dim=4, num_layers=0, network_type="quasihole").to_c()
    hc = hole_configs(HR.states(*[HR.CASES["laughlin3-K3"][i] for i in (0, 2)]))
    bad_hc = hole_configs(HR.states(*[HR.CASES["laughlin3-K3"][i] for i in (0, 2)]))
    bad_hc.holes[2][0][0] = float("nan")
    for rc in (
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), null, 8, one_f, 4608, one_f, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), one_f, 8, null, 4608, one_f, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), one_f, 8, one_f, 4608, null, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), one_f, 0, one_f, 4608, one_f, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), one_f, 8, one_f, 4607, one_f, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(hc), one_f, 2**30, one_f, 4608, one_f, None),
        lib.dh_hole_logs(C.byref(cfg), C.byref(bad_hc), one_f, 8, one_f, 4608, one_f, None),
        lib.dh_hole_logs(None, C.byref(hc), one_f, 8, one_f, 4608, one_f, None),
        lib.dh_hole_gram(null, 8, 3, one_f, one_f, one_f, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 3, null, one_f, one_f, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 3, one_f, null, one_f, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 3, one_f, one_f, null, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 3, one_f, one_f, one_f, null, 1 << 20, None),
        lib.dh_hole_gram(one_f, 0, 3, one_f, one_f, one_f, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 0, one_f, one_f, one_f, one_f, 1 << 20, None),
        lib.dh_hole_gram(one_f, 8, 17, one_f, one_f, one_f, one_f, 1 << 20, None),
    ):
        assert rc == -1 and lib.dh_last_error().startswith(b"Holes:"), lib.dh_last_error()
    assert lib.dh_hole_gram(one_f, 8, 3, one_f, one_f, one_f, one_f, 16, None) == -3  # DH_ENOMEM
    assert lib.dh_hole_workspace_bytes(257, 3) >= 257 * 3 * 16 + 257 * 4
    for B, K in ((0, 3), (8, 0), (8, 17), (2**30, 16)):
        assert lib.dh_hole_workspace_bytes(B, K) == 0, (B, K)


@pytest.mark.parametrize("name", ["laughlin3-K3", "halperin22-up-down", "pfaffian6-pairings", "laughlin32-8holes-K16"])
def test_table_holds_the_spinors_of_the_handle(name):
    """uv of configuration c is what dh_create_quasihole computes, (cos(th/2) cos(ph/2), cos(th/2) sin(ph/2),
    sin(th/2) cos(ph/2), -sin(th/2) sin(ph/2)): the Python formula to 1 ulp; the kinds; -1 and 0 where unused."""
    system, _, configs = HR.CASES[name]
    states = HR.states(system, configs)
    spec = NetworkSpec(nspins=system["nspins"], flux=system["flux"], ndets=1, num_heads=1, heads_dim=4, num_layers=0,
                       network_type="quasihole")
    tab = hole_table(spec, states)
    K, nh = len(configs), len(configs[0]["holes"])
    assert tab.n_configs == K and tab.n_holes == nh and tab.spinors.shape == (K, nh, 2)
    raw = tab.host[:4096].view(torch.float64).reshape(16, 8, 4).numpy()
    kinds = tab.host[4096:].view(torch.int32).reshape(16, 8).numpy()
    for c, st in enumerate(states):
        for a, (th, ph, kind) in enumerate(st[3]):
            want = np.array([math.cos(th / 2) * math.cos(ph / 2), math.cos(th / 2) * math.sin(ph / 2),
                             math.sin(th / 2) * math.cos(ph / 2), -math.sin(th / 2) * math.sin(ph / 2)])
            assert np.all(np.abs(raw[c, a] - want) <= np.spacing(np.abs(want))), (c, a)
            assert kinds[c, a] == KINDS[kind] == tab.kinds[c, a]
    assert np.all(raw[K:] == 0) and np.all(raw[:, nh:] == 0) and np.all(kinds[K:] == -1) and np.all(kinds[:, nh:] == -1)
    with pytest.raises(ValueError, match="Holes"):
        hole_configs(states + [HR.states(dict(nspins=(3, 0), flux=8, exponents=HR.L0), [dict(holes=(HR.G1, HR.G2))])[0]])
    with pytest.raises(RuntimeError, match="Holes: need 1 <= n_configs"):
        hole_table(spec, [])


def test_uniform_walkers_stay_clear_of_the_exclusion():
    """The GPU test drops walkers whose smallest |w| or |s| is below 1e-3: at most 2 % of any case."""
    for name, (system, B, configs) in HR.CASES.items():
        x = HR.uniform(B, sum(system["nspins"]), seed=B + sum(system["nspins"]))
        d = HR.smallest_distance(x, configs)
        assert (d < 1e-3).mean() <= 0.02, name
        L = HR.logs(system, configs, x)
        assert L.shape == (B, len(configs)) and np.isfinite(L.real).all() and np.isfinite(L.imag).all()


def test_gram_restatement_drops_non_finite_walkers():
    rng = np.random.default_rng(1)
    L = rng.uniform(-3, 3, (7, 3)) + 1j * rng.uniform(-9, 9, (7, 3))
    S, mag, n = HR.gram(L)
    assert n == 7 and np.allclose(S, S.conj().T) and S[0, 0] == pytest.approx(7.0)
    L2 = np.concatenate([L, [[np.nan, 0, 0], [0, np.inf, 0]]])
    S2, _, n2 = HR.gram(L2)
    assert n2 == 7 and np.array_equal(S2, S)
    S3, _, _ = HR.gram(L, shift=[0.0, 0.5, -1.0])
    assert np.allclose(S3, S * np.exp(-np.add.outer([0.0, 0.5, -1.0], [0.0, 0.5, -1.0])), rtol=1e-13)


def _cfg(**network):
    return Config.from_dict({"batch_size": 8, "system": {"nspins": (4, 0), "flux": 10},
                             "network": {"type": "quasihole", "halperin": {"exponents": [3, 3, 0]}, **network}})


def test_estimator_options_and_registry():
    assert ESTIMATORS["hole_overlap"] is EXTRA_ESTIMATORS["hole_overlap"] is hole_overlap.DEFAULT
    assert EXTRA_ESTIMATORS.more["hole_overlap"] is hole_overlap.HoleOverlapEstimator
    assert "hole_overlap" not in list(ESTIMATORS) and "hole_overlap" not in list(EXTRA_ESTIMATORS)
    cfg = _cfg(quasihole={"holes": [[1.0, 0.0]]})
    adaptor = types.SimpleNamespace(cfg=cfg)
    est = hole_overlap.HoleOverlapEstimator(adaptor, None, {"configs": [{"holes": [[1.0, 0.3]]}, {"holes": [[1.0, 0.6]]}]}, {})
    assert est.K == 3 and est.states[0] == ("halperin", (3, 3, 0), 1, ((1.0, 0.0, "both"),))
    assert [s[3][0][:2] for s in est.states] == [(1.0, 0.0), (1.0, 0.3), (1.0, 0.6)]
    assert est.table.n_configs == 3 and est.table.nelec == 4
    vals, state = est.empty_val_state(5)
    assert vals["gram"].shape == (5, 3, 3) and vals["gram"].dtype == torch.complex128 and state == {"shift": None}
    assert hole_overlap.HoleOverlapEstimator(adaptor, None, None, None).K == 1  # the network's own state alone
    # the digest on exact step values: the overlaps, the links and zero scatter
    pts = [(1.0, 0.0), (1.0, 0.3), (1.0, 0.6)]
    G = exact_gram(pts, 4) * 2.5
    out = est.digest({"gram": G[None].repeat(4, 1, 1), "walkers": torch.full((4,), 8.0)}, state)
    assert (out["overlap"] - exact_gram(pts, 4)).abs().max() < 1e-15
    assert out["berry_links"].tolist() == pytest.approx([cmath.phase(H.coherent_overlap(pts[c], pts[c + 1], 4)) for c in (0, 1)])
    assert out["gram_err"].abs().max() == 0 and out["overlap_err"].abs().max() < 1e-15 and out["walkers"] == 32
    assert out["berry_links_err"].abs().max() < 1e-15
    # pairings of the pfaffian base inherit the holes
    pf = Config.from_dict({"batch_size": 8, "system": {"nspins": (6, 0), "flux": 11},
                           "network": {"type": "quasihole", "quasihole": {"base": "pfaffian", "holes": [list(h) for h in HOLES4],
                                                                          "pairing": [[0, 1], [2, 3]]}}})
    est = hole_overlap.HoleOverlapEstimator(types.SimpleNamespace(cfg=pf), None,
                                            {"configs": [{"pairing": [[0, 2], [1, 3]]}, {"pairing": [[0, 3], [1, 2]]}]}, {})
    assert [tuple(h[2] for h in s[3]) for s in est.states] == [("A", "A", "B", "B"), ("A", "B", "A", "B"), ("A", "B", "B", "A")]
    assert est.table.kinds.tolist() == [[3, 3, 4, 4], [3, 4, 3, 4], [3, 4, 4, 3]]
    for options, match in (
        ({"configs": {"holes": [[1.0, 0.3]]}}, "configs must be a list"),
        ({"configs": [[[1.0, 0.3]]]}, "must be a dict"),
        ({"configs": [{"hole": [[1.0, 0.3]]}]}, "must be a dict"),
        ({"configs": [{"holes": [[1.0, 0.3], [2.0, 0.1]]}]}, "configuration 1: Quasihole"),  # another flux
        ({"configs": [{"holes": [[4.0, 0.3]]}]}, "configuration 1: Quasihole"),
        ({"configs": [{"holes": [[1.0, 0.1 * c]]} for c in range(16)]}, "n_configs"),  # 17 with the network's own
    ):
        with pytest.raises(ValueError, match=match):
            hole_overlap.HoleOverlapEstimator(adaptor, None, options, {})
    for ntype in ("laughlin", "halperin", "psiformer"):
        other = Config.from_dict({"batch_size": 8, "system": {"nspins": (2, 2), "flux": 7}, "network": {"type": ntype}})
        with pytest.raises(ValueError, match="hole_overlap: the network must be 'quasihole'"):
            hole_overlap.HoleOverlapEstimator(types.SimpleNamespace(cfg=other), None, {}, {})
