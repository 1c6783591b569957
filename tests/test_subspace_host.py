"""The subspace estimator on the host: netobs/subspace.py (solve, reprice, jackknife) in float64,
the estimator's options and registry entry, and the argument checks of dh_subspace_accumulate, which
come before any launch (no device call here).  The kernel is tested in test_gpu_subspace.py."""

from __future__ import annotations

import ctypes as C
import math
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from deephall_amd import Config, _lib
from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS, subspace as SS
from deephall_amd.netobs.observables import subspace as est_mod
from deephall_amd.networks import Halperin, Jain, Laughlin

ROOT = Path(__file__).resolve().parents[1]
K = 5


def pencil(seed, duplicate=None):
    """(S, H, H0, Cmat): S = C^H C and H = C^H H0 C of a random Hermitian H0 and a random complex C."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(K, K)) + 1j * rng.normal(size=(K, K))
    H0 = (A + A.conj().T) / 2
    Cmat = rng.normal(size=(K, K)) + 1j * rng.normal(size=(K, K))
    if duplicate is not None:
        Cmat[:, duplicate[1]] = Cmat[:, duplicate[0]]
    return Cmat.conj().T @ Cmat, Cmat.conj().T @ H0 @ Cmat, H0, Cmat


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solver_on_a_full_rank_pencil(seed):
    S, H, H0, Cmat = pencil(seed)
    assert np.linalg.cond(Cmat) < 1e3  # invertible, and far from the rank cut
    sol = SS.solve(S, H)
    want = np.linalg.eigvalsh(H0)
    assert sol.rank == K and sol.energies.shape == (K,) and sol.vectors.shape == (K, K)
    assert np.all(np.diff(sol.energies) > 0)
    assert np.abs(sol.energies - want).max() <= 1e-10 * np.abs(want).max()
    resid = H @ sol.vectors - (S @ sol.vectors) * sol.energies[None, :]
    assert np.abs(resid).max() <= 1e-10 * np.abs(H).max() * np.abs(sol.vectors).max()
    assert sol.asymmetry < 1e-14  # H is Hermitian to rounding
    # the scaling of the states drops out of the energies, and comes back in the vectors
    scale = np.array([1.0, 1e3, 1e-3, 2.0 - 1.0j, 0.5j])
    sol2 = SS.solve(scale.conj()[:, None] * S * scale[None, :], scale.conj()[:, None] * H * scale[None, :])
    assert np.abs(sol2.energies - want).max() <= 1e-10 * np.abs(want).max()


def test_hermitised_and_asymmetry():
    """An anti-Hermitian addition to H changes nothing but `asymmetry`, which reports it from the raw H."""
    S, H, H0, _ = pencil(3)
    rng = np.random.default_rng(4)
    N = rng.normal(size=(K, K)) + 1j * rng.normal(size=(K, K))
    anti = 0.01 * (N - N.conj().T)
    sol, noisy = SS.solve(S, H), SS.solve(S, H + anti)
    assert np.abs(sol.energies - noisy.energies).max() < 1e-10 * np.abs(sol.energies).max()
    assert noisy.asymmetry == pytest.approx(np.abs(2 * anti).max() / np.abs(H + anti).max(), rel=1e-12)
    assert noisy.asymmetry > 1e-4


def test_rank_deficiency():
    S, H, H0, Cmat = pencil(5, duplicate=(1, 3))
    sol = SS.solve(S, H)
    assert sol.rank == K - 1 and sol.energies.shape == (K - 1,) and sol.vectors.shape == (K, K - 1)
    Q = np.linalg.qr(np.delete(Cmat, 3, axis=1))[0]  # the column space
    want = np.linalg.eigvalsh(Q.conj().T @ H0 @ Q)
    assert np.abs(sol.energies - want).max() <= 1e-10 * np.abs(want).max()
    resid = H @ sol.vectors - (S @ sol.vectors) * sol.energies[None, :]
    assert np.abs(resid).max() <= 1e-10 * np.abs(H).max() * np.abs(sol.vectors).max()
    assert sol.s_min > 1e-8  # the kept directions are well away from the cut
    # a rank_tol above every eigenvalue but the largest keeps one direction
    assert SS.solve(S, H, rank_tol=0.999).rank == 1
    with pytest.raises(ValueError, match="rank_tol"):
        SS.solve(S, H, rank_tol=0.0)
    with pytest.raises(ValueError, match="square"):
        SS.solve(S[:, :3], H)
    with pytest.raises(ValueError, match="non-finite"):
        SS.solve(S * math.nan, H)


@pytest.mark.parametrize("s", [0.0, 0.4, 2.5])
def test_repricing(s):
    S, T, _, _ = pencil(6)
    _, V, _, _ = pencil(7)
    a, b = SS.reprice(S, T, V, s), SS.solve(S, T + s * V)
    assert a.rank == b.rank and np.array_equal(a.energies, b.energies) and np.array_equal(a.vectors, b.vectors)
    if s == 0.0:
        assert np.array_equal(a.energies, SS.solve(S, T).energies)


def test_jackknife():
    """K = 1, S = 1: the energy is the step mean of H, so the jackknife is its standard error, by hand:
    H = 1, 2, 6 -> the means without a step 4, 3.5, 1.5 (mean 3), sqrt(2/3 (1 + 0.25 + 2.25)) = sqrt(7/3).
    K = 2, diagonal: the same per level, the levels sorted."""
    ones = np.ones((3, 1, 1))
    err = SS.jackknife(ones, np.array([1.0, 2.0, 6.0]).reshape(3, 1, 1))
    assert err.shape == (1,) and err[0] == pytest.approx(math.sqrt(7.0 / 3.0), rel=1e-14)
    assert err[0] == pytest.approx(np.std([1.0, 2.0, 6.0], ddof=1) / math.sqrt(3), rel=1e-14)
    S2 = np.broadcast_to(np.diag([2.0, 0.5]), (3, 2, 2)).copy()
    H2 = np.stack([np.diag([2.0 * h, 0.5 * g]) for h, g in zip((1.0, 2.0, 6.0), (-10.0, -11.0, -12.0))])
    err2 = SS.jackknife(S2, H2)
    assert err2 == pytest.approx([1.0 / math.sqrt(3), math.sqrt(7.0 / 3.0)], rel=1e-13)  # ascending: -11, then 3
    # fewer than 2 steps: NaN, one per level
    one = SS.jackknife(S2[:1], H2[:1])
    assert one.shape == (2,) and np.isnan(one).all()
    assert SS.jackknife(S2[:0], H2[:0]).shape == (0,)
    # a step without which the span loses a direction
    S3 = np.stack([np.ones((2, 2)), np.ones((2, 2)), np.array([[1.0, 0.0], [0.0, 1.0]])]).astype(complex)
    with pytest.raises(ValueError, match="rank is 1 without step 2"):
        SS.jackknife(S3, S3.copy())
    with pytest.raises(ValueError, match="alike"):
        SS.jackknife(S2, H2[:2])


def _cfg(ntype="jain", **network):
    return Config.from_dict({"batch_size": 8, "system": {"nspins": (4, 0), "flux": 9},
                             "network": {"type": ntype, **network}})


GROUND = [[0, -1.5], [0, -0.5], [0, 0.5], [0, 1.5]]


def test_estimator_options_and_registry():
    assert ESTIMATORS["subspace"] is EXTRA_ESTIMATORS["subspace"] is est_mod.DEFAULT is est_mod.SubspaceEstimator
    assert EXTRA_ESTIMATORS.more["subspace"] is est_mod.SubspaceEstimator
    assert list(EXTRA_ESTIMATORS) == ["renyi2"] and list(ESTIMATORS) == ["density", "pair_corr", "overlap", "one_rdm"]
    assert callable(SS.solve)  # netobs.subspace is the solver, not the estimator's module
    adaptor = types.SimpleNamespace(cfg=_cfg(jain={"occupation": GROUND}))
    exciton = [[0, -0.5], [0, 0.5], [0, 1.5], [1, 0.5]]
    est = est_mod.SubspaceEstimator(adaptor, None, {"states": [
        {"type": "laughlin"}, {"type": "jain", "jain": {"occupation": exciton}},
        {"type": "halperin", "halperin": {"exponents": [3, 3, 0]}}, {"type": "jain"}], "strengths": [0.5, 2]}, {})
    assert est.K == 5 and est.rank_tol == 1e-8 and est.strengths == [0.5, 2.0]
    assert [type(n) for n in est.networks] == [Jain, Laughlin, Jain, Halperin, Jain]
    assert est.networks[2].occupation == tuple((n, m) for n, m in exciton)
    assert est.networks[4].occupation == est.networks[0].occupation  # what an entry does not name: cfg.network's
    assert all(n.spec.flux == 9 and n.spec.nspins == (4, 0) for n in est.networks)
    vals, state = est.empty_val_state(7)
    assert state == {"shift": None} and vals["walkers"].shape == (7,)
    for k in ("gram", "hamiltonian", "kinetic"):
        assert vals[k].shape == (7, 5, 5) and vals[k].dtype == torch.complex128
    assert est_mod.SubspaceEstimator(adaptor, None, None, None).K == 1  # the run's own state alone
    # state 0 is the adaptor's own network when it has one
    own = types.SimpleNamespace(cfg=adaptor.cfg, model=object())
    assert est_mod.SubspaceEstimator(own, None, {}, {}).networks[0] is own.model
    for options, match in (
        ({"states": [{"type": "psiformer"}]}, "state 1 is a psiformer"),
        ({"states": [{"type": "laughlin"}, {"type": "slater"}]}, "state 2 has the unknown type 'slater'"),
        ({"states": [{"type": "laughlin"}] * 32}, "at most 32 states"),
        ({"rank_tol": 0.0}, "rank_tol must be > 0"),
        ({"rank_tol": -1e-8}, "rank_tol must be > 0"),
        ({"states": {"type": "laughlin"}}, "states must be a list"),
        ({"states": ["laughlin"]}, "must be a dict"),
        ({"states": [{"jain": {}}]}, "must be a dict"),
        ({"states": [{"type": "jain", "occupation": exciton}]}, "must be a dict"),
        ({"states": [{"type": "jain", "jain": {"levels": 2}}]}, "state 1: "),
        ({"states": [{"type": "jain", "jain": {"occupation": exciton[:3]}}]}, "state 1: Jain"),
        ({"states": [{"type": "pfaffian"}]}, "state 1: "),  # no Moore-Read state at this flux
    ):
        with pytest.raises(ValueError, match=match):
            est_mod.SubspaceEstimator(adaptor, None, options, {})
    assert est_mod.SubspaceEstimator(adaptor, None, {"states": [{"type": "laughlin"}] * 31}, {}).K == 32
    # strengths rescale H - T: that must be the pair interaction and nothing else
    free = _cfg(jain={"occupation": GROUND})
    free.system.interaction_strength = 0.0
    with pytest.raises(ValueError, match="strengths"):
        est_mod.SubspaceEstimator(types.SimpleNamespace(cfg=free), None, {"strengths": [1.0]}, {})


def test_digest_on_exact_steps():
    """Step values made from an exact pencil: the digest's energies are the pencil's, V = H - T, NaN steps
    are left out, and energies@s is the spectrum of T + (s / strength) V."""
    cfg = _cfg(jain={"occupation": GROUND})
    cfg.system.interaction_strength = 2.0
    est = est_mod.SubspaceEstimator(types.SimpleNamespace(cfg=cfg), None,
                                    {"states": [{"type": "laughlin"}] * (K - 1), "strengths": [2.0, 0.5]}, {})
    S, H, H0, _ = pencil(8)
    _, T, _, _ = pencil(9)
    nan = np.full((K, K), complex(math.nan, math.nan))
    steps = {"gram": torch.tensor(np.stack([S, nan, S, S])), "hamiltonian": torch.tensor(np.stack([H, H, H, H])),
             "kinetic": torch.tensor(np.stack([T, T, T, T])), "walkers": torch.tensor([8.0, 0.0, 8.0, 7.0])}
    out = est.digest(steps, {"shift": None})
    want = np.linalg.eigvalsh(H0)
    assert out["rank"] == K and out["steps"] == 3 and out["walkers"] == 23.0
    assert np.abs(out["energies"].numpy() - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(out["energies_err"].numpy()).max() <= 1e-10 * np.abs(want).max()  # identical steps
    assert torch.equal(out["potential"], out["hamiltonian"] - out["kinetic"])
    assert np.array_equal(out["gram"].numpy(), np.stack([S, S, S]).mean(axis=0))
    assert (torch.diagonal(out["overlap"]) - 1).abs().max() < 1e-15
    V = out["vectors"].numpy()
    assert np.abs(H @ V - (S @ V) * out["energies"].numpy()[None, :]).max() <= 1e-9 * np.abs(H).max() * np.abs(V).max()
    assert np.abs(out["energies@2"].numpy() - want).max() <= 1e-10 * np.abs(want).max()  # the run's own strength
    quarter = SS.solve(S, T + 0.25 * (H - T)).energies
    assert np.abs(out["energies@0.5"].numpy() - quarter).max() <= 1e-10 * np.abs(quarter).max()
    none = est.digest({k: v[1:2] for k, v in steps.items()}, {"shift": None})
    assert none["rank"] == 0 and none["steps"] == 0 and none["energies"].shape == (0,)
    assert torch.isnan(none["gram"].real).all()


def test_accumulate_arguments():
    """dh_subspace_accumulate: DH_EINVAL with a message before any launch."""
    lib = _lib.load()
    p, null, big = C.c_void_p(64), C.c_void_p(0), 1 << 20

    def call(logs=p, e_l=p, ke=p, B=8, Kc=3, shift=p, out=p, nvalid=p, ws=p, nbytes=big):
        rc = lib.dh_subspace_accumulate(logs, e_l, ke, B, Kc, shift, out, nvalid, ws, nbytes, None)
        return rc, lib.dh_last_error()

    bad = {"K = 0": call(Kc=0), "K = 33": call(Kc=33), "K = -1": call(Kc=-1), "B = 0": call(B=0),
           "K B = 2^31": call(B=2**26, Kc=32, nbytes=2**62),
           "short workspace": call(nbytes=int(lib.dh_subspace_workspace_bytes(8, 3)) - 1)}
    for name in ("logs", "e_l", "ke", "shift", "out", "nvalid", "ws"):
        bad[f"null {name}"] = call(**{name: null})
    for why, (rc, msg) in bad.items():
        assert rc == -1, why  # DH_EINVAL
        assert msg.startswith(b"subspace:") and len(msg) > len(b"subspace: "), (why, msg)
    assert b"null pointer" in bad["null shift"][1] and b"workspace" in bad["short workspace"][1]
    assert b"2^31" in bad["K B = 2^31"][1] and b"K outside" in bad["K = 33"][1] and b"B < 1" in bad["B = 0"][1]
    # ratio [K][B] double2 and valid [B] int32
    assert lib.dh_subspace_workspace_bytes(257, 3) >= 257 * 3 * 16 + 257 * 4
    assert lib.dh_subspace_workspace_bytes(1, 1) >= 20 and lib.dh_subspace_workspace_bytes(2**26 - 1, 32) > 0
    for B, Kc in ((0, 3), (8, 0), (8, 33), (2**26, 32)):
        assert lib.dh_subspace_workspace_bytes(B, Kc) == 0, (B, Kc)


def test_header_and_exports_list_the_symbols():
    txt = (ROOT / "include" / "deephall_amd.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(dh_\w+)\(", txt, re.M))
    lib = _lib.load()
    for sym in ("dh_subspace_workspace_bytes", "dh_subspace_accumulate"):
        assert sym in declared and sym in _lib.EXPORTS and hasattr(lib, sym)
    assert "#define DH_SUBSPACE_MAX_STATES 32" in txt and _lib.DH_SUBSPACE_MAX_STATES == 32
