"""Energies in the span of K non-orthogonal wavefunctions, on the host in float64 numpy.

Not in the reference.  ``observables/subspace.py`` estimates the overlap matrix S[c, c'] ~
<psi_c | psi_c'> and the Hamiltonian matrix H[c, c'] ~ <psi_c | H | psi_c'> of K states on one set
of walkers; this module solves the generalised eigenproblem H v = E S v for them (composite-fermion
diagonalisation when the states are Jain determinants).  No device call.

The estimated H carries the operator on the ket, H[c, c'] = <conj(r_c) r_c' E_c'>: its exact value
is Hermitian, a finite sample of it is not, and the anti-Hermitian part is pure noise, so ``solve``
works on (H + H^H) / 2 and reports the relative size of what it dropped as ``asymmetry``.  The
states may be linearly dependent (the L = 1 composite-fermion exciton vanishes under projection):
canonical orthogonalisation drops the directions whose eigenvalue of the unit-diagonal S is below
``rank_tol`` times the largest.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np


class Solution(NamedTuple):
    energies: np.ndarray  # [rank] ascending
    vectors: np.ndarray  # [K, rank] complex: H v = E S v in the basis of the states as given
    rank: int
    asymmetry: float  # max |H - H^H| / max |H| of the H passed in
    s_min: float  # the smallest kept eigenvalue of S scaled to a unit diagonal


def _square(M, name: str) -> np.ndarray:
    M = np.asarray(M, dtype=np.complex128)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 1:
        raise ValueError(f"subspace: {name} must be a square matrix, got shape {M.shape}")
    return M


def solve(S, H, rank_tol: float = 1e-8) -> Solution:
    """The energies of H in the span of the states with Gram matrix S.

    Both matrices are Hermitised, (M + M^H) / 2, and scaled by 1 / sqrt(diag S); the eigenvectors of
    the scaled S with an eigenvalue above ``rank_tol`` times the largest span the subspace, H is
    diagonalised in it, and the eigenvectors come back in the original, unscaled basis."""
    S, H = _square(S, "S"), _square(H, "H")
    if S.shape != H.shape:
        raise ValueError(f"subspace: S {S.shape} and H {H.shape} differ in shape")
    if not rank_tol > 0.0:
        raise ValueError(f"subspace: rank_tol must be > 0, got {rank_tol}")
    if not (np.isfinite(S).all() and np.isfinite(H).all()):
        raise ValueError("subspace: S or H has a non-finite entry")
    hmax = np.abs(H).max()
    asymmetry = float(np.abs(H - H.conj().T).max() / hmax) if hmax > 0 else 0.0
    S, H = (S + S.conj().T) / 2, (H + H.conj().T) / 2
    diag = np.diagonal(S).real
    if not (diag > 0).all():
        raise ValueError(f"subspace: S needs a positive diagonal, got {diag}")
    d = 1.0 / np.sqrt(diag)
    Ss, Hs = d[:, None] * S * d[None, :], d[:, None] * H * d[None, :]
    w, U = np.linalg.eigh(Ss)
    keep = w > rank_tol * w[-1]
    X = U[:, keep] / np.sqrt(w[keep])[None, :]  # X^H Ss X = 1
    Hx = X.conj().T @ Hs @ X
    energies, V = np.linalg.eigh((Hx + Hx.conj().T) / 2)
    return Solution(energies, d[:, None] * (X @ V), int(keep.sum()), asymmetry, float(w[keep].min()))


def reprice(S, T, V, strength: float, rank_tol: float = 1e-8) -> Solution:
    """``solve(S, T + strength * V)``: the spectrum with the potential part scaled, from one run's
    kinetic matrix T and potential matrix V = H - T."""
    return solve(S, _square(T, "T") + float(strength) * _square(V, "V"), rank_tol)


def jackknife(steps_S, steps_H, rank_tol: float = 1e-8) -> np.ndarray:
    """Delete-one-step errors of ``solve``'s energies from the per-step matrices [steps, K, K]:
    sqrt((n - 1) / n sum_i (E_(i) - mean E_())^2) with E_(i) from the means without step i.  NaN for
    fewer than 2 steps.  A deleted-step solve of another rank than the full one is an error: its
    energies are not those of the same levels."""
    steps_S, steps_H = np.asarray(steps_S, dtype=np.complex128), np.asarray(steps_H, dtype=np.complex128)
    if steps_S.ndim != 3 or steps_S.shape != steps_H.shape:
        raise ValueError(f"subspace: step matrices must be [steps, K, K] alike, got {steps_S.shape}, {steps_H.shape}")
    n = steps_S.shape[0]
    if n == 0:
        return np.full(0, math.nan)
    full = solve(steps_S.mean(axis=0), steps_H.mean(axis=0), rank_tol)
    if n < 2:
        return np.full(full.rank, math.nan)
    sum_S, sum_H = steps_S.sum(axis=0), steps_H.sum(axis=0)
    E = np.empty((n, full.rank))
    for i in range(n):
        part = solve((sum_S - steps_S[i]) / (n - 1), (sum_H - steps_H[i]) / (n - 1), rank_tol)
        if part.rank != full.rank:
            raise ValueError(f"subspace: the rank is {part.rank} without step {i} and {full.rank} with every step; "
                             "the span is not resolved at this rank_tol (raise it, or evaluate more steps)")
        E[i] = part.energies
    return np.sqrt((n - 1) / n * ((E - E.mean(axis=0)) ** 2).sum(axis=0))


__all__ = ["Solution", "solve", "reprice", "jackknife"]
