"""Haldane pseudopotentials on the sphere, host side, float64.

A pair interaction v(cos gamma) = sum_k v_k P_k(cos gamma) acts inside the lowest Landau level only
through V_L = sum_{k <= 2Q} v_k <P_k>_L, its expectation in a pair state of total angular momentum
L (relative angular momentum m = 2Q - L): multipoles above 2Q drop out exactly.  With the pair
amplitudes A_L of the ``pair_amplitude`` estimator the interaction energy of a lowest-level state is
sum_L V_L A_L.

<P_k>_L is the same for every M of the multiplet, so it is the mean of P_k over the multiplet's
rotation-invariant pair density, a function of x = cos gamma alone:

    rho_L(x) = ((1 - x) / 2)^(2Q - L) p_L(1, (1 + x) / 2),

the diagonal of the projector of csrc/pairamp.hip (a = 1, b = |<1|2>|^2, d = 1 - b), p_L from its
recurrence.  rho_L P_k is a polynomial of degree <= 2Q + k <= 4Q: Gauss-Legendre on 2Q + 2 nodes is
exact.  Every term is positive, so nothing cancels.
"""

from __future__ import annotations

import numpy as np


def _legendre(kmax: int, x: np.ndarray) -> np.ndarray:
    """P_k(x), k = 0..kmax: [kmax + 1, len(x)]."""
    P = np.ones((kmax + 1, x.size))
    if kmax >= 1:
        P[1] = x
    for k in range(1, kmax):
        P[k + 1] = ((2 * k + 1) * x * P[k] - k * P[k - 1]) / (k + 1)
    return P


def _check_flux(flux) -> int:
    if int(flux) != flux or not 0 <= flux <= 126:
        raise ValueError(f"pseudopotential: flux must be an integer in 0..126, got {flux!r}")
    return int(flux)


def pair_legendre_moments(flux: int) -> np.ndarray:
    """M[k, L] = <P_k(cos gamma_12)>_L for k, L = 0..flux; M[0] = 1."""
    flux = _check_flux(flux)
    x, w = np.polynomial.legendre.leggauss(flux + 2)
    b = (1 + x) / 2
    d = 1 - b
    p = np.ones((flux + 1, x.size))  # p_L(1, b)
    if flux >= 1:
        p[1] = 1 + b
    for L in range(1, flux):
        p[L + 1] = ((2 * L + 1) * (1 + b) * p[L] - L * d * d * p[L - 1]) / (L + 1)
    rho = np.stack([d ** (flux - L) * p[L] for L in range(flux + 1)]) * w  # [L, nodes]
    return (_legendre(flux, x) @ rho.T) / rho.sum(-1)


def pseudopotentials(flux: int, v_k) -> np.ndarray:
    """V_L, L = 0..flux, of v(cos gamma) = sum_k v_k P_k(cos gamma); coefficients past k = flux are ignored."""
    flux = _check_flux(flux)
    v = np.zeros(flux + 1)
    v_k = np.asarray(v_k, dtype=np.float64).reshape(-1)[:flux + 1]
    v[:v_k.size] = v_k
    return v @ pair_legendre_moments(flux)


def coulomb_pseudopotentials(flux: int, radius: float) -> np.ndarray:
    """V_L of the chord Coulomb interaction 1 / (R sqrt(2 - 2 cos gamma)) = (1 / R) sum_k P_k(cos gamma)."""
    flux = _check_flux(flux)
    if not radius > 0:
        raise ValueError(f"pseudopotential: radius must be positive, got {radius!r}")
    return pseudopotentials(flux, np.full(flux + 1, 1.0 / float(radius)))


def harmonic_pseudopotentials(flux: int) -> np.ndarray:
    """V_L of the ``harmonic`` interaction 1 + (Q + 1) / Q cos gamma: L (L + 1) / (2Q (Q + 1))."""
    flux = _check_flux(flux)
    if flux < 1:
        raise ValueError("pseudopotential: the harmonic interaction needs flux >= 1")
    Q = flux / 2
    return pseudopotentials(flux, [1.0, (Q + 1) / Q])


def interaction_energy(A, V):
    """sum_L V_L A_L over the last axis of A[..., flux + 1] (numpy in, numpy out)."""
    A, V = np.asarray(A), np.asarray(V, dtype=np.float64)
    if A.shape[-1] != V.shape[-1]:
        raise ValueError(f"interaction_energy: {A.shape[-1]} amplitudes, {V.shape[-1]} pseudopotentials")
    return A @ V


__all__ = ["pair_legendre_moments", "pseudopotentials", "coulomb_pseudopotentials", "harmonic_pseudopotentials",
           "interaction_energy"]
