"""Exact entanglement of a polar cap for the filled lowest Landau level (free fermions).

A check of the sampling behind ``observables/renyi2.py``, and the known answer its tests pin.
N = 2Q + 1 electrons fill the orbitals Y_{Q,Q,m}, m = -Q..Q, of ``dh_monopole_orbitals``
(|Y|^2 proportional to (1 - cos theta)^(Q - m) (1 + cos theta)^(Q + m)).  The cap theta < theta_a
keeps the rotation about z, so the orbitals stay orthogonal on it and the state factorises over m:
orbital m is inside with probability

    lambda_m = integral over the cap of |Y_{Q,Q,m}|^2 = 1 - I_t(Q + m + 1, Q - m + 1),  t = (1 + cos theta) / 2,

and the regularised incomplete beta function of integer arguments is the finite binomial sum
I_t(a, b) = sum_{j >= a} C(n, j) t^j (1 - t)^(n - j), n = a + b - 1 = 2Q + 1.  Then

    Tr rho_A^2          = prod_m (lambda_m^2 + (1 - lambda_m)^2)
    Tr rho_{A,n}^2      = the coefficient of z^n in prod_m ((1 - lambda_m)^2 + z lambda_m^2)
    P(n electrons in A) = the coefficient of z^n in prod_m ((1 - lambda_m) + z lambda_m).

Plain Python floats (``math.comb``), no scipy; the results come back as numpy arrays.
"""

from __future__ import annotations

import math

import numpy as np


def cap_occupations(flux: int, theta: float) -> list[float]:
    """lambda_m, m = -Q..Q (index k = Q + m = 0..flux), of the cap theta' < theta."""
    n = int(flux) + 1
    t = min(max(0.5 * (1.0 + math.cos(theta)), 0.0), 1.0)
    terms = [math.comb(n, j) * t**j * (1.0 - t) ** (n - j) for j in range(n + 1)]
    # 1 - I_t(k + 1, n - k) = sum_{j <= k} terms[j]: summed upwards, no cancellation
    out, acc = [], 0.0
    for k in range(n):
        acc += terms[k]
        out.append(acc)
    return out


def _poly_product(factors) -> list[float]:
    """Coefficients (ascending powers of z) of prod (c0 + c1 z)."""
    poly = [1.0]
    for c0, c1 in factors:
        nxt = [0.0] * (len(poly) + 1)
        for i, p in enumerate(poly):
            nxt[i] += p * c0
            nxt[i + 1] += p * c1
        poly = nxt
    return poly


def filled_lll_cap(flux: int, thetas):
    """(purity[A], sector_purity[A, N + 1], number_distribution[A, N + 1]) of the filled lowest
    Landau level at flux 2Q = ``flux`` (N = flux + 1 electrons, one spin) for the caps theta < thetas[a]."""
    purity, sector, number = [], [], []
    for theta in thetas:
        lam = cap_occupations(flux, float(theta))
        purity.append(math.prod(x * x + (1.0 - x) * (1.0 - x) for x in lam))
        sector.append(_poly_product(((1.0 - x) * (1.0 - x), x * x) for x in lam))
        number.append(_poly_product((1.0 - x, x) for x in lam))
    return np.asarray(purity), np.asarray(sector), np.asarray(number)
