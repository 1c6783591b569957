"""float64 numpy restatement of the structure-factor kernels (csrc/sfactor.hip), by routes that share
nothing with them: the pair sums through ``numpy.polynomial.legendre.legval`` on the same float32
coordinates upcast, the harmonics through P_L^M = (-1)^M (1 - x^2)^{M/2} d^M P_L / dx^M
(``legder`` / ``legval``) times the exact normalisation from ``math.factorial``.

(1 - x^2)^{M/2} is taken as sin(theta)^M: the same on 0 <= theta <= pi, and the analytic continuation
past it (float32(pi) > pi), where (theta, phi) is the point (2 pi - theta, phi + pi) — the reading
under which cos gamma's formula and the addition theorem hold for such coordinates too.
"""

from __future__ import annotations

import math

import numpy as np
from numpy.polynomial import legendre as NL


def nlm(lmax):
    return (lmax + 1) * (lmax + 2) // 2


def uniform(B, N, seed):
    """float32 walkers [B, N, 2], uniform on the sphere."""
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


def cos_gamma(x):
    """[B, N, N] float64 from float32 walkers [B, N, 2]."""
    th, ph = x[..., 0].astype(np.float64), x[..., 1].astype(np.float64)
    ct, st = np.cos(th), np.sin(th)
    return ct[:, :, None] * ct[:, None, :] + st[:, :, None] * st[:, None, :] * np.cos(ph[:, :, None] - ph[:, None, :])


def pair_sums(x, n_up, lmax, chunk=32, threads=8):
    """T[B, 3, lmax + 1]: sums of P_L(cos gamma_ij) over the pairs i < j both up, up-down, both down.
    Chunks of walkers on a few threads (numpy's loops run without the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor

    B, N, _ = x.shape
    i, j = np.triu_indices(N, 1)
    kind = np.where(j < n_up, 0, np.where(i < n_up, 1, 2))
    T = np.zeros((B, 3, lmax + 1))
    eye = np.eye(lmax + 1)

    def one(b0):
        cg = cos_gamma(x[b0:b0 + chunk])[:, i, j]                    # [b, pairs]
        P = NL.legval(cg, eye)                                       # [lmax + 1, b, pairs]
        for s in range(3):
            T[b0:b0 + chunk, s] = P[:, :, kind == s].sum(-1).T

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(0, B, chunk)))
    return T


def ylm(th, ph, lmax):
    """Y_LM(th, ph) for 0 <= M <= L <= lmax at lm = L (L + 1) / 2 + M: complex128 [..., nlm]."""
    th, ph = np.asarray(th, np.float64), np.asarray(ph, np.float64)
    x, s = np.cos(th), np.sin(th)
    out = np.zeros(th.shape + (nlm(lmax),), np.complex128)
    for L in range(lmax + 1):
        c = np.zeros(L + 1)
        c[L] = 1.0
        for M in range(L + 1):
            d = NL.legval(x, NL.legder(c, M)) if M else NL.legval(x, c)
            norm = math.sqrt((2 * L + 1) / (4 * math.pi) * math.factorial(L - M) / math.factorial(L + M))
            out[..., L * (L + 1) // 2 + M] = norm * (-1) ** M * s**M * d * np.exp(1j * M * ph)
    return out


def multipoles(x, n_up, lmax):
    """rho[B, 2, nlm]: sum of Y_LM over the up and over the down electrons."""
    y = ylm(x[..., 0], x[..., 1], lmax)                              # [B, N, nlm]
    return np.stack([y[:, :n_up].sum(1), y[:, n_up:].sum(1)], 1)


def addition_lhs(rho, lmax):
    """(4 pi / (2L + 1)) (|rho_L0|^2 + 2 sum_{M>0} |rho_LM|^2) of rho[..., nlm] (both species added
    already): [..., lmax + 1].  By the addition theorem it equals N + 2 (T_uu + T_ud + T_dd)."""
    w = np.abs(rho) ** 2
    out = np.zeros(rho.shape[:-1] + (lmax + 1,))
    for L in range(lmax + 1):
        k = L * (L + 1) // 2
        out[..., L] = 4 * math.pi / (2 * L + 1) * (w[..., k] + 2 * w[..., k + 1:k + L + 1].sum(-1))
    return out


def form_factor_quadrature(flux, lmax, points=80):
    """(S(0), [F_1 .. F_lmax]) of the filled lowest level (N = flux + 1) from its pair density
    g(x) proportional to 1 - ((1 + x) / 2)^flux, by Gauss-Legendre quadrature:
    S(L) = 1 + (N - 1) int P_L g / int g = 1 - F_L for L >= 1."""
    xs, ws = NL.leggauss(points)
    g = 1.0 - ((1.0 + xs) / 2.0) ** flux
    norm = np.sum(ws * g)
    S = [1.0 + flux * np.sum(ws * g * NL.legval(xs, np.eye(lmax + 1)[L])) / norm for L in range(lmax + 1)]
    return S[0], [1.0 - s for s in S[1:]]
