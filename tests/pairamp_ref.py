"""Float64 numpy restatement of the pair-amplitude estimator (csrc/pairamp.hip,
netobs/observables/pair_amplitude.py, netobs/pseudopotential.py).

* ``pair_kernel``: the closed form (4 pi)^2 K_L = n_L d^(2Q - L) p_L with p_L from its recurrence;
  ``pair_kernel_sum`` the same with p_L from the explicit sum over binomials;
* ``pair_kernel_orbitals``: the orbital route, K_L = sum_M Phi_LM conj(Phi_LM), Phi_LM the products of
  ``oracle.netobs.lll_orbitals`` coupled by the eigenvectors of (L1 + L2)^2 in each M sector;
* ``accumulate``: the sums over samples and pairs by class, with the drop rule;
* ``legendre_moments``: <P_k>_L of the highest-weight pair state by Gauss-Legendre in cos theta_1,
  cos theta_2 and a uniform rule in phi_1 - phi_2.
"""

from __future__ import annotations

import numpy as np
from scipy import special as ss

from oracle import netobs as O


def uniform(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


def spinor(r):
    """(u, v) of points r[..., 2] = (theta, phi): the gauge of oracle.netobs.monopole_harm."""
    r = np.asarray(r, dtype=np.float64)
    th, ph = r[..., 0], r[..., 1]
    return np.cos(th / 2) * np.exp(0.5j * ph), np.sin(th / 2) * np.exp(-0.5j * ph)


def bracket(p, q):
    return p[0] * np.conj(q[0]) + p[1] * np.conj(q[1])


def geometry(r1, r2, r1p, r2p):
    """(a, b, d) of the pair (r1, r2) and the primed pair; d = w12 conj(w1'2'), exactly 0 at r1 = r2."""
    s1, s2, t1, t2 = spinor(r1), spinor(r2), spinor(r1p), spinor(r2p)
    a = bracket(s1, t1) * bracket(s2, t2)
    b = bracket(s1, t2) * bracket(s2, t1)
    return a, b, wedge(s1, s2) * np.conj(wedge(t1, t2))


def wedge(p, q):
    """u_p v_q - v_p u_q from real products, each rounded before it is added: exactly 0 at p = q."""
    (pu, pv), (qu, qv) = p, q
    re = (pu.real * qv.real - pu.imag * qv.imag) - (pv.real * qu.real - pv.imag * qu.imag)
    im = (pu.real * qv.imag + pu.imag * qv.real) - (pv.imag * qu.real + pv.real * qu.imag)
    return re + 1j * im


def norms(flux):
    """n_L, L = 0..flux."""
    L = np.arange(flux + 1)
    lb = lambda n, k: ss.gammaln(n + 1.0) - ss.gammaln(k + 1.0) - ss.gammaln(n - k + 1.0)  # noqa: E731
    return (flux + 1.0) ** 2 * (2 * L + 1.0) / (flux + L + 1.0) * np.exp(lb(flux, L) - lb(flux + L, L))


def p_recurrence(a, b, d, flux):
    """p_L[..., flux + 1] by (L + 1) p_{L+1} = (2L + 1)(a + b) p_L - L d^2 p_{L-1}."""
    p = np.zeros(np.shape(a) + (flux + 1,), dtype=np.complex128)
    p[..., 0] = 1.0
    if flux >= 1:
        p[..., 1] = a + b
    for L in range(1, flux):
        p[..., L + 1] = ((2 * L + 1) * (a + b) * p[..., L] - L * d * d * p[..., L - 1]) / (L + 1)
    return p


def p_sum(a, b, flux):
    """p_L = sum_j C(L, j)^2 a^(L - j) b^j."""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    out = np.zeros(a.shape + (flux + 1,), dtype=np.complex128)
    for L in range(flux + 1):
        j = np.arange(L + 1)
        out[..., L] = np.sum(ss.comb(L, j) ** 2 * a[..., None] ** (L - j) * b[..., None] ** j, -1)
    return out


def d_powers(d, flux):
    """d^(flux - L), L = 0..flux, by multiplication (0^0 = 1)."""
    pw = np.ones(np.shape(d) + (flux + 1,), dtype=np.complex128)
    for L in range(flux - 1, -1, -1):
        pw[..., L] = pw[..., L + 1] * d
    return pw


def pair_kernel(r1, r2, r1p, r2p, flux):
    """(4 pi)^2 K_L [..., flux + 1] complex128, the closed form with the recurrence."""
    a, b, d = geometry(r1, r2, r1p, r2p)
    return norms(flux) * d_powers(d, flux) * p_recurrence(a, b, d, flux)


def pair_kernel_sum(r1, r2, r1p, r2p, flux):
    a, b, d = geometry(r1, r2, r1p, r2p)
    return norms(flux) * d_powers(d, flux) * p_sum(a, b, flux)


def coupling(flux):
    """U[L][M index][m1 index]: for each L the coefficients <m1, M - m1 | L M> (up to a phase per
    (L, M), which K_L does not see) from the eigenvectors of (L1 + L2)^2 in every M sector.
    A list over L of lists of (M, m1 values, coefficients)."""
    Q = flux / 2
    ms = np.arange(-Q, Q + 1)
    out = [[] for _ in range(flux + 1)]
    for M in np.arange(-flux, flux + 1):
        m1 = np.array([m for m in ms if -Q <= M - m <= Q])
        m2 = M - m1
        n = len(m1)
        # (L1 + L2)^2 = L1^2 + L2^2 + 2 L1z L2z + L1+ L2- + L1- L2+
        H = np.diag(2 * Q * (Q + 1) + 2 * m1 * m2)
        for k in range(n - 1):  # m1 -> m1 + 1, m2 -> m2 - 1
            off = np.sqrt(Q * (Q + 1) - m1[k] * (m1[k] + 1)) * np.sqrt(Q * (Q + 1) - m2[k] * (m2[k] - 1))
            H[k, k + 1] = H[k + 1, k] = off
        vals, vecs = np.linalg.eigh(H)
        for e, vec in zip(vals, vecs.T):
            L = int(round((-1 + np.sqrt(1 + 4 * e)) / 2))
            out[L].append((M, m1, vec))
    return out


def pair_kernel_orbitals(r1, r2, r1p, r2p, flux):
    """(4 pi)^2 K_L by the orbital route; points [n, 2]."""
    Q = flux / 2
    y1, y2, z1, z2 = (O.lll_orbitals(np.asarray(r, dtype=np.float64), flux) for r in (r1, r2, r1p, r2p))
    out = np.zeros((y1.shape[0], flux + 1), dtype=np.complex128)
    for L, states in enumerate(coupling(flux)):
        for M, m1, vec in states:
            i1 = np.round(m1 + Q).astype(int)
            i2 = np.round(M - m1 + Q).astype(int)
            phi = np.sum(vec * y1[:, i1] * y2[:, i2], -1)
            phip = np.sum(vec * z1[:, i1] * z2[:, i2], -1)
            out[:, L] += phi * np.conj(phip)
    return (4 * np.pi) ** 2 * out


def pair_list(N):
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


def pair_class(i, j, n_up):
    return 0 if j < n_up else (1 if i < n_up else 2)


def displace(x, r1, r2, pair0=0, pair1=None):
    """xp[pair1 - pair0, P, B, N, 2] from x[B, N, 2], r1, r2 [P, B, 2]."""
    B, N, _ = x.shape
    pairs = pair_list(N)[pair0:pair1]
    xp = np.broadcast_to(x, (len(pairs), r1.shape[0], B, N, 2)).copy()
    for k, (i, j) in enumerate(pairs):
        xp[k, :, :, i] = r1
        xp[k, :, :, j] = r2
    return xp


def accumulate(x, r1, r2, lp, lpp, n_up, flux):
    """(A[3, flux + 1] complex128, the sum over the kept samples; the number kept) from x[B, N, 2],
    r1, r2 [P, B, 2], lp[B, 2] and lpp[pairs P B, 2] float32 (re, im)."""
    B, N, _ = x.shape
    P = r1.shape[0]
    pairs = pair_list(N)
    c = lambda a: a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.exp(c(lpp).reshape(len(pairs), P, B) - c(lp)[None, None, :])
    keep = np.isfinite(ratio).all(0) & np.isfinite(c(lp))[None, :]  # [P, B]
    A = np.zeros((3, flux + 1), dtype=np.complex128)
    for q, (i, j) in enumerate(pairs):
        K = pair_kernel(x[None, :, i], x[None, :, j], r1, r2, flux)  # [P, B, flux + 1]
        A[pair_class(i, j, n_up)] += np.sum(np.where(keep, ratio[q], 0.0)[..., None] * K, axis=(0, 1))
    return A, int(keep.sum())


def legendre_moments(flux):
    """M[k, L] = <P_k(cos gamma_12)>_L, k, L = 0..flux, in the highest-weight pair state of total L:
    density ((1 - cos gamma) / 2)^(2Q - L) ((1 + x1) / 2)^L ((1 + x2) / 2)^L.  Times P_k it is a
    polynomial of degree <= flux - L + k <= 2 flux in cos(phi) and <= flux + k <= 2 flux in x1 and in
    x2 (odd powers of the square root drop out in the phi sum), so flux + 2 Gauss-Legendre nodes
    (exact to degree 2 flux + 3) and 2 flux + 2 angles are exact."""
    xs, ws = np.polynomial.legendre.leggauss(flux + 2)
    nphi = 2 * flux + 2
    cphi = np.cos(2 * np.pi * np.arange(nphi) / nphi)
    x1, x2, cp = xs[:, None, None], xs[None, :, None], cphi[None, None, :]
    cg = x1 * x2 + np.sqrt((1 - x1 * x1) * (1 - x2 * x2)) * cp
    w = (ws[:, None, None] * ws[None, :, None] / nphi) * np.ones_like(cg)
    Pk = np.stack([ss.eval_legendre(k, cg) for k in range(flux + 1)])
    M = np.zeros((flux + 1, flux + 1))
    for L in range(flux + 1):
        rho = w * ((1 - cg) / 2) ** (flux - L) * ((1 + x1) / 2) ** L * ((1 + x2) / 2) ** L
        M[:, L] = np.sum(Pk * rho, axis=(1, 2, 3)) / np.sum(rho)
    return M
