"""numpy / torch float64 restatement of the quasihole overlap kernels (csrc/quasihole.hip
hole_logs_kernel, csrc/holes.hip), for test_holonomy_host.py and test_gpu_holonomy.py.

Logs come from `QuasiholeCallable` on the float32-rounded walkers, Gram sums from plain numpy.
A case is a system and a list of hole configurations `{holes, species | pairing}`."""

from __future__ import annotations

import math

import numpy as np
import torch

from deephall_amd.networks import QuasiholeCallable
from deephall_amd.networks.quasihole import check_quasihole

L0 = (3, 3, 0)  # Laughlin 1/3 on nspins (N, 0)
G1, G2, G3, G4 = (0.7, 0.3), (1.9, -2.1), (2.6, 1.2), (1.1, 2.8)  # generic points
PAIRINGS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))


def _ring(k, n=8):
    """n holes on a tilted ring, configuration k"""
    return tuple((0.4 + 0.3 * a + 0.01 * k, -3.0 + 0.7 * a + 0.05 * k) for a in range(n))


# the cases of test_gpu_holonomy.py (a) and (b): name -> (system and base, B, configurations)
CASES = {
    "laughlin3-K1": (dict(nspins=(3, 0), flux=7, exponents=L0), 5, [dict(holes=(G1,))]),
    "laughlin3-K3": (dict(nspins=(3, 0), flux=7, exponents=L0), 5,
                     [dict(holes=(G1,)), dict(holes=(G2,)), dict(holes=((0.0, 0.0),))]),
    "halperin22-up-down": (dict(nspins=(2, 2), flux=8), 257,
                           [dict(holes=(G1, G2), species=("up", "down")), dict(holes=(G3, G4), species=("up", "down")),
                            dict(holes=(G2, G1), species=("down", "up"))]),
    "halperin32-down": (dict(nspins=(3, 2), flux=10), 5,
                        [dict(holes=(G3,), species=("down",)), dict(holes=(G4,), species=("down",))]),
    "pfaffian6-pairings": (dict(nspins=(6, 0), flux=11, base="pfaffian"), 257,
                           [dict(holes=(G1, G2, G3, G4), pairing=p) for p in PAIRINGS]),
    "pfaffian2": (dict(nspins=(2, 0), flux=2, base="pfaffian"), 3,
                  [dict(holes=(G1, G2), pairing=((0,), (1,))), dict(holes=(G3, G4), pairing=((1,), (0,)))]),
    "pfaffian28": (dict(nspins=(28, 0), flux=54, base="pfaffian"), 3,
                   [dict(holes=(G1, G2), pairing=((0,), (1,))), dict(holes=(G3, G2), pairing=((0,), (1,)))]),
    "laughlin32-8holes-K16": (dict(nspins=(32, 0), flux=101, exponents=L0), 3, [dict(holes=_ring(k)) for k in range(16)]),
}


def uniform(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


def callables(system, configs):
    return [QuasiholeCallable(**system, **c) for c in configs]


def states(system, configs):
    """`check_quasihole`'s tuples, what `_native.hole_table` takes"""
    return [check_quasihole(system["nspins"], system["flux"], system.get("base", "halperin"), c["holes"],
                            c.get("species"), c.get("pairing"), system.get("exponents", (3, 3, 2)),
                            system.get("cf_flux", 1)) for c in configs]


def logs(system, configs, x) -> np.ndarray:
    """L[B, K] complex128: log psi_c of the float32 walkers x, in float64"""
    xd = torch.as_tensor(np.asarray(x, dtype=np.float32)).double()
    return np.stack([m(None, xd).numpy() for m in callables(system, configs)], axis=1)


def spinors(points):
    th, ph = np.asarray(points, dtype=np.float64).T
    return np.cos(th / 2) * np.exp(0.5j * ph), np.sin(th / 2) * np.exp(-0.5j * ph)


def smallest_distance(x, configs) -> np.ndarray:
    """[B]: the smallest |w_ik| between two electrons and |s_a(i)| between an electron and any hole"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    u, v = np.cos(x[..., 0] / 2) * np.exp(0.5j * x[..., 1]), np.sin(x[..., 0] / 2) * np.exp(-0.5j * x[..., 1])
    w = np.abs(u[:, :, None] * v[:, None, :] - u[:, None, :] * v[:, :, None])
    w = w + 10.0 * np.eye(x.shape[1])
    out = w.reshape(len(x), -1).min(axis=1)
    for c in configs:
        U, V = spinors(c["holes"])
        s = np.abs(u[:, :, None] * V[None, None, :] - v[:, :, None] * U[None, None, :])
        out = np.minimum(out, s.reshape(len(x), -1).min(axis=1))
    return out


def deviation(L, L_ref):
    """(Re deviation relative to max(1, |Re|), wrapped phase deviation), each [B, K]"""
    re = np.abs(L.real - L_ref.real) / np.maximum(1.0, np.abs(L_ref.real))
    im = np.abs(np.angle(np.exp(1j * (L.imag - L_ref.imag))))
    return re, im


def gram(L, shift=None):
    """(S[K, K], sum of |terms| [K, K], nvalid): the sums dh_hole_gram forms, over the walkers whose logs are finite"""
    L = np.asarray(L, dtype=np.complex128)
    K = L.shape[1]
    shift = np.zeros(K) if shift is None else np.asarray(shift, dtype=np.float64)
    ok = np.isfinite(L.real).all(axis=1) & np.isfinite(L.imag).all(axis=1)
    Lv = L[ok]
    r = np.exp(Lv - Lv[:, :1] - shift[None, :])
    S = np.einsum("bc,bd->cd", r.conj(), r)
    mag = np.einsum("bc,bd->cd", np.abs(r), np.abs(r))
    return S, mag, int(ok.sum())


def coherent_quadrature(eta, eta2, N, m):
    """<psi_eta | psi_eta'> / sqrt(<eta|eta> <eta'|eta'>) of one hole on Laughlin 1/m with N electrons by exact
    quadrature over all electrons: Gauss-Legendre in cos theta, the trapezoid rule in phi (exact for the
    trigonometric polynomials the integrands are made of: degree flux = m (N - 1) + 1 per electron)."""
    flux = m * (N - 1) + 1
    n_theta, n_phi = flux + 1, 2 * flux + 2
    ct, wt = np.polynomial.legendre.leggauss(n_theta)
    phi = 2 * np.pi * np.arange(n_phi) / n_phi
    th1, ph1 = np.meshgrid(np.arccos(ct), phi, indexing="ij")
    w1 = (wt[:, None] * np.full(n_phi, 2 * np.pi / n_phi)[None, :]).ravel()
    pts = np.stack([th1.ravel(), ph1.ravel()], -1)  # [P, 2]
    P = len(pts)
    idx = np.stack(np.meshgrid(*[np.arange(P)] * N, indexing="ij"), -1).reshape(-1, N)
    x = torch.as_tensor(pts[idx])  # [P^N, N, 2] float64
    weight = np.prod(w1[idx], axis=1)
    a = QuasiholeCallable((N, 0), flux, holes=(eta,), exponents=(m, m, 0))(None, x).numpy()
    b = QuasiholeCallable((N, 0), flux, holes=(eta2,), exponents=(m, m, 0))(None, x).numpy()
    pa, pb = np.exp(a), np.exp(b)
    ab = np.sum(weight * pa.conj() * pb)
    return ab / math.sqrt(np.sum(weight * np.abs(pa) ** 2).real * np.sum(weight * np.abs(pb) ** 2).real)


def case_walkers(name):
    """The uniform float32 walkers of a case: [B, N, 2], the same on every call"""
    system, B, _ = CASES[name]
    N = sum(system["nspins"])
    return uniform(B, N, seed=B + N)


def normalised_spectrum(S):
    """Ascending eigenvalues of the normalised Gram matrix S / sqrt(diag diag^T)"""
    d = np.sqrt(np.diagonal(S).real)
    return np.linalg.eigvalsh(S / np.outer(d, d))
