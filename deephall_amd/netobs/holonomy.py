"""Overlap matrices to Berry phases and non-Abelian holonomies: float64 host arithmetic.

Not in the reference.  The Gram matrices come from ``observables/hole_overlap.py`` (or are exact);
everything here is small dense linear algebra on the host in complex128.

A path is T steps of M states each (M = 1: one Abelian hole; M > 1: the degenerate pairings of
Moore-Read holes).  With G_st the M x M block of overlaps <a of step s | b of step t>, the states
of a step are orthonormalised by G_tt^(-1/2) and the link between neighbouring steps is

    U_t = G_tt^(-1/2) G_t,t+1 G_t+1,t+1^(-1/2),        W = U_0 U_1 ... U_(T-1),

the last link closing the path back to step 0.  W is the holonomy in the orthonormalised basis of
step 0: unitary as far as the steps span the same space, unchanged when a state of a later step
is rescaled by a complex constant, and conjugated by a unitary when one of step 0 is.  At M = 1
the Berry phase is gamma = -arg W = -arg prod_t O[t, t + 1].

The exact answer to check against: one hole at eta = (theta, phi) acting on n electrons of a
rotationally invariant base is a spin-n/2 coherent state in the hole's spinor U = cos(theta/2)
e^(i phi/2), V = sin(theta/2) e^(-i phi/2), so O(eta, eta') = (conj(U) U' + conj(V) V')^n.  Around
a latitude in T equal steps gamma -> n pi (1 - cos theta) mod 2 pi, n times half the solid angle
(the spinor changes sign once around: the n pi).
"""

from __future__ import annotations

import cmath
import dataclasses
import math

import torch


def _c128(a) -> torch.Tensor:
    return torch.as_tensor(a).to(torch.complex128).cpu()


def overlap_matrix(S) -> torch.Tensor:
    """O = S / sqrt(diag diag^T) of a Gram matrix S [K, K]: the overlaps of the normalised states."""
    S = _c128(S)
    d = torch.sqrt(torch.diagonal(S).real)
    return S / (d[:, None] * d[None, :])


def inv_sqrt(G) -> torch.Tensor:
    """G^(-1/2) of a Hermitian positive block by its eigendecomposition."""
    G = _c128(G)
    w, v = torch.linalg.eigh(0.5 * (G + G.conj().T))
    return (v * (w.to(torch.complex128) ** -0.5)[None, :]) @ v.conj().T


def wilson_loop(G, steps: int, closed: bool = True) -> torch.Tensor:
    """The M x M holonomy of a path of ``steps`` steps of M states.

    ``G``: the Gram matrix [T M, T M] of all states, step-major, or a sequence of one [2 M, 2 M]
    Gram matrix per link, of {states of step t, states of step t + 1} (``steps`` links when closed,
    the last one onto step 0; ``steps - 1`` when not)."""
    T = int(steps)
    nlinks = T if closed else T - 1
    if T < 1 or nlinks < 1:
        raise ValueError(f"wilson_loop: a {'closed' if closed else 'open'} path of {T} steps has no link")
    if isinstance(G, (list, tuple)):
        blocks = [_c128(g) for g in G]
        if len(blocks) != nlinks or any(b.ndim != 2 or b.shape[0] != b.shape[1] or b.shape != blocks[0].shape
                                        or b.shape[0] % 2 for b in blocks):
            raise ValueError(f"wilson_loop: need {nlinks} link blocks [2 M, 2 M]")
    else:
        G = _c128(G)
        if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] % T:
            raise ValueError(f"wilson_loop: G must be [T M, T M] with T = {T}, got {tuple(G.shape)}")
        M = G.shape[0] // T
        idx = [torch.cat([torch.arange(t * M, (t + 1) * M), torch.arange(((t + 1) % T) * M, ((t + 1) % T + 1) * M)])
               for t in range(nlinks)]
        blocks = [G[i][:, i] for i in idx]
    M = blocks[0].shape[0] // 2
    W = torch.eye(M, dtype=torch.complex128)
    for b in blocks:
        W = W @ inv_sqrt(b[:M, :M]) @ b[:M, M:] @ inv_sqrt(b[M:, M:])
    return W


def berry_angle(W) -> float:
    """gamma = -arg det W in (-pi, pi]: the Berry phase at M = 1, the Abelian part of a holonomy."""
    return -cmath.phase(complex(torch.linalg.det(_c128(W))))


def spinor(eta) -> tuple[complex, complex]:
    """(U, V) of a point eta = (theta, phi)."""
    theta, phi = float(eta[0]), float(eta[1])
    return math.cos(theta / 2) * cmath.exp(0.5j * phi), math.sin(theta / 2) * cmath.exp(-0.5j * phi)


def coherent_overlap(eta, eta_prime, n: int) -> complex:
    """<psi_eta | psi_eta'> of the normalised one-hole states on n electrons: (conj(U) U' + conj(V) V')^n."""
    (U, V), (U2, V2) = spinor(eta), spinor(eta_prime)
    return (U.conjugate() * U2 + V.conjugate() * V2) ** int(n)


def latitude_path(theta: float, T: int, phi0: float = 0.0, arc: float = 2.0 * math.pi) -> list:
    """T points (theta, phi0 + arc t / T), t = 0 .. T - 1: a closed latitude for the default arc."""
    return [(float(theta), float(phi0) + float(arc) * t / int(T)) for t in range(int(T))]


def berry_phase(cfg, path, steps: int = 20, burn_in: int = 50, walk_steps: int = 10, closed: bool = False,
                seed: int = 0, device=None):
    """Holonomy of the quasihole state of ``cfg`` (network.type quasihole) along ``path``.

    ``path``: one entry per step, each a configuration ``{holes, species | pairing}`` or a list of M
    of them (the degenerate states of the step).  Step t is sampled from its own first state, so a
    long path stays within reach of the walkers: the network with that state is built, walked for
    ``burn_in`` calls and the ``hole_overlap`` estimator run for ``steps`` steps on {states of step t,
    states of step t + 1}; ``wilson_loop`` chains the links.  Returns {"holonomy" [M, M], "phase"
    (-arg det), "phase_err" (the links' step-scatter errors in quadrature), "links"}."""
    from ..networks import make_network
    from ..random import Key
    from ..train import initalize_state
    from . import DeepHallAdaptor
    from .observables.hole_overlap import HoleOverlapEstimator

    path = [list(p) if isinstance(p, (list, tuple)) else [p] for p in path]
    M, nlinks = len(path[0]), len(path) if closed else len(path) - 1
    blocks, var = [], 0.0
    for t in range(nlinks):
        here, there = path[t], path[(t + 1) % len(path)]
        q = dataclasses.replace(cfg.network.quasihole, **here[0])
        cfg_t = dataclasses.replace(cfg, seed=int(seed) + t, network=dataclasses.replace(cfg.network, quasihole=q))
        adaptor = DeepHallAdaptor()
        adaptor.cfg, adaptor.model = cfg_t, make_network(cfg_t.system, cfg_t.network)
        _, (params, data, _, width) = initalize_state(cfg_t, adaptor.model, device)
        adaptor.batch_per_device = data.shape[0]
        est = HoleOverlapEstimator(adaptor, None, {"configs": here[1:] + there}, None)
        walk, key = adaptor.make_walking_step(None, walk_steps), Key(int(seed) + t)
        values, state = est.empty_val_state(steps)
        for i in range(-burn_in, steps):
            data, _ = walk(key, params, data, {"mcmc_width": width})
            key = key.advance(walk_steps)
            if i >= 0:
                values["gram"][i] = est.evaluate(i, params, None, data, None, state, None)[0]["gram"][0]
        out = est.digest(values, state)
        blocks.append(out["gram"])
        var += float((out["overlap_err"][:M, M:] ** 2).sum() / (out["overlap"][:M, M:].abs() ** 2).sum())
    W = wilson_loop(blocks, len(path), closed)
    return {"holonomy": W, "phase": berry_angle(W), "phase_err": math.sqrt(var), "links": blocks}

