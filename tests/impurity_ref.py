"""A float64 numpy restatement of the impurity potential and of the axis histogram
(deephall_amd/csrc/impurity.hip), for the host and GPU tests.

An impurity is (theta, phi, strength, kind, width, species), the field order of config.Impurity.
Walkers x[B, N, 2] (theta, phi); the slots below nspins[0] are up electrons.  u = r_i . r_a,
c^2 = 2 R^2 (1 - u) (never below 0):
    gaussian  U = strength exp(-c^2 / (2 width^2))
    charge    U = strength / sqrt(c^2 + width^2)
"""

from __future__ import annotations

import math

import numpy as np


def unit(theta, phi):
    theta, phi = np.asarray(theta, np.float64), np.asarray(phi, np.float64)
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=-1)


def fields(imp):
    """(theta, phi, strength, kind, width, species) of a tuple or a config.Impurity."""
    if hasattr(imp, "theta"):
        return imp.theta, imp.phi, imp.strength, imp.kind, imp.width, imp.species
    theta, phi, strength, kind, width, species = imp
    return float(theta), float(phi), float(strength), kind, float(width), species


def potential_of_u(u, strength, kind, width, radius):
    c2 = 2.0 * radius * radius * np.maximum(1.0 - np.asarray(u, np.float64), 0.0)
    if kind == "gaussian":
        return strength * np.exp(-c2 / (2.0 * width * width))
    if kind == "charge":
        return strength / np.sqrt(c2 + width * width)
    raise ValueError(kind)


def per_electron(x, nspins, radius, impurities):
    """U[B, N] float64: sum over the impurities acting on each electron's species."""
    x = np.asarray(x, np.float64)
    B, N, _ = x.shape
    n_up = int(nspins[0])
    r = unit(x[..., 0], x[..., 1])
    out = np.zeros((B, N))
    for imp in impurities:
        theta, phi, strength, kind, width, species = fields(imp)
        U = potential_of_u(r @ unit(theta, phi), strength, kind, width, radius)
        sel = np.ones(N, bool) if species == "both" else (np.arange(N) < n_up) == (species == "up")
        out += U * sel
    return out


def external(x, nspins, radius, impurities):
    """ext[B] float64; NaN for a walker with a non-finite coordinate."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        out = per_electron(x, nspins, radius, impurities).sum(axis=1)
    out[~np.isfinite(x).all(axis=(1, 2))] = np.nan
    return out


def histogram(x, nspins, axis, bins):
    """(counts[2, bins] int64, flagged): bin k is 1 - 2 (k + 1) / bins < u <= 1 - 2 k / bins, the last
    closed at u = -1, NaN dropped.  ``flagged``: the electrons whose u lies within 1e-12 of a bin
    edge 1 - 2 k / bins, k = 0..bins, where a last-bit difference could change the bin."""
    x = np.asarray(x, np.float64)
    B, N, _ = x.shape
    n_up = int(nspins[0])
    with np.errstate(invalid="ignore"):
        u = unit(x[..., 0], x[..., 1]) @ unit(axis[0], axis[1])  # [B, N]
    ok = ~np.isnan(u)
    t = (1.0 - u) * (0.5 * bins)
    k = np.clip(np.floor(np.where(ok, t, 0.0)), 0, bins - 1).astype(np.int64)
    edges = 1.0 - 2.0 * np.arange(bins + 1) / bins
    flagged = int((np.abs(u[ok][:, None] - edges[None, :]).min(axis=1) < 1e-12).sum()) if ok.any() else 0
    counts = np.zeros((2, bins), np.int64)
    up = np.broadcast_to(np.arange(N) < n_up, (B, N))
    np.add.at(counts[0], k[ok & up], 1)
    np.add.at(counts[1], k[ok & ~up], 1)
    return counts, flagged


# ---- the integrals over the sphere ----------------------------------------------------------------

def integral_closed(strength, kind, width, radius):
    """The integral of U over the unit sphere's solid angle."""
    R2 = radius * radius
    if kind == "gaussian":
        return 2.0 * math.pi * strength * (width * width / R2) * (1.0 - math.exp(-2.0 * R2 / (width * width)))
    return 2.0 * math.pi * strength * (math.sqrt(4.0 * R2 + width * width) - width) / R2


def integral_quadrature(strength, kind, width, radius, points=200):
    """The same by Gauss-Legendre in u = cos gamma: 2 pi int_{-1}^{1} U(u) du."""
    u, w = np.polynomial.legendre.leggauss(points)
    return 2.0 * math.pi * float(np.sum(w * potential_of_u(u, strength, kind, width, radius)))


def uniform_mean(nspins, radius, impurities):
    """<sum_i U> of a state of uniform one-body density: n_species int U dOmega / (4 pi) per impurity."""
    total = 0.0
    for imp in impurities:
        _, _, strength, kind, width, species = fields(imp)
        n = {"both": nspins[0] + nspins[1], "up": nspins[0], "down": nspins[1]}[species]
        total += n * integral_closed(strength, kind, width, radius) / (4.0 * math.pi)
    return total


# ---- walkers and impurity lists the tests share ---------------------------------------------------

def walkers(B, N, seed):
    """float32 [B, N, 2]: uniform on the sphere."""
    rng = np.random.default_rng(seed)
    theta = np.arccos(1.0 - 2.0 * rng.random((B, N)))
    phi = 2.0 * math.pi * rng.random((B, N)) - math.pi
    return np.stack([theta, phi], axis=-1).astype(np.float32)


# eight impurities of mixed kinds and species; the first and last sit on the poles
MIXED = (
    (0.0, 0.0, 0.7, "gaussian", 1.3, "both"),
    (1.1, 2.8, -0.4, "charge", 0.5, "up"),
    (2.3, -1.9, 1.2, "gaussian", 0.6, "down"),
    (0.4, 0.3, 0.9, "charge", 2.0, "both"),
    (1.7, 5.1, -1.1, "gaussian", 2.5, "up"),
    (2.9, -0.2, 0.3, "charge", 0.05, "down"),
    (1.3, 1.0, 2.0, "gaussian", 0.2, "both"),
    (math.pi, 0.0, 0.6, "charge", 1.0, "both"),
)


def mixed(K):
    """K of MIXED that always include both poles when K >= 3 (K = 1: the north pole alone)."""
    return {1: MIXED[:1], 3: (MIXED[0], MIXED[1], MIXED[7]), 8: MIXED}[K]
