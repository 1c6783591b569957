"""Float64 numpy restatement of the Renyi-2 swap estimator's classify, swap and reduce steps
(csrc/swap.hip), written walker by walker from the definition; the tests' reference.

Walkers x[B, N, 2] float32; pair p = (walker p, walker p + P), P = B // 2; region a is the cap
x[..., 0] < float32(theta_a), the float32 comparison on the stored value; slots below n_up are up.
"""

from __future__ import annotations

import numpy as np


def classify(x, thetas, nspins):
    """sector[A, P] int32 (-1: unmatched) and counts[A, K] int64 (the sectors of all 2 P members)."""
    x = np.asarray(x, np.float32)
    n_up, n_dn = nspins
    P, A, K = x.shape[0] // 2, len(thetas), (n_up + 1) * (n_dn + 1)
    sector = np.full((A, P), -1, np.int32)
    counts = np.zeros((A, K), np.int64)
    for a, theta in enumerate(thetas):
        inside = x[..., 0] < np.float32(theta)                     # [B, N]
        k = inside[:, :n_up].sum(-1) * (n_dn + 1) + inside[:, n_up:].sum(-1)
        for p in range(P):
            counts[a, k[p]] += 1
            counts[a, k[p + P]] += 1
            if k[p] == k[p + P]:
                sector[a, p] = k[p]
    return sector, counts


def swapped(r1, r2, theta, n_up):
    """(R1', R2') of a matched pair: in-A coordinates exchanged in ascending slot order per spin."""
    o1, o2 = r1.copy(), r2.copy()
    N = r1.shape[0]
    for lo, hi in ((0, n_up), (n_up, N)):
        i1 = [i for i in range(lo, hi) if r1[i, 0] < np.float32(theta)]
        i2 = [i for i in range(lo, hi) if r2[i, 0] < np.float32(theta)]
        assert len(i1) == len(i2)
        for s1, s2 in zip(i1, i2):
            o1[s1] = r2[s2]
            o2[s2] = r1[s1]
    return o1, o2


def compact(x, thetas, nspins, sector):
    """(M, start[A + 1], pair[M], xs[2 M, N, 2]) in flattened (a-major, then p) order."""
    x = np.asarray(x, np.float32)
    A, P = sector.shape
    start, pair, rows = [0], [], []
    for a in range(A):
        for p in range(P):
            if sector[a, p] >= 0:
                r1, r2 = swapped(x[p], x[p + P], thetas[a], nspins[0])
                pair.append(a * P + p)
                rows += [r1, r2]
        start.append(len(pair))
    xs = np.stack(rows) if rows else np.zeros((0, *x.shape[1:]), np.float32)
    return len(pair), np.asarray(start, np.int32), np.asarray(pair, np.int32), xs.astype(np.float32)


def reduce(logpsi, logpsi_s, nspins, pair, sector):
    """(sums[A, K] complex128, mags[A, K] = the sum of |terms|) from complex logs of x and of xs."""
    logpsi = np.asarray(logpsi, np.complex128)
    logpsi_s = np.asarray(logpsi_s, np.complex128)
    A, P = sector.shape
    K = (nspins[0] + 1) * (nspins[1] + 1)
    sums = np.zeros((A, K), np.complex128)
    mags = np.zeros((A, K))
    for o, idx in enumerate(pair):
        a, p = divmod(int(idx), P)
        v = np.exp(logpsi_s[2 * o] + logpsi_s[2 * o + 1] - logpsi[p] - logpsi[p + P])
        sums[a, sector[a, p]] += v
        mags[a, sector[a, p]] += abs(v)
    return sums, mags


def swap_sums(logpsi_fn, x, thetas, nspins):
    """The whole estimator with ``logpsi_fn(rows float64 [n, N, 2]) -> complex log psi [n]``."""
    sector, counts = classify(x, thetas, nspins)
    M, start, pair, xs = compact(x, thetas, nspins, sector)
    lp = logpsi_fn(np.asarray(x, np.float64))
    lps = logpsi_fn(xs.astype(np.float64)) if M else np.zeros(0, np.complex128)
    sums, _ = reduce(lp, lps, nspins, pair, sector)
    return sums, counts, M
