"""Float64 numpy restatement of the total-spin estimator (csrc/spin.hip), written from the
definition; the tests' reference.

Walkers x[B, N, 2]; the slots below n_up are up.  Pair p = i n_dn + (j - n_up) of an up slot i and
a down slot j, P = n_up n_dn pairs; R_p is the walker with the coordinates of i and j exchanged and

    S^2_loc(R) = ((n_up - n_dn) / 2)^2 + N / 2 - sum_p psi(R_p) / psi(R).

A walker with a non-finite log or ratio is left out of every sum and of nvalid.
"""

from __future__ import annotations

import numpy as np


def pair_slots(nspins):
    """[(i, j)] in pair order."""
    n_up, n_dn = nspins
    return [(i, n_up + d) for i in range(n_up) for d in range(n_dn)]


def exchange_rows(x, nspins, pair0=0, pair1=None):
    """xs[pair1 - pair0, B, N, 2]: copies of x with the two slots of each pair exchanged."""
    x = np.asarray(x)
    slots = pair_slots(nspins)[pair0:pair1]
    xs = np.empty((len(slots), *x.shape), x.dtype)
    for k, (i, j) in enumerate(slots):
        xs[k] = x
        xs[k, :, i] = x[:, j]
        xs[k, :, j] = x[:, i]
    return xs


def as_complex(lp):
    """Complex log psi from a complex array or from float [..., 2] (re, im) pairs, in float64."""
    lp = np.asarray(lp)
    if np.iscomplexobj(lp):
        return lp.astype(np.complex128)
    return lp[..., 0].astype(np.float64) + 1j * lp[..., 1].astype(np.float64)


def ratios(logpsi, logpsi_s):
    """r[P, B] = exp(logpsi_s - logpsi), NaN where a log or the ratio is not finite."""
    lp, lps = as_complex(logpsi), as_complex(logpsi_s)
    with np.errstate(all="ignore"):
        d = lps - lp[None, :]
        r = np.exp(d.real) * (np.cos(d.imag) + 1j * np.sin(d.imag))
    ok = np.isfinite(lp.real) & np.isfinite(lp.imag)
    ok = ok[None, :] & np.isfinite(lps.real) & np.isfinite(lps.imag) & np.isfinite(r.real) & np.isfinite(r.imag)
    return np.where(ok, r, np.nan + 1j * np.nan)


def spin_square(logpsi, logpsi_s, nspins):
    """(s2[B] complex128, NaN for an invalid walker; pairs[n_up, n_dn], the valid walkers' sums of
    each pair's ratio; total, their sum of s2; nvalid) from logpsi [B] and logpsi_s [P, B] (complex,
    or float pairs [..., 2])."""
    n_up, n_dn = nspins
    lp = as_complex(logpsi)
    B, P = lp.shape[0], n_up * n_dn
    r = ratios(lp, as_complex(logpsi_s).reshape(P, B)) if P else np.zeros((0, B), np.complex128)
    valid = np.isfinite(lp.real) & np.isfinite(lp.imag) & np.isfinite(r.real).all(0) & np.isfinite(r.imag).all(0)
    c0 = ((n_up - n_dn) / 2) ** 2 + (n_up + n_dn) / 2
    s2 = np.where(valid, c0 - r.sum(0), np.nan + 1j * np.nan)
    pairs = np.where(valid[None, :], r, 0).sum(1).reshape(n_up, n_dn)
    return s2, pairs, s2[valid].sum(), int(valid.sum())


def spin_square_of(logpsi_fn, x, nspins):
    """spin_square with ``logpsi_fn(rows float64 [n, N, 2]) -> complex log psi [n]``, plus the
    logs themselves: (s2, pairs, total, nvalid, logpsi [B], logpsi_s [P, B])."""
    x = np.asarray(x, np.float64)
    B, N, _ = x.shape
    xs = exchange_rows(x, nspins)
    lp = np.asarray(logpsi_fn(x), np.complex128)
    lps = np.asarray(logpsi_fn(xs.reshape(-1, N, 2)), np.complex128).reshape(-1, B) if len(xs) else np.zeros((0, B), np.complex128)
    return (*spin_square(lp, lps, nspins), lp, lps)


def float32_log_bound(logpsi, logpsi_s):
    """What storing the logs in float32 can move S^2_loc of each walker: with relative rounding
    2^-24 per stored float, |delta S^2_b| <= 2 * 2^-23 sum_p |r_p| (|log psi(R_p)| + |log psi(R_b)|),
    the factor 2 covering the real and the imaginary parts."""
    lp, lps = as_complex(logpsi), as_complex(logpsi_s)
    r = np.abs(np.exp(lps - lp[None, :]))
    return 2 * 2.0**-23 * (r * (np.abs(lps) + np.abs(lp)[None, :])).sum(0)
