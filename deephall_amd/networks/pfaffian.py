"""The Moore-Read Pfaffian state on MI355X (not in the reference).

The paired trial state at even denominator: N even electrons with 2p vortices attached
(p = ``cf_flux``; nu = 1/2 at p = 1).  With u = cos(theta/2) e^(i phi/2),
v = sin(theta/2) e^(-i phi/2) and w_ik = u_i v_k - u_k v_i

    log psi = log Pf(A) + 2p sum_{i<k} log w_ik,      A_ik = 1 / w_ik (i != k),  A_ii = 0

Each electron has degree 2p (N - 1) - 1 in (u, v): the state lives at flux
2Q = 2p (N - 1) - 1 exactly, and any other flux is an error.  No normalisation; the pair part
runs over i < k as for `Jain`.  All N electrons enter the one Pfaffian whatever ``nspins`` says.

``MooreRead`` runs on the kernels of pfaffian.hip through the Psiformer's native plumbing, as
`Laughlin` and `Jain` do (no parameters; dh_logpsi, dh_mcmc_step, dh_local_energy with the
analytic Hessian in double).  ``MooreReadCallable`` is the same state as a float64 torch
log-psi callable: an out-of-place skew elimination with pivoting written in torch operations,
an independent route the tests compare the kernel with; it runs on CPU tensors.
"""

from __future__ import annotations

import math

import torch

from .laughlin import Laughlin, TrialCallable


def check_pfaffian(nspins, flux, cf_flux: int = 1) -> int:
    """N after the checks dh_create repeats."""
    N = sum(int(n) for n in nspins)
    p = int(cf_flux)
    if N < 2 or N % 2:
        raise ValueError(f"Pfaffian: the paired state needs an even number of electrons >= 2, got N = {N}")
    if p < 1:
        raise ValueError(f"Pfaffian: need cf_flux >= 1, got {cf_flux}")
    if int(flux) != 2 * p * (N - 1) - 1:
        raise ValueError(f"Pfaffian: N = {N}, cf_flux = {p} lives at flux 2p(N-1)-1 = {2 * p * (N - 1) - 1}, got {flux}")
    return N


class MooreRead(Laughlin):
    """Parameter-free analytic wavefunction on pfaffian.hip."""

    name = "Moore-Read"
    network_type = "pfaffian"

    def __init__(self, nspins, flux, cf_flux: int = 1, system=None):
        self._sphere(nspins, flux)
        self.cf_flux = int(cf_flux)
        check_pfaffian(self.nspins, self.flux, self.cf_flux)
        self.spec = self._spec(system, cf_flux=self.cf_flux)


def log_pfaffian(A: torch.Tensor) -> torch.Tensor:
    """log Pf of one antisymmetric complex matrix [n, n], n even; the phase is defined modulo
    2 pi.  Skew elimination in 2x2 blocks, out of place: the largest entry of the first row is
    brought to column 1 by a simultaneous row and column swap (a factor -1), the pivot A[0][1]
    is multiplied into Pf and the Schur complement of the leading block carries on.  Only torch
    operations on tensors (argmax, where, matmul), so it runs under torch.func grad / hessian
    and vmap."""
    n = A.shape[-1]
    out = torch.zeros((), dtype=A.dtype, device=A.device)
    while n > 2:
        idx = torch.arange(n, device=A.device)
        j = torch.argmax(torch.abs(A[0, 1:]).detach()) + 1
        perm = torch.where(idx == 1, j, torch.where(idx == j, torch.ones_like(j), idx))
        P = (perm[:, None] == idx[None, :]).to(A.dtype)  # the swap as a 0 / 1 matrix: exact, and batches under vmap
        A = P @ A @ P.T
        out = out + (j != 1).to(A.real.dtype) * (1j * math.pi)
        p = A[0, 1]
        out = out + torch.log(p)
        A = A[2:, 2:] + (A[2:, 0:1] * A[1:2, 2:] - A[2:, 1:2] * A[0:1, 2:]) / p
        n -= 2
    return out + torch.log(A[0, 1])


class MooreReadCallable(TrialCallable):
    """`MooreRead` through `log_pfaffian` (see `TrialCallable`)."""

    def __init__(self, nspins, flux, cf_flux: int = 1, system=None):
        self.nspins = tuple(int(n) for n in nspins)
        self.flux = int(flux)
        self.cf_flux = int(cf_flux)
        self.system = system
        check_pfaffian(self.nspins, self.flux, self.cf_flux)

    @staticmethod
    def pair_matrix(x: torch.Tensor):
        """(A, w): A_ik = 1 / w_ik off the diagonal and 0 on it; w with its diagonal set to 1."""
        x = x.to(torch.float64)
        theta, phi = x[:, 0], x[:, 1]
        u = torch.cos(theta / 2) * torch.exp(0.5j * phi)
        v = torch.sin(theta / 2) * torch.exp(-0.5j * phi)
        eye = torch.eye(x.shape[0], dtype=u.dtype, device=x.device)
        w = u[:, None] * v[None, :] - u[None, :] * v[:, None] + eye
        return (1.0 - eye) / w, w

    def _logpsi(self, x: torch.Tensor) -> torch.Tensor:
        A, w = self.pair_matrix(x)
        pair = torch.sum(torch.triu(torch.log(w), diagonal=1))  # sum_{i<k} log w_ik
        return log_pfaffian(A) + 2 * self.cf_flux * pair


__all__ = ["MooreRead", "MooreReadCallable", "log_pfaffian", "check_pfaffian"]
