"""Jain composite-fermion states with two Lambda levels on MI355X (not in the reference).

N electrons at flux 2Q with 2p vortices attached (p = ``cf_flux``) see the reduced monopole
Q1 = Q - p (N - 1).  An occupation is a list of N distinct composite-fermion orbitals (n, m),
Lambda level n in {0, 1}, m in {-Q1 - n, ..., Q1 + n}; with A = Q1 + m, B = Q1 - m,
u = cos(theta/2) e^(i phi/2), v = sin(theta/2) e^(-i phi/2) and w_ik = u_i v_k - u_k v_i

    log psi = log det E + 2p sum_{i<k} log w_ik,      one column of E per orbital, in order:
    n = 0:  E_i = u_i^A v_i^B
    n = 1:  E_i = (A + 1) u_i^A v_i^(B+1) Dv_i - (B + 1) u_i^(A+1) v_i^B Du_i,
            Du_i = p sum_{k != i} v_k / w_ik,   Dv_i = -p sum_{k != i} u_k / w_ik

(the lowest-Landau-level projected second-level orbital: at p = 1 the quasiparticle column of
networks/laughlin.py).  No normalisation; the column order is part of the definition.  The
default occupation is the ground state with both levels filled, N = 4 Q1 + 4 (nu = 2/5 at
p = 1, 2/9 at p = 2): all of level 0, then all of level 1, m ascending.

``Jain`` runs on the kernels of cf.hip through the Psiformer's native plumbing, as `Laughlin`
does (no parameters; dh_logpsi, dh_mcmc_step, dh_local_energy with the analytic Hessian in
double).  ``JainCallable`` is the same state as a float64 torch log-psi callable through
``slogdet``: an independent route the tests compare the kernel with; it runs on CPU tensors.
All N electrons enter one determinant whatever ``nspins`` says.
"""

from __future__ import annotations

import torch

from .laughlin import Laughlin, TrialCallable, laughlin_q1


def default_occupation(nspins, flux, cf_flux: int = 1) -> tuple:
    """Both Lambda levels filled: N = 4 Q1 + 4."""
    N = sum(nspins)
    q2 = int(flux) - 2 * int(cf_flux) * (N - 1)  # 2 Q1
    if q2 < 0 or N != 2 * q2 + 4:
        raise ValueError(f"Jain: no ground state of two filled levels for N = {N}, 2 Q1 = {q2} (needs N = 4 Q1 + 4)")
    return tuple((n, m2 / 2) for n in (0, 1) for m2 in range(-q2 - 2 * n, q2 + 2 * n + 1, 2))


def check_occupation(nspins, flux, cf_flux, occupation) -> tuple:
    """((n, 2 m), ...) in integers after the checks dh_create_cf repeats."""
    N = sum(nspins)
    q2 = int(flux) - 2 * int(cf_flux) * (N - 1)
    if q2 < 0:
        raise ValueError("Jain: flux too small for N electrons (Q1 < 0)")
    if len(occupation) != N:
        raise ValueError(f"Jain: the occupation needs one orbital per electron, got {len(occupation)} for N = {N}")
    out = []
    for n, m in occupation:
        m2 = round(2 * float(m))
        if int(n) not in (0, 1):
            raise ValueError(f"Jain: Lambda level must be 0 or 1, got {n}")
        if abs(2 * float(m) - m2) > 1e-9 or (m2 - q2) % 2:
            raise ValueError(f"Jain: m = {m} is not Q1 = {q2 / 2} plus an integer")
        if abs(m2) > q2 + 2 * int(n):
            raise ValueError(f"Jain: |m| = {abs(m)} > Q1 + n = {q2 / 2 + int(n)}")
        if (int(n), m2) in out:
            raise ValueError(f"Jain: orbital ({n}, {m}) occupied twice")
        out.append((int(n), m2))
    return tuple(out)


class Jain(Laughlin):
    """Parameter-free analytic wavefunction on cf.hip."""

    name = "Jain"
    network_type = "jain"

    def __init__(self, nspins, flux, cf_flux: int = 1, occupation=None, system=None):
        self._sphere(nspins, flux)
        self.cf_flux = int(cf_flux)
        self.Q1 = laughlin_q1(self.nspins, self.flux, self.cf_flux)
        if occupation is None:
            self.occupation = default_occupation(self.nspins, self.flux, self.cf_flux)
            occ2 = None  # dh_create builds the same table
        else:
            occ2 = check_occupation(self.nspins, self.flux, self.cf_flux, occupation)
            self.occupation = tuple((n, m2 / 2) for n, m2 in occ2)
        self.spec = self._spec(system, cf_flux=self.cf_flux, occupation=occ2)


class JainCallable(TrialCallable):
    """`Jain` through ``slogdet`` (see `TrialCallable`)."""

    def __init__(self, nspins, flux, cf_flux: int = 1, occupation=None, system=None):
        self.nspins = tuple(int(n) for n in nspins)
        self.flux = int(flux)
        self.cf_flux = int(cf_flux)
        self.system = system
        self.Q1 = laughlin_q1(self.nspins, self.flux, self.cf_flux)
        if occupation is None:
            occupation = default_occupation(self.nspins, self.flux, self.cf_flux)
        occ2 = check_occupation(self.nspins, self.flux, self.cf_flux, occupation)
        self.occupation = tuple((n, m2 / 2) for n, m2 in occ2)
        q2 = int(round(2 * self.Q1))
        self._cols = tuple((n, (q2 + m2) // 2, (q2 - m2) // 2) for n, m2 in occ2)  # (n, A, B)

    def _logpsi(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(torch.float64)
        N, p = x.shape[0], self.cf_flux
        theta, phi = x[:, 0], x[:, 1]
        u = torch.cos(theta / 2) * torch.exp(0.5j * phi)
        v = torch.sin(theta / 2) * torch.exp(-0.5j * phi)
        eye = torch.eye(N, dtype=u.dtype, device=x.device)
        w = u[:, None] * v[None, :] - u[None, :] * v[:, None] + eye  # w_ik, diagonal 1
        off = 1.0 - eye
        Du = p * torch.sum(off * v[None, :] / w, dim=-1)
        Dv = -p * torch.sum(off * u[None, :] / w, dim=-1)
        cols = []
        for n, A, B in self._cols:
            if n == 0:
                cols.append(u**A * v**B)
                continue
            # an exponent -1 only comes with the weight 0: that term is absent
            c = torch.zeros_like(u)
            if A + 1 != 0:
                c = c + (A + 1) * u**A * v ** (B + 1) * Dv
            if B + 1 != 0:
                c = c - (B + 1) * u ** (A + 1) * v**B * Du
            cols.append(c)
        sign, logdet = torch.linalg.slogdet(torch.stack(cols, dim=-1))
        pair = torch.sum(torch.triu(torch.log(w), diagonal=1))  # sum_{i<k} log w_ik
        return logdet + torch.log(sign) + 2 * p * pair


__all__ = ["Jain", "JainCallable", "default_occupation", "check_occupation"]
