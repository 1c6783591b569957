"""Halperin (m_up, m_dn, n) two-component states on MI355X (not in the reference).

The slots below n_up = nspins[0] are up electrons, the rest down.  With
u = cos(theta/2) e^(i phi/2), v = sin(theta/2) e^(-i phi/2) and w_ik = u_i v_k - u_k v_i

    log psi = sum_{i<k} c_ik log w_ik,      c_ik = m_up (both up), m_dn (both down), n (one of each)

No determinant and no normalisation; the sum runs over i < k as for `Jain` and `MooreRead`, and
Im log psi is the principal phase.  An up electron has degree m_up (n_up - 1) + n n_dn in (u, v)
and a down electron m_dn (n_dn - 1) + n n_up: both must equal the flux, and the intra-species
exponents are odd.  (3,3,2) is the spin singlet at nu = 2/5, (1,1,0) two filled lowest Landau
levels, (1,1,1) the quantum Hall ferromagnet; (3,3,1) is no total-spin eigenstate.  Unlike the
other three analytic states this one reads ``nspins``.

``Halperin`` runs on the kernels of halperin.hip through the Psiformer's native plumbing, as
`Laughlin`, `Jain` and `MooreRead` do (no parameters; dh_logpsi, dh_mcmc_step, dh_local_energy
with the analytic Hessian in double).  ``HalperinCallable`` is the same state as a float64 torch
log-psi callable (batched and differentiable): the independent route the tests compare the
kernel with, and what `spin_square` is checked on without a GPU; it runs on CPU tensors.
"""

from __future__ import annotations

import torch

from .laughlin import Laughlin, TrialCallable


def check_halperin(nspins, flux, exponents) -> tuple:
    """(m_up, m_dn, n) in integers after the checks dh_create_halperin repeats."""
    try:
        n_up, n_dn = (int(n) for n in nspins)
        m_up, m_dn, n = (int(e) for e in exponents)
    except (TypeError, ValueError) as e:
        raise ValueError(f"Halperin: need nspins (n_up, n_dn) and exponents (m_up, m_dn, n), got {nspins!r}, {exponents!r}") from e
    N, flux = n_up + n_dn, int(flux)
    if n_up < 0 or n_dn < 0 or not 1 <= N <= 32:
        raise ValueError(f"Halperin: need 1 <= N <= 32 electrons, got nspins = {tuple(nspins)}")
    if not 1 <= flux <= 126:
        raise ValueError(f"Halperin needs 1 <= flux <= 126, got {flux}")
    if m_up < 1 or m_dn < 1 or m_up % 2 == 0 or m_dn % 2 == 0:
        raise ValueError(f"Halperin: m_up and m_dn must be odd and >= 1, got {m_up}, {m_dn}")
    if n < 0:
        raise ValueError(f"Halperin: need n >= 0, got {n}")
    if n_up > 0 and flux != m_up * (n_up - 1) + n * n_dn:
        raise ValueError(f"Halperin: the up electrons live at flux m_up (n_up - 1) + n n_dn = "
                         f"{m_up * (n_up - 1) + n * n_dn}, got {flux}")
    if n_dn > 0 and flux != m_dn * (n_dn - 1) + n * n_up:
        raise ValueError(f"Halperin: the down electrons live at flux m_dn (n_dn - 1) + n n_up = "
                         f"{m_dn * (n_dn - 1) + n * n_up}, got {flux}")
    return m_up, m_dn, n


class Halperin(Laughlin):
    """Parameter-free analytic wavefunction on halperin.hip."""

    name = "Halperin"
    network_type = "halperin"

    def __init__(self, nspins, flux, exponents=(3, 3, 2), system=None):
        self._sphere(nspins, flux)
        self.exponents = check_halperin(self.nspins, self.flux, exponents)
        self.spec = self._spec(system, halperin=self.exponents)


class HalperinCallable(TrialCallable):
    """`Halperin` in torch operations (see `TrialCallable`)."""

    def __init__(self, nspins, flux, exponents=(3, 3, 2), system=None):
        self.nspins = tuple(int(n) for n in nspins)
        self.flux = int(flux)
        self.exponents = check_halperin(self.nspins, self.flux, exponents)
        self.system = system
        N, n_up = sum(self.nspins), self.nspins[0]
        m_up, m_dn, n = self.exponents
        up = torch.arange(N) < n_up
        c = torch.where(up[:, None] & up[None, :], m_up, torch.where(~up[:, None] & ~up[None, :], m_dn, n))
        self._c = torch.triu(c, diagonal=1).to(torch.float64)  # c_ik for i < k, 0 elsewhere

    def _logpsi(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(torch.float64)
        theta, phi = x[:, 0], x[:, 1]
        u = torch.cos(theta / 2) * torch.exp(0.5j * phi)
        v = torch.sin(theta / 2) * torch.exp(-0.5j * phi)
        c = self._c.to(x.device)
        w = u[:, None] * v[None, :] - u[None, :] * v[:, None]
        # a pair without weight (the diagonal, k < i, and every up-down pair at n = 0, which may
        # coincide) is taken out before the logarithm: 0 x log 0 must not reach the sum
        w = torch.where(c != 0, w, torch.ones_like(w))
        return torch.sum(c * torch.log(w))


__all__ = ["Halperin", "HalperinCallable", "check_halperin"]
