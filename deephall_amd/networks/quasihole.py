"""Quasiholes pinned at chosen points of the sphere on MI355X (not in the reference).

With u = cos(theta/2) e^(i phi/2), v = sin(theta/2) e^(-i phi/2) and w_ik = u_i v_k - u_k v_i, a
hole a at (theta_a, phi_a) has the spinor (U_a, V_a) of an electron there and

    s_a(i) = u_i V_a - v_i U_a,

zero when electron i sits on the hole.

Base ``"halperin"`` (Laughlin 1/m is nspins (N, 0) with exponents (m, ., 0)):

    log psi = sum_{i<k} c_ik log w_ik + sum_a sum_{i in S_a} log s_a(i)

c_ik as for `Halperin`; S_a all electrons (``"both"``), the up slots (``"up"``) or the down slots
(``"down"``).  With h_up and h_dn holes acting on a species, a non-empty species needs
flux = m_up (n_up - 1) + n n_dn + h_up = m_dn (n_dn - 1) + n n_up + h_dn.

Base ``"pfaffian"``: ``pairing = (A, B)`` splits 2k holes into two groups of k, the holes not
listed are Abelian (they act on every electron),

    F_i = prod_{a in A} s_a(i),   G_i = prod_{b in B} s_b(i),
    A_ik = (F_i G_k + F_k G_i) / w_ik (i != k),   A_ii = 0,
    log psi = log Pf(A) + 2p sum_{i<k} log w_ik + sum_{a Abelian} sum_i log s_a(i)

at flux 2p (N - 1) - 1 + k + (number of Abelian holes) exactly (k = 0: A_ik = 1 / w_ik, Moore-Read's
own entries).  Four holes have the three
pairings (01)(23), (02)(13), (03)(12): three states of one two-dimensional space.

No normalisation; Im log psi is the principal phase.  At most 8 holes.  ``Quasihole`` runs on the
kernels of quasihole.hip through the Psiformer's native plumbing, as the other analytic states do
(no parameters).  ``QuasiholeCallable`` is the same state as a float64 torch log-psi callable
(batched, and differentiable under torch.func): the independent route the tests compare the kernel
with; it runs on CPU tensors.
"""

from __future__ import annotations

import math

import torch

from .laughlin import Laughlin, TrialCallable
from .pfaffian import log_pfaffian

MAX_HOLES = 8
BASES = ("halperin", "pfaffian")


def check_quasihole(nspins, flux, base="halperin", holes=(), species=None, pairing=None, exponents=(3, 3, 2),
                    cf_flux: int = 1) -> tuple:
    """(base, (m_up, m_dn, n), p, ((theta, phi, kind), ...)) after the checks dh_create_quasihole
    repeats; kind is "both", "up", "down", "A" or "B"."""
    base = str(getattr(base, "value", base))
    if base not in BASES:
        raise ValueError(f"Quasihole: base must be 'halperin' or 'pfaffian', got {base!r}")
    try:
        n_up, n_dn = (int(n) for n in nspins)
        holes = tuple((float(t), float(p)) for t, p in holes)
    except (TypeError, ValueError) as e:
        raise ValueError(f"Quasihole: need nspins (n_up, n_dn) and holes ((theta, phi), ...), got {nspins!r}, {holes!r}") from e
    N, flux, nh = n_up + n_dn, int(flux), len(holes)
    if n_up < 0 or n_dn < 0 or not 1 <= N <= 32:
        raise ValueError(f"Quasihole: need 1 <= N <= 32 electrons, got nspins = {tuple(nspins)}")
    if not 1 <= flux <= 126:
        raise ValueError(f"Quasihole needs 1 <= flux <= 126, got {flux}")
    if not 1 <= nh <= MAX_HOLES:
        raise ValueError(f"Quasihole: need 1 <= number of holes <= {MAX_HOLES}, got {nh}"
                         + (f" (without holes this is the {base} state)" if nh == 0 else ""))
    for a, (t, p) in enumerate(holes):
        if not (math.isfinite(t) and math.isfinite(p)):
            raise ValueError(f"Quasihole: hole {a} has a non-finite angle")
        if not 0.0 <= t <= math.pi:
            raise ValueError(f"Quasihole: hole {a} needs 0 <= theta <= pi, got {t}")
    if base == "halperin":
        if pairing is not None:
            raise ValueError("Quasihole: pairing belongs to the pfaffian base")
        kinds = tuple(str(s) for s in species) if species is not None else ("both",) * nh
        if len(kinds) != nh or any(k not in ("both", "up", "down") for k in kinds):
            raise ValueError(f"Quasihole: species needs one of 'both', 'up', 'down' per hole, got {species!r}")
        try:
            m_up, m_dn, n = (int(e) for e in exponents)
        except (TypeError, ValueError) as e:
            raise ValueError(f"Quasihole: need exponents (m_up, m_dn, n), got {exponents!r}") from e
        if m_up < 1 or m_dn < 1 or m_up % 2 == 0 or m_dn % 2 == 0:
            raise ValueError(f"Quasihole: m_up and m_dn must be odd and >= 1, got {m_up}, {m_dn}")
        if n < 0:
            raise ValueError(f"Quasihole: need n >= 0, got {n}")
        h_up = sum(k in ("both", "up") for k in kinds)
        h_dn = sum(k in ("both", "down") for k in kinds)
        f_up, f_dn = m_up * (n_up - 1) + n * n_dn + h_up, m_dn * (n_dn - 1) + n * n_up + h_dn
        if n_up > 0 and flux != f_up:
            raise ValueError(f"Quasihole: the up electrons live at flux m_up (n_up - 1) + n n_dn + h_up = {f_up}, got {flux}")
        if n_dn > 0 and flux != f_dn:
            raise ValueError(f"Quasihole: the down electrons live at flux m_dn (n_dn - 1) + n n_up + h_dn = {f_dn}, got {flux}")
        return base, (m_up, m_dn, n), 1, tuple((t, p, k) for (t, p), k in zip(holes, kinds))
    if species is not None and any(str(s) != "both" for s in species):
        raise ValueError("Quasihole: species 'up' and 'down' belong to the halperin base")
    p = int(cf_flux)
    if N % 2:
        raise ValueError(f"Quasihole: the pfaffian base needs an even number of electrons, got N = {N}")
    if p < 1:
        raise ValueError(f"Quasihole: the pfaffian base needs cf_flux >= 1, got {cf_flux}")
    try:
        ga, gb = (tuple(int(a) for a in grp) for grp in (pairing if pairing is not None else ((), ())))
    except (TypeError, ValueError) as e:
        raise ValueError(f"Quasihole: pairing needs two tuples of hole indices, got {pairing!r}") from e
    if len(ga) != len(gb):
        raise ValueError(f"Quasihole: the groups A and B need the same number of holes, got {len(ga)} and {len(gb)}")
    listed = ga + gb
    if len(set(listed)) != len(listed) or any(not 0 <= a < nh for a in listed):
        raise ValueError(f"Quasihole: pairing must list each hole index at most once, within 0..{nh - 1}, got {pairing!r}")
    kinds = tuple("A" if a in ga else "B" if a in gb else "both" for a in range(nh))
    want = 2 * p * (N - 1) - 1 + len(ga) + (nh - len(listed))
    if flux != want:
        raise ValueError(f"Quasihole: the state lives at flux 2p (N - 1) - 1 + k + (Abelian holes) = {want}, got {flux}")
    # the energy kernel's LDS (quasihole.hip qsm_layout): 16 (11 N^2 + 29 N + 20) bytes in 160 KiB
    if 16 * (11 * N * N + 29 * N + 20) > 160 * 1024:
        raise ValueError(f"Quasihole: N = {N} does not fit the pfaffian base's one-workgroup kernel (N <= 28)")
    return base, (2 * p, 2 * p, 2 * p), p, tuple((t, ph, k) for (t, ph), k in zip(holes, kinds))


class Quasihole(Laughlin):
    """Parameter-free analytic wavefunction on quasihole.hip."""

    name = "quasihole"
    network_type = "quasihole"

    def __init__(self, nspins, flux, base="halperin", holes=(), species=None, pairing=None, exponents=(3, 3, 2),
                 cf_flux: int = 1, system=None):
        self._sphere(nspins, flux)
        self.state = check_quasihole(self.nspins, self.flux, base, holes, species, pairing, exponents, cf_flux)
        self.base, self.exponents, self.cf_flux, self.holes = self.state
        self.spec = self._spec(system, quasihole=self.state)


class QuasiholeCallable(TrialCallable):
    """`Quasihole` in torch operations (see `TrialCallable`)."""

    def __init__(self, nspins, flux, base="halperin", holes=(), species=None, pairing=None, exponents=(3, 3, 2),
                 cf_flux: int = 1, system=None):
        self.nspins = tuple(int(n) for n in nspins)
        self.flux = int(flux)
        self.state = check_quasihole(self.nspins, self.flux, base, holes, species, pairing, exponents, cf_flux)
        self.base, self.exponents, self.cf_flux, self.holes = self.state
        self.system = system
        N, n_up = sum(self.nspins), self.nspins[0]
        th = torch.tensor([h[0] for h in self.holes], dtype=torch.float64)
        ph = torch.tensor([h[1] for h in self.holes], dtype=torch.float64)
        self._U = torch.cos(th / 2) * torch.exp(0.5j * ph)
        self._V = torch.sin(th / 2) * torch.exp(-0.5j * ph)
        up = torch.arange(N) < n_up
        m_up, m_dn, n = self.exponents
        c = torch.where(up[:, None] & up[None, :], m_up, torch.where(~up[:, None] & ~up[None, :], m_dn, n))
        self._c = torch.triu(c, diagonal=1).to(torch.float64)  # c_ik for i < k, 0 elsewhere
        kinds = [h[2] for h in self.holes]
        # acts[i, a]: hole a enters the one-body part of electron i
        self._acts = torch.stack([torch.ones(N, dtype=torch.bool) if k == "both" else up if k == "up" else ~up
                                  if k == "down" else torch.zeros(N, dtype=torch.bool) for k in kinds], dim=1)
        self._groups = tuple([a for a, k in enumerate(kinds) if k == g] for g in ("A", "B"))

    def _logpsi(self, x: torch.Tensor) -> torch.Tensor:
        x = x.to(torch.float64)
        theta, phi = x[:, 0], x[:, 1]
        u = torch.cos(theta / 2) * torch.exp(0.5j * phi)
        v = torch.sin(theta / 2) * torch.exp(-0.5j * phi)
        U, V, c, acts = self._U.to(x.device), self._V.to(x.device), self._c.to(x.device), self._acts.to(x.device)
        w = u[:, None] * v[None, :] - u[None, :] * v[:, None]
        s = u[:, None] * V[None, :] - v[:, None] * U[None, :]  # s[i, a]
        # a pair without weight (the diagonal, k < i, an up-down pair at n = 0) and a hole that does
        # not act on an electron are taken out before the logarithm
        out = torch.sum(c * torch.log(torch.where(c != 0, w, torch.ones_like(w))))
        out = out + torch.sum(torch.log(torch.where(acts, s, torch.ones_like(s))))
        if self.base == "pfaffian":
            F = torch.ones_like(u)
            G = torch.ones_like(u) * (1.0 if self._groups[0] else 0.5)  # k = 0: the numerator is 1
            for a in self._groups[0]:
                F = F * s[:, a]
            for b in self._groups[1]:
                G = G * s[:, b]
            eye = torch.eye(x.shape[0], dtype=u.dtype, device=x.device)
            A = (1.0 - eye) * (F[:, None] * G[None, :] + F[None, :] * G[:, None]) / (w + eye)
            out = out + log_pfaffian(A)
        return out


__all__ = ["Quasihole", "QuasiholeCallable", "check_quasihole"]
