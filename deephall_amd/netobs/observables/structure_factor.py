"""Static structure factor in angular-momentum space,

    S(L) = (4 pi / (N (2L+1))) sum_M < |rho_LM|^2 >,      rho_LM = sum_i Y_LM(Omega_i).

Not in the reference.  Slots 0..n_up-1 are up electrons and the rest are down, N = n_up + n_dn,
gamma_ij is the angle between electrons i and j:

    cos gamma = cos th_i cos th_j + sin th_i sin th_j cos(ph_i - ph_j)

Per-walker pair sums (no harmonics needed, by the addition theorem):
T_uu(L) = sum_{i<j, both up} P_L(cos gamma_ij), T_dd(L) likewise for both down,
T_ud(L) = sum_{i up, j down} P_L(cos gamma_ij).  Per-walker multipoles:
rho^a_LM = sum_{i in species a} Y_LM(th_i, ph_i) for a = up, down and 0 <= M <= L <= lmax, orthonormal
Y_LM with the Condon-Shortley phase (Y_{L,-M} = (-1)^M conj(Y_LM)), at index lm = L(L+1)/2 + M,
nlm = (lmax+1)(lmax+2)/2.  With means over the valid walkers (all 2N coordinates finite):

    S(L)      = 1 + (2/N) <T_uu + T_ud + T_dd>
    S_uu(L)   = n_up/N + (2/N) <T_uu>,  S_dd likewise,  S_ud(L) = (1/N) <T_ud>
                (S = S_uu + S_dd + 2 S_ud)
    S_spin(L) = S_uu + S_dd - 2 S_ud
    S_c(L)    = S(L) - (4 pi / (N (2L+1))) (|<rho_L0>|^2 + 2 sum_{M>0} |<rho_LM>|^2),  rho = rho^up + rho^dn

and the guiding-centre structure factor S̄(L) = S(L) - 1 + F_L with
F_L = (2Q+1)! (2Q)! / ((2Q-L)! (2Q+L+1)!) for L <= 2Q = flux and 0 above.  S̄ is meaningful for
lowest-Landau-level states only: it vanishes identically for the filled level, and a lowest-level
state of total angular momentum L_tot has S̄(1) = L_tot (L_tot + 1) / (N (Q + 1)^2).

Everything comes from the walkers alone — no wavefunction evaluation beyond the MCMC walk — so the
estimator runs on every network type.  The sums over walkers are ``dh_sf_accumulate``
(csrc/sfactor.hip: double arithmetic, a fixed order, no float atomics), read back once per step.

Options: ``lmax`` (default min(2 flux + 2, 64); an int in 0..64) and ``multipoles`` (default true;
false skips the multipoles and ``connected``).  Step values ``pairs`` [1, 3, lmax+1] float64 (the
walker means of T_uu, T_ud, T_dd) and, with multipoles, ``rho`` [1, 2, nlm] complex128; state
``walkers`` (the valid walkers, summed over steps).  ``form_factor`` and ``digest_steps`` are plain
torch and run on CPU tensors.
"""

from __future__ import annotations

import math
from fractions import Fraction

import torch

from ... import _lib
from .._native import sf_accumulate_host
from ..estimator import Estimator, Observable


def sf_options(options, flux: int) -> tuple[int, bool]:
    """(lmax, multipoles) of the estimator options, validated."""
    options = options or {}
    lmax = options.get("lmax")
    if lmax is None:
        lmax = min(2 * int(flux) + 2, _lib.DH_SF_MAX_L)
    if not isinstance(lmax, int) or isinstance(lmax, bool) or not 0 <= lmax <= _lib.DH_SF_MAX_L:
        raise ValueError(f"structure_factor: lmax must be an int in 0..{_lib.DH_SF_MAX_L}, got {lmax!r}")
    return lmax, bool(options.get("multipoles", True))


def form_factor(flux: int, lmax: int) -> torch.Tensor:
    """1 - F_L for L = 0..lmax (float64), F_L = (2Q+1)! (2Q)! / ((2Q-L)! (2Q+L+1)!) for L <= 2Q = flux
    and 0 above, in exact integers: S(L >= 1) of the filled lowest level.  F_0 = 1."""
    f = math.factorial
    n = int(flux)
    F = [float(Fraction(f(n + 1) * f(n), f(n - L) * f(n + L + 1))) if L <= n else 0.0 for L in range(int(lmax) + 1)]
    return 1.0 - torch.tensor(F, dtype=torch.float64)


def digest_steps(pairs: torch.Tensor, rho: torch.Tensor | None, nspins, flux: int) -> dict[str, torch.Tensor]:
    """The digest from the step arrays pairs [steps, 3, lmax+1] and rho [steps, 2, nlm] (or None)."""
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    N = n_up + n_dn
    pairs = torch.as_tensor(pairs, dtype=torch.float64)
    steps, _, nl = pairs.shape
    s_steps = 1.0 + (2.0 / N) * pairs.sum(dim=1)          # [steps, lmax+1]
    err = (s_steps.std(dim=0, unbiased=True) / math.sqrt(steps) if steps > 1
           else torch.full((nl,), math.nan, dtype=torch.float64))
    T = pairs.mean(dim=0)
    s_uu, s_dd, s_ud = n_up / N + (2.0 / N) * T[0], n_dn / N + (2.0 / N) * T[2], T[1] / N
    s = s_uu + s_dd + 2.0 * s_ud
    ff = form_factor(flux, nl - 1)
    out = {
        "structure_factor": s,
        "structure_factor_err": err,
        "partial": torch.stack([s_uu, s_ud, s_dd]),
        "spin_structure_factor": s_uu + s_dd - 2.0 * s_ud,
        "guiding_center": s - ff,
        "form_factor": ff,
    }
    if rho is not None:
        mean = torch.as_tensor(rho, dtype=torch.complex128).mean(dim=0)   # [2, nlm]
        w = (mean[0] + mean[1]).abs() ** 2
        L = torch.arange(nl)
        row = torch.zeros(nl, dtype=torch.float64).index_add_(0, torch.repeat_interleave(L, L + 1), w)  # 0 <= M <= L
        out["connected"] = s - (4.0 * math.pi / N) * (2.0 * row - w[L * (L + 1) // 2]) / (2 * L + 1)
        out["multipole_mean"] = mean
    return out


class StructureFactor(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return (sf_options(self.options, system["flux"])[0] + 1,)


class StructureFactorEstimator(Estimator):
    observable_type = StructureFactor

    def __init__(self, adaptor, system, estimator_options, observable_options):
        self.lmax, self.multipoles = sf_options(estimator_options, system["flux"])
        super().__init__(adaptor, system, estimator_options, {"lmax": self.lmax, **(observable_options or {})})
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))
        self.flux = int(system["flux"])
        self.nlm = (self.lmax + 1) * (self.lmax + 2) // 2

    def empty_val_state(self, steps: int):
        values = {"pairs": torch.zeros((steps, 3, self.lmax + 1), dtype=torch.float64)}
        if self.multipoles:
            values["rho"] = torch.zeros((steps, 2, self.nlm), dtype=torch.complex128)
        return values, {"walkers": 0}

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, params, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        pairs, rho, nvalid = sf_accumulate_host(x, self.nspins[0], self.lmax, self.multipoles)
        state["walkers"] = state["walkers"] + nvalid
        # nvalid = 0: NaN, which the driver's mean drops
        values = {"pairs": (pairs / nvalid)[None]}
        if self.multipoles:
            values["rho"] = (rho / nvalid)[None]
        return values, state

    def digest(self, all_values, state):
        del state
        return digest_steps(all_values["pairs"], all_values.get("rho") if self.multipoles else None, self.nspins,
                            self.flux)


DEFAULT = StructureFactorEstimator  # Useful in CLI
