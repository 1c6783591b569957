"""Renyi-2 entanglement entropy of the polar caps theta < theta_a by the swap estimator.

Not in the reference.  Two independent replicas (R1, R2) ~ |psi|^2 |psi|^2 and the swap of the
electrons inside region A give Tr rho_A^2 = < psi(R1') psi(R2') / (psi(R1) psi(R2)) >.  The
walkers of one step are paired (walker p, walker p + P), P = B // 2 (an odd last walker is
ignored).  A pair contributes only when the up count and the down count inside A agree between
its members (otherwise the swapped configurations do not exist in the fixed-number sectors and
the value is 0); its sector is k = nA_up (n_dn + 1) + nA_dn.  R1' is R1 with the coordinates of
its in-A slots, in ascending slot order within each spin, replaced by R2's, R2' the mirror image:
any spin-preserving bijection gives the same product, its sign cancels between the two factors.

Classification, the deterministic compaction of the matched pairs and the reduction are HIP
kernels (csrc/swap.hip, ``dh_swap_*``); the swapped rows of all angles go through ONE batched
``dh_logpsi`` call, so only matched pairs cost a forward pass.

Options: ``thetas`` — a list of cap angles, or an int n for linspace(0, pi, n + 2)[1:-1]
(default 16).  Step value ``purity`` [1, A, K] complex128 (the sums over pairs / P; the driver
averages axis 0); state ``counts`` [A, K] (sector counts of all pair members, summed over
steps) and ``pairs``.  ``entanglement.filled_lll_cap`` gives the exact free-fermion values.
"""

from __future__ import annotations

import math

import torch

from .._native import swap_purity
from ..estimator import Estimator, Observable


def cap_angles(thetas) -> list[float]:
    """The ``thetas`` option: a list as given, an int n as the n interior points of linspace(0, pi, n + 2)."""
    if isinstance(thetas, int):
        if thetas < 1:
            raise ValueError(f"renyi2: thetas must be a list or a positive int, got {thetas}")
        return [math.pi * (j + 1) / (thetas + 1) for j in range(thetas)]
    out = [float(t) for t in thetas]
    if not out or any(math.isnan(t) for t in out):
        raise ValueError("renyi2: thetas must be a non-empty list of angles without NaN")
    return out


class Renyi2(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return (len(cap_angles(self.options.get("thetas", 16))),)


class Renyi2Estimator(Estimator):
    observable_type = Renyi2

    def __init__(self, adaptor, system, estimator_options, observable_options):
        thetas = cap_angles((estimator_options or {}).get("thetas", 16))
        super().__init__(adaptor, system, estimator_options, {**(observable_options or {}), "thetas": thetas})
        self.thetas = thetas
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))
        self.sectors = (self.nspins[0] + 1) * (self.nspins[1] + 1)

    def empty_val_state(self, steps: int):
        A, K = len(self.thetas), self.sectors
        return ({"purity": torch.zeros((steps, A, K), dtype=torch.complex128)},
                {"counts": torch.zeros((A, K), dtype=torch.int64), "pairs": 0})

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        P = x.shape[0] // 2
        sums, counts = swap_purity(lambda rows: self.adaptor.call_network(params, rows), x, self.thetas, self.nspins)
        state["counts"] = state["counts"] + counts.cpu()
        state["pairs"] = state["pairs"] + P
        return {"purity": (sums / P).cpu()[None]}, state

    def digest(self, all_values, state):
        steps = all_values["purity"]                       # [steps, A, K]
        sector_purity = steps.mean(dim=0)                  # [A, K]
        purity = sector_purity.sum(dim=-1)                 # [A]
        per_step = steps.sum(dim=-1).real                  # [steps, A]
        n = per_step.shape[0]
        err = per_step.std(dim=0, unbiased=True) / math.sqrt(n) if n > 1 else torch.full_like(purity.real, math.nan)
        number = state["counts"].double() / max(2 * int(state["pairs"]), 1)
        ratio = sector_purity.real / number**2             # 0 / 0 = NaN where the sector is empty
        return {
            "purity": purity.real,
            "renyi2": -torch.log(purity.real),
            "renyi2_err": err / purity.real,
            "purity_imag": purity.imag,
            "sector_purity": sector_purity.real,
            "number_distribution": number,
            "sector_renyi2": torch.where(number > 0, -torch.log(ratio), torch.full_like(ratio, math.nan)),
        }


DEFAULT = Renyi2Estimator  # Useful in CLI
