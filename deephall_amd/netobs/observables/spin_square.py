"""Total spin <S^2> of a two-component state by exchanging one up and one down electron.

Not in the reference.  The slots below n_up are up electrons, the rest down; with R_{i<->j} the
walker R with the coordinates of an up slot i and a down slot j exchanged,

    S^2_loc(R) = ((n_up - n_dn) / 2)^2 + N / 2 - sum_{i up, j down} psi(R_{i<->j}) / psi(R)

(S^2 = S_z^2 + N / 2 + sum_{i != j} S_i^+ S_j^- on the amplitude of a fixed assignment of spins
to slots: the raising-lowering term exchanges the two coordinates, and the antisymmetry of the
full wavefunction turns its sign).  On a total-spin eigenstate
this is S (S + 1) on every walker, with zero variance, as L^2 is for an angular-momentum
eigenstate: 0 for the Halperin (3,3,2) and (1,1,0) singlets, (N/2)(N/2 + 1) for (1,1,1).

The exchanged rows (``dh_spin_exchange``: copies of the stored coordinates), the ratios in double
from the float32 logs and the reduction over walkers (``dh_spin_ratios``, ``dh_spin_reduce``: a
fixed order, no float atomics, walkers with a non-finite log or ratio dropped as
``estimator._batch_mean`` drops NaN walkers) are HIP kernels (csrc/spin.hip).  The cost is
n_up n_dn B forward rows per step through ``dh_logpsi``.

Options: ``max_rows`` — the rows in flight per wavefunction call, in whole pairs (at least one);
the default is all n_up n_dn B rows in one call.  It bounds memory only: the results are the
same bits.  Step values ``spin_square`` [1] complex128 (the mean over the valid walkers) and
``exchange`` [1, n_up, n_dn] complex128 (the mean ratio of each pair); state ``walkers`` (the
valid walkers, summed over steps).
"""

from __future__ import annotations

import math

import torch

from .._native import spin_square_sums
from ..estimator import Estimator, Observable


def spin_options(options) -> int | None:
    """``max_rows`` of the estimator options, validated."""
    max_rows = (options or {}).get("max_rows")
    if max_rows is not None and (not isinstance(max_rows, int) or isinstance(max_rows, bool) or max_rows < 1):
        raise ValueError(f"spin_square: max_rows must be a positive int or None, got {max_rows!r}")
    return max_rows


class SpinSquare(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return ()


class SpinSquareEstimator(Estimator):
    observable_type = SpinSquare

    def __init__(self, adaptor, system, estimator_options, observable_options):
        self.max_rows = spin_options(estimator_options)
        super().__init__(adaptor, system, estimator_options, observable_options)
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))

    def empty_val_state(self, steps: int):
        n_up, n_dn = self.nspins
        return ({"spin_square": torch.zeros(steps, dtype=torch.complex128),
                 "exchange": torch.zeros((steps, n_up, n_dn), dtype=torch.complex128)}, {"walkers": 0})

    def local(self, params, x: torch.Tensor):
        """(S^2_loc [B] complex128 on the device, NaN for a dropped walker; the valid walkers' sums of
        each pair's ratio [n_up, n_dn]; their sum of S^2_loc; their number) for walkers x [B, N, 2]."""
        return spin_square_sums(lambda rows: self.adaptor.call_network(params, rows), x, self.nspins, self.max_rows)

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        _, pairs, total, nvalid = self.local(params, x)
        state["walkers"] = state["walkers"] + nvalid
        # nvalid = 0: NaN, which the driver's mean drops
        return {"spin_square": (total / nvalid).cpu()[None], "exchange": (pairs / nvalid).cpu()[None]}, state

    def digest(self, all_values, state):
        del state
        steps = all_values["spin_square"]                   # [steps]
        s2 = steps.mean()
        n = steps.shape[0]
        err = steps.real.std(unbiased=True) / math.sqrt(n) if n > 1 else torch.full_like(s2.real, math.nan)
        n_up, n_dn = self.nspins
        return {
            "spin_square": s2.real,
            "spin_square_err": err,
            "spin_square_imag": s2.imag,
            "total_spin": (torch.sqrt(torch.clamp(1.0 + 4.0 * s2.real, min=0.0)) - 1.0) / 2.0,
            "exchange": all_values["exchange"].mean(dim=0),
            "sz": torch.tensor((n_up - n_dn) / 2.0, dtype=torch.float64),
        }


DEFAULT = SpinSquareEstimator  # Useful in CLI
