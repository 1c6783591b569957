"""Pair amplitudes: the mean number A_L of electron pairs with total pair angular momentum L in the
lowest Landau level, that is relative angular momentum m = 2Q - L.  Not in the reference.

    A_L = < sum_{i<j} (4 pi)^2 K_L(r_i, r_j; r1', r2') psi(R_{ij -> r1' r2'}) / psi(R) >

with r1', r2' independent and uniform on the sphere, R_{ij -> r1' r2'} the walker with electron i at
r1' and electron j at r2', and K_L the projector of a pair onto angular momentum L built from the
orbitals Y_{Q,Q,m} (closed form and recurrence: csrc/pairamp.hip).  The sum is split into up-up,
up-down and down-down pairs.  For a lowest-level state sum_L A_L = N (N - 1) / 2, same-species
pairs have no even m, and any pair interaction has the energy sum_L V_L A_L with its Haldane
pseudopotentials V_L (netobs/pseudopotential.py), so one run prices every interaction afterwards;
for a Psiformer sum_L A_L / (N (N - 1) / 2) is the weight of its pairs inside the lowest level, the
two-body counterpart of ``ll_rdm``'s ``lll_weight``.  The displaced rows (``dh_pair_displace``) and
the reduction over walkers, points and pairs (``dh_pair_accumulate``: double, a fixed order, samples
with a non-finite log-amplitude or ratio dropped whole) are HIP kernels; only A [3, 2Q + 1] leaves
the device.  A step costs points x B N (N - 1) / 2 forward rows.

Options: ``points`` (default 1) draws of (r1', r2') per walker per step; ``max_rows`` (default
None: all pairs at once) bounds the rows of one wavefunction call; ``legendre`` [v_0, v_1, ...]
adds the energy of v(cos gamma) = sum_k v_k P_k(cos gamma); ``radius`` and ``interaction_strength``
default to the adaptor's system (``adaptor.cfg.system``), else sqrt(Q) and 1.  The points of a step
are ONE ``init_guess`` draw of 2 x points x B single-electron walkers with the step's key: draw
p B + b is r1' of point p of walker b, draw (points + p) B + b its r2' (``init_guess`` reads the
key's seed, not its counter, so a second call would repeat the first: see ll_rdm.py).
Step value ``pair_amplitude`` [1, 3, 2Q + 1] complex128 (the sample mean; the driver averages axis
0; NaN for a step that kept no sample, which the digest leaves out of its means and errors); state
``samples`` (the (walker, point) samples kept, summed over steps).
"""

from __future__ import annotations

import math

import torch

from ...train import init_guess
from .. import pseudopotential
from .._native import pair_amplitude_sums
from ..estimator import Estimator, Observable


def pair_options(options):
    """(points, max_rows, legendre) of the estimator options, validated."""
    options = options or {}
    points, max_rows, legendre = options.get("points", 1), options.get("max_rows"), options.get("legendre")
    if not isinstance(points, int) or isinstance(points, bool) or points < 1:
        raise ValueError(f"pair_amplitude: points must be a positive int, got {points!r}")
    if max_rows is not None and (not isinstance(max_rows, int) or isinstance(max_rows, bool) or max_rows < 1):
        raise ValueError(f"pair_amplitude: max_rows must be a positive int or None, got {max_rows!r}")
    if legendre is not None:
        legendre = [float(v) for v in legendre]
        if not legendre or not all(math.isfinite(v) for v in legendre):
            raise ValueError(f"pair_amplitude: legendre must be a non-empty list of finite numbers, got {legendre!r}")
    return points, max_rows, legendre


class PairAmplitude(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return (3, system["flux"] + 1)


class PairAmplitudeEstimator(Estimator):
    observable_type = PairAmplitude

    def __init__(self, adaptor, system, estimator_options, observable_options):
        self.points, self.max_rows, self.legendre = pair_options(estimator_options)
        super().__init__(adaptor, system, estimator_options, observable_options)
        self.flux = int(system["flux"])
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))
        if not 1 <= self.flux <= 126:
            raise ValueError(f"pair_amplitude: flux must be in 1..126, got {self.flux}")
        sys_cfg = getattr(getattr(adaptor, "cfg", None), "system", None)
        radius = self.options.get("radius", getattr(sys_cfg, "radius", None)) or math.sqrt(self.flux / 2)
        strength = self.options.get("interaction_strength", getattr(sys_cfg, "interaction_strength", 1.0))
        self.radius, self.strength = float(radius), float(strength)
        as_t = lambda v: torch.as_tensor(v, dtype=torch.float64) * self.strength  # noqa: E731
        self.potentials = {"coulomb": as_t(pseudopotential.coulomb_pseudopotentials(self.flux, self.radius)),
                           "harmonic": as_t(pseudopotential.harmonic_pseudopotentials(self.flux))}
        if self.legendre is not None:
            self.potentials["legendre"] = as_t(pseudopotential.pseudopotentials(self.flux, self.legendre))

    def empty_val_state(self, steps: int):
        return {"pair_amplitude": torch.zeros((steps, *self.observable.shape), dtype=torch.complex128)}, {"samples": 0}

    def accumulate(self, params, x: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor):
        """(the sum over the kept samples of the pair terms [3, 2Q + 1] complex128 on the device, the
        number kept) for walkers x [B, N, 2] and points r1, r2 [P, B, 2]."""
        return pair_amplitude_sums(lambda rows: self.adaptor.call_network(params, rows), x, r1, r2, self.nspins[0],
                                   self.flux, self.max_rows)

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, aux_data, system
        x = data.reshape(-1, *data.shape[-2:])
        B = x.shape[0]
        draws = init_guess(key, 2 * self.points * B, 1, x.device, network=self.adaptor.model)[:, 0, :]
        draws = draws.reshape(2, self.points, B, 2)
        A, nvalid = self.accumulate(params, x, draws[0], draws[1])
        state["samples"] = state["samples"] + nvalid
        return {"pair_amplitude": (A / nvalid).cpu()[None]}, state  # nvalid = 0: a NaN step, which the digest leaves out

    def digest(self, all_values, state):
        del state
        steps = all_values["pair_amplitude"]                          # [steps, 3, 2Q + 1]
        steps = steps[~torch.isnan(torch.view_as_real(steps)).flatten(1).any(dim=1)]  # without the NaN steps
        n = steps.shape[0]
        mean = steps.mean(dim=0)
        amp = mean.real

        def stderr(v):                                                # over axis 0
            return v.std(dim=0, unbiased=True) / math.sqrt(n) if n > 1 else torch.full(v.shape[1:], math.nan, dtype=v.dtype)

        total_steps = steps.real.sum(dim=1)                           # [steps, 2Q + 1]
        nelec = sum(self.nspins)
        npairs = nelec * (nelec - 1) / 2
        m = self.flux - torch.arange(self.flux + 1)                   # relative angular momentum of each L
        same = amp[[0, 2]][:, m % 2 == 0]
        out = {
            "amplitudes": amp,
            "amplitudes_err": stderr(steps.real),
            "by_relative": amp.flip(-1),
            "total": amp.sum(dim=0),
            "pairs_in_lll": amp.sum() / npairs if npairs else torch.tensor(math.nan, dtype=torch.float64),
            "forbidden": same.abs().max(),
            "imag": mean.imag.abs().max(),
        }
        for name, V in self.potentials.items():
            e_steps = total_steps @ V                                 # [steps]
            out[f"{name}_energy"] = e_steps.mean()
            out[f"{name}_energy_err"] = stderr(e_steps)
        return out


DEFAULT = PairAmplitudeEstimator  # Useful in CLI
