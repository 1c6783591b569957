"""Electron density around a chosen point of the sphere, and the excess charge it encloses.

Not in the reference.  ``density`` histograms the polar angle only, so it resolves a localised
object on the z axis alone; this estimator measures the angle gamma from any axis a = (theta, phi):
u_i = r_i . a = cos gamma_i for every electron, binned in ``bins`` bins of equal area,

    bin k:  1 - 2 (k + 1) / bins < u <= 1 - 2 k / bins,     k = 0 at the axis, bins - 1 opposite it.

The counts come from ``dh_axis_histogram`` (csrc/impurity.hip: double arithmetic, integer counts in
LDS, integer atomics, so the order of the sum does not matter), up and down electrons apart.  They
need the walkers only, so the estimator runs on every network type.

Options: ``axis: [theta, phi]``, or ``impurity: k`` to take the axis of ``system.impurities[k]`` from
the restored config; ``bins`` (default 50; 1..4096).  State: ``counts`` int64 [2, bins] summed over
the steps and ``walkers``, the walkers seen.  With W walkers of N electrons the digest gives

    theta        the angle of each bin's centre in u, arccos(1 - (2 k + 1) / bins)
    theta_edge   the angle of each bin's far edge, arccos(1 - 2 (k + 1) / bins); the last is pi
    density      [3, bins]: up, down and both, in units of the uniform density N / (4 pi R^2);
                 the bins have equal area, so this is counts bins / (W N)
    density_err  its binomial standard error, sqrt(c (1 - c / (W N))) bins / (W N) for a count c
    excess       Q(theta_edge[k]) = sum_{k' <= k} (<n_k'> - N / bins), <n_k> = counts_k / W of both
                 species: the electrons inside the cap minus the uniform state's; Q(pi) = 0
    excess_err   sqrt(C (1 - C / (W N))) / W for the cumulative count C: binomial, the W N electron
                 positions taken as independent draws (correlations between a walker's electrons
                 and between steps are not in it)

``digest_counts`` is plain torch and runs on CPU tensors.
"""

from __future__ import annotations

import math

import torch

from ... import _lib
from .._native import axis_histogram
from ..estimator import Estimator, Observable


def axis_options(options, impurities=()) -> tuple[tuple[float, float], int]:
    """((theta, phi), bins) of the estimator options, validated."""
    options = options or {}
    bins = options.get("bins", 50)
    if not isinstance(bins, int) or isinstance(bins, bool) or not 1 <= bins <= _lib.DH_AXIS_MAX_BINS:
        raise ValueError(f"axis_density: bins must be an int in 1..{_lib.DH_AXIS_MAX_BINS}, got {bins!r}")
    has_axis, has_imp = options.get("axis") is not None, options.get("impurity") is not None
    if has_axis == has_imp:
        raise ValueError("axis_density: give one of the options axis: [theta, phi] and impurity: k")
    if has_imp:
        k = options["impurity"]
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < len(impurities):
            raise ValueError(f"axis_density: impurity {k!r} is not an index into the system's {len(impurities)} "
                             "impurities")
        axis = (impurities[k].theta, impurities[k].phi)
    else:
        axis = tuple(float(v) for v in options["axis"])
    if len(axis) != 2 or not all(math.isfinite(v) for v in axis) or not 0.0 <= axis[0] <= math.pi:
        raise ValueError(f"axis_density: axis must be finite [theta, phi] with 0 <= theta <= pi, got {axis!r}")
    return axis, bins


def digest_counts(counts: torch.Tensor, walkers: int, nspins) -> dict[str, torch.Tensor]:
    """The digest from the accumulated counts [2, bins] of ``walkers`` walkers."""
    counts = torch.as_tensor(counts).to(device="cpu", dtype=torch.float64)
    bins, N, W = counts.shape[1], int(nspins[0]) + int(nspins[1]), float(walkers)
    k = torch.arange(bins, dtype=torch.float64)
    c3 = torch.cat([counts, counts.sum(dim=0, keepdim=True)])  # up, down, both
    cum = c3[2].cumsum(dim=0)
    draws = W * N
    return {
        "theta": torch.acos(1.0 - (2.0 * k + 1.0) / bins),
        "theta_edge": torch.acos((1.0 - 2.0 * (k + 1.0) / bins).clamp(min=-1.0)),
        "density": c3 * bins / draws,
        "density_err": (c3 * (1.0 - c3 / draws)).clamp(min=0.0).sqrt() * bins / draws,
        "excess": (cum - (k + 1.0) * draws / bins) / W,  # one rounding: Q(pi) is 0 exactly when no electron is dropped
        "excess_err": (cum * (1.0 - cum / draws)).clamp(min=0.0).sqrt() / W,
    }


class AxisDensity(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return (int(self.options.get("bins", 50)),)


class AxisDensityEstimator(Estimator):
    observable_type = AxisDensity

    def __init__(self, adaptor, system, estimator_options, observable_options):
        cfg = getattr(adaptor, "cfg", None)
        impurities = tuple(cfg.system.impurities) if cfg is not None else ()
        self.axis, self.bins = axis_options(estimator_options, impurities)
        super().__init__(adaptor, system, estimator_options, {"bins": self.bins, **(observable_options or {})})
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))

    def empty_val_state(self, steps: int):
        del steps
        return {}, {"counts": None, "walkers": 0}

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, params, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        counts = axis_histogram(x, self.nspins, self.axis, self.bins)
        state["counts"] = counts if state["counts"] is None else state["counts"] + counts
        state["walkers"] = state["walkers"] + x.shape[0]
        return {}, state

    def digest(self, all_values, state):
        del all_values
        if state["counts"] is None:
            return {}
        return digest_counts(state["counts"], state["walkers"], self.nspins)


DEFAULT = AxisDensityEstimator  # Useful in CLI
