"""Overlap matrix of a pinned-quasihole state with its holes moved.

Not in the reference.  The network must be ``quasihole``; configuration 0 is the network's own
state psi_0, so the walkers sample |psi_0|^2.  ``estimator_options["configs"]`` lists the other
configurations, each ``{"holes": ..., "species": ... | "pairing": ...}`` with the fields it does
not name taken from ``network.quasihole``; every configuration lives at the system's flux.  With
r_c = psi_c / psi_0 on a walker,

    S[c, c'] = sum_walkers conj(r_c) r_c'  ~  <psi_c | psi_c'> / <psi_0 | psi_0>,

so the normalised O = S / sqrt(diag diag^T) is the overlap matrix of the K states: the fractional
charge and statistics of the holes are read off its phases (``holonomy.wilson_loop``), and the
pairings of the Moore-Read holes enter as configurations that differ in their kinds.

``dh_hole_logs`` gives log psi_c of all K configurations in double in one pass over the walkers
(csrc/quasihole.hip: the spinors and the pair part once per walker), ``dh_hole_gram`` the K x K sums
(csrc/holes.hip: a fixed order, no float atomics, walkers with a non-finite log dropped).  The
real shift[c] that keeps exp in range is the walker mean of Re (log psi_c - log psi_0) of the first
evaluated step and stays in the state: every step's S is in the same units, so step sums add.

Step values ``gram`` [1, K, K] complex128 (S / valid walkers) and ``walkers`` [1]; digest: the
mean ``gram``, ``overlap`` (normalised), ``berry_links`` (arg O[c, c + 1]) and the step-scatter
errors ``gram_err``, ``overlap_err``, ``berry_links_err``.
"""

from __future__ import annotations

import math

import torch

from ...networks import make_network
from ...networks.quasihole import check_quasihole
from .. import holonomy
from .._native import hole_gram, hole_logs, hole_table
from ..estimator import Estimator, Observable


def hole_states(cfg, configs) -> list:
    """The quasihole states (``check_quasihole``'s tuples) of the estimator: the network's own, then one
    per entry of ``configs``, the fields an entry does not name taken from ``cfg.network.quasihole``."""
    net, q = cfg.network, cfg.network.quasihole
    if str(getattr(net.type, "value", net.type)) != "quasihole":
        raise ValueError(f"hole_overlap: the network must be 'quasihole', got {getattr(net.type, 'value', net.type)!r}")
    if not isinstance(configs, (list, tuple)):
        raise ValueError(f"hole_overlap: configs must be a list of {{holes, species | pairing}}, got {configs!r}")
    states = []
    for c, entry in enumerate([{}] + list(configs)):
        if not isinstance(entry, dict) or set(entry) - {"holes", "species", "pairing"}:
            raise ValueError(f"hole_overlap: configuration {c} must be a dict of holes, species, pairing, got {entry!r}")
        try:
            states.append(check_quasihole(cfg.system.nspins, cfg.system.flux, q.base, entry.get("holes", q.holes),
                                          entry.get("species", q.species), entry.get("pairing", q.pairing),
                                          net.halperin.exponents, net.pfaffian.cf_flux))
        except ValueError as e:
            raise ValueError(f"hole_overlap: configuration {c}: {e}") from e
    return states


class HoleOverlap(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return ()


class HoleOverlapEstimator(Estimator):
    observable_type = HoleOverlap

    def __init__(self, adaptor, system, estimator_options, observable_options):
        super().__init__(adaptor, system, estimator_options, observable_options)
        self.states = hole_states(adaptor.cfg, self.options.get("configs", ()))
        spec = make_network(adaptor.cfg.system, adaptor.cfg.network).spec  # configuration 0 is its state
        self.table = hole_table(spec, self.states)
        self.K = len(self.states)

    def empty_val_state(self, steps: int):
        return ({"gram": torch.zeros((steps, self.K, self.K), dtype=torch.complex128),
                 "walkers": torch.zeros(steps, dtype=torch.float64)}, {"shift": None})

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, params, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        L = hole_logs(x, self.table)
        if state.get("shift") is None:
            d = (L - L[:, :1]).real
            state["shift"] = torch.nan_to_num(torch.where(torch.isfinite(d), d, torch.nan).nanmean(dim=0)).cpu()
        S, nvalid = hole_gram(L, state["shift"])
        # nvalid = 0: NaN, which the driver's mean drops
        return {"gram": (S / nvalid).cpu()[None], "walkers": torch.tensor([float(nvalid)], dtype=torch.float64)}, state

    def digest(self, all_values, state):
        del state
        steps = all_values["gram"]  # [steps, K, K]
        n = steps.shape[0]
        gram = steps.mean(dim=0)
        overlap = holonomy.overlap_matrix(gram)
        links = torch.angle(torch.diagonal(overlap, offset=1))

        def scatter(v):  # of the step values around their mean, re and im together
            if n < 2:
                return torch.full(v.shape[1:], math.nan, dtype=torch.float64)
            dev = v - v.mean(dim=0)
            return torch.sqrt((dev.abs() ** 2).sum(dim=0) / (n - 1) / n)

        step_overlap = torch.stack([holonomy.overlap_matrix(s) for s in steps])
        step_links = torch.diagonal(step_overlap * overlap.conj(), offset=1, dim1=1, dim2=2).angle()  # about the mean
        return {
            "gram": gram,
            "gram_err": scatter(steps),
            "overlap": overlap,
            "overlap_err": scatter(step_overlap),
            "berry_links": links,
            "berry_links_err": scatter(step_links),
            "walkers": all_values["walkers"].sum(),
        }


DEFAULT = HoleOverlapEstimator  # Useful in CLI
