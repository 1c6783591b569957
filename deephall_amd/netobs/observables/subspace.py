"""Energies in the span of K wavefunctions: the overlap and Hamiltonian matrices on one set of walkers.

Not in the reference.  State 0 is the adaptor's own network with ``params`` (of any type), and the
walkers sample |psi_0|^2.  ``estimator_options["states"]`` lists the others, each a dict with a
``type`` (``laughlin``, ``jain``, ``pfaffian``, ``halperin``, ``quasihole``) and, optionally, sub-configs
by the names of ``cfg.network`` (``{"type": "jain", "jain": {"occupation": ...}}``); what an entry does
not name comes from ``cfg.network``, and every state is built at the run's own system.  A
``psiformer`` entry is an error: its parameters exist only for state 0.  K = 1 + len(states) <= 32.
With r_c = psi_c / psi_0 on a walker,

    S[c, c'] = <conj(r_c) r_c'>,   H[c, c'] = <conj(r_c) r_c' E_c'>,   T[c, c'] = <conj(r_c) r_c' KE_c'>

estimate <psi_c | psi_c'>, <psi_c | H | psi_c'> and the kinetic part of the latter up to one common
factor; E_c and KE_c are the local energy (impurities included) and the kinetic energy of state c.
The operator acts on the ket, so a finite sample of H is not Hermitian; ``netobs.subspace.solve``
Hermitises it, drops the linearly dependent directions of S (``rank_tol``) and solves H v = E S v.

Per step one ``dh_local_energy`` call per state gives E_c, KE_c and log psi_c of every walker, and
``dh_subspace_accumulate`` (csrc/subspace.hip) the three K x K sums in double: a fixed order, no
float atomics, a walker with a non-finite input or ratio dropped whole.  The real shift[c] that
keeps exp in range is the walker mean of Re (log psi_c - log psi_0) of the first evaluated step and
stays in the state: every step's matrices are in the same units, so step sums add.

The walkers sample |psi_0|^2 alone: the variance of S[c, c] is that of |psi_c / psi_0|^2, so psi_0
should not vanish where the other states do not.

Step values ``gram``, ``hamiltonian``, ``kinetic`` [1, K, K] complex128 (the sums / valid walkers; NaN
with none) and ``walkers`` [1].  Digest over the steps that are not NaN: the mean ``gram``,
``hamiltonian``, ``kinetic`` and ``potential`` = hamiltonian - kinetic, the normalised ``overlap``,
``energies`` (ascending), ``energies_err`` (delete-one-step jackknife), ``vectors`` [K, rank], ``rank``,
``asymmetry`` (max |H - H^H| / max |H|) and, for each s of ``strengths``, ``energies@s``: the spectrum
of T + (s / the run's interaction_strength) V, the same Hamiltonian at the interaction strength s
(the Landau-level-mixing parameter) without another run.
"""

from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from ... import _lib
from ...config import NetworkType
from ...hamiltonian import _run_local_energy
from ...networks import make_network
from .. import holonomy, subspace
from .._native import subspace_sums
from ..estimator import Estimator, Observable

STATE_TYPES = ("laughlin", "jain", "pfaffian", "halperin", "quasihole")
SUB_CONFIGS = ("jain", "pfaffian", "halperin", "quasihole")


def state_network(cfg, entry, c: int):
    """The network of state c >= 1: ``entry``'s type at ``cfg.system``, its sub-configs over ``cfg.network``'s."""
    if not isinstance(entry, dict) or "type" not in entry or set(entry) - {"type", *SUB_CONFIGS}:
        raise ValueError(f"subspace: state {c} must be a dict of type and any of {SUB_CONFIGS}, got {entry!r}")
    ntype = str(getattr(entry["type"], "value", entry["type"]))
    if ntype == "psiformer":
        raise ValueError(f"subspace: state {c} is a psiformer; its parameters exist only for state 0, the run's own network")
    if ntype not in STATE_TYPES:
        raise ValueError(f"subspace: state {c} has the unknown type {ntype!r}; one of {STATE_TYPES}")
    try:
        subs = {}
        for name in SUB_CONFIGS:
            if name in entry:
                if not isinstance(entry[name], dict):
                    raise ValueError(f"{name} must be a dict, got {entry[name]!r}")
                subs[name] = dataclasses.replace(getattr(cfg.network, name), **entry[name])
        return make_network(cfg.system, dataclasses.replace(cfg.network, type=NetworkType(ntype), **subs))
    except (TypeError, ValueError) as e:
        raise ValueError(f"subspace: state {c}: {e}") from e


class Subspace(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        return ()


class SubspaceEstimator(Estimator):
    observable_type = Subspace

    def __init__(self, adaptor, system, estimator_options, observable_options):
        super().__init__(adaptor, system, estimator_options, observable_options)
        cfg = adaptor.cfg
        states = self.options.get("states", ())
        if not isinstance(states, (list, tuple)):
            raise ValueError(f"subspace: states must be a list of {{type, ...}}, got {states!r}")
        self.K = 1 + len(states)
        if self.K > _lib.DH_SUBSPACE_MAX_STATES:
            raise ValueError(f"subspace: at most {_lib.DH_SUBSPACE_MAX_STATES} states with the run's own, got {self.K}")
        self.rank_tol = float(self.options.get("rank_tol", 1e-8))
        if not self.rank_tol > 0.0:
            raise ValueError(f"subspace: rank_tol must be > 0, got {self.rank_tol}")
        self.strengths = [float(s) for s in self.options.get("strengths") or ()]
        self.strength = float(cfg.system.interaction_strength)
        if self.strengths and (self.strength == 0.0 or cfg.system.impurities):
            raise ValueError("subspace: strengths rescale hamiltonian - kinetic, which must be the pair interaction "
                             "alone and not zero (interaction_strength != 0, no impurities)")
        model = getattr(adaptor, "model", None)
        self.networks = [model if model is not None else make_network(cfg.system, cfg.network)]  # state 0
        self.networks += [state_network(cfg, entry, c + 1) for c, entry in enumerate(states)]

    def empty_val_state(self, steps: int):
        mats = {k: torch.zeros((steps, self.K, self.K), dtype=torch.complex128) for k in ("gram", "hamiltonian", "kinetic")}
        return {**mats, "walkers": torch.zeros(steps, dtype=torch.float64)}, {"shift": None}

    def local_energies(self, params, x):
        """(logs, e_l, ke) [K, B, 2] float32 on the device: one dh_local_energy call per state."""
        logs, e_ls, kes = [], [], []
        for c, net in enumerate(self.networks):
            e_l, obs, _ = _run_local_energy(net, params if c == 0 else {}, x, external=True)
            logs.append(obs[:, 6:8])
            e_ls.append(e_l)
            kes.append(obs[:, 0:2])
        return torch.stack(logs), torch.stack(e_ls), torch.stack(kes)

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, key, system, aux_data
        x = data.reshape(-1, *data.shape[-2:])
        logs, e_l, ke = self.local_energies(params, x)
        if state.get("shift") is None:
            d = logs[:, :, 0].double() - logs[:1, :, 0].double()
            state["shift"] = torch.nan_to_num(torch.where(torch.isfinite(d), d, torch.nan).nanmean(dim=1)).cpu()
        out, nvalid = subspace_sums(logs, e_l, ke, state["shift"])
        out = (out / nvalid).cpu()  # nvalid = 0: NaN, which the driver's mean and the digest drop
        return {"gram": out[0][None], "hamiltonian": out[1][None], "kinetic": out[2][None],
                "walkers": torch.tensor([float(nvalid)], dtype=torch.float64)}, state

    def digest(self, all_values, state):
        del state
        names = ("gram", "hamiltonian", "kinetic")
        steps = {k: torch.as_tensor(all_values[k]).to(torch.complex128) for k in names}
        keep = torch.ones(steps["gram"].shape[0], dtype=torch.bool)
        for v in steps.values():
            keep &= torch.isfinite(torch.view_as_real(v)).reshape(v.shape[0], -1).all(dim=1)
        steps = {k: v[keep].numpy() for k, v in steps.items()}
        out = {"walkers": torch.as_tensor(all_values["walkers"])[keep].sum(), "steps": int(keep.sum())}
        if not keep.any():
            nan = torch.full((self.K, self.K), complex(math.nan, math.nan), dtype=torch.complex128)
            out.update({k: nan.clone() for k in (*names, "potential", "overlap")})
            out.update(energies=torch.full((0,), math.nan, dtype=torch.float64), rank=0, asymmetry=math.nan,
                       energies_err=torch.full((0,), math.nan, dtype=torch.float64),
                       vectors=torch.zeros((self.K, 0), dtype=torch.complex128))
            return out
        S, H, T = (steps[k].mean(axis=0) for k in names)
        sol = subspace.solve(S, H, self.rank_tol)
        out.update(gram=torch.from_numpy(S), hamiltonian=torch.from_numpy(H), kinetic=torch.from_numpy(T),
                   potential=torch.from_numpy(H - T), overlap=holonomy.overlap_matrix(torch.from_numpy(S)),
                   energies=torch.from_numpy(sol.energies), vectors=torch.from_numpy(sol.vectors), rank=sol.rank,
                   asymmetry=sol.asymmetry,
                   energies_err=torch.from_numpy(subspace.jackknife(steps["gram"], steps["hamiltonian"], self.rank_tol)))
        for s in self.strengths:
            priced = subspace.reprice(S, T, H - T, s / self.strength, self.rank_tol)
            out[f"energies@{s:g}"] = torch.from_numpy(priced.energies)
        return out


DEFAULT = SubspaceEstimator  # Useful in CLI
