"""Excited states by overlap penalties against frozen lower states (not in the reference).

Minimise, on walkers x_b ~ |psi|^2,

    L(p) = E[psi_p] + sum_k lambda_k F_k(p),      F_k = |<phi_k|psi>|^2 / (<phi_k|phi_k> <psi|psi>)

against frozen states phi_k: for lambda_k above the gap to phi_k the minimum is the lowest state
orthogonal to them.  With d_kb = log phi_k(x_b) - log psi(x_b), r_kb = e^{d_kb} and
eps_kb = 1 - r_kb / mean_b(r_k) (pretrain.py), dF_k/dp = -F_k 2 Re mean(conj(O) eps_k), so

    dL/dp = 2 Re mean_b conj(O_b) [ (E_L,b - <E_L>) - sum_k lambda_k F_k eps_kb ]

and the per-walker residual R_b = E_L,b - sum_k w_k eps_kb, w_k = lambda_k F_k, takes the local
energy's place in front of every optimizer (``make_loss_fn(..., residual=)``); its mean is the
energy, because every eps_k has mean zero.

The sums and R run in csrc/orthogonal.hip (dh_ortho_partial: one launch, one workgroup per state;
dh_ortho_residual: one thread per walker).  Across ranks the K x DH_NFID partial sums are combined
after one all-gather, on the device; w stays there as a float64 tensor.

A frozen state is a trial state of this library (the ``subspace`` estimator's entries) or a
Psiformer checkpoint.  A frozen Psiformer gets a native handle of its own (``handle_tag`` in its
spec): with the run's own architecture it would share the trained network's handle, and every
iteration would pack both parameter sets in turn.  So its parameters are packed once per run.
"""

from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import math
import re
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, constants
from .config import Config, NetworkType, OptimizerName
from .hamiltonian import _run_local_energy
from .mcmc import resolve_network
from .networks import make_network, psiformer
from .networks.psiformer import ParamTree, _ptr, _stream, flat_params, param_shapes

MAX_STATES = _lib.DH_ORTHO_MAX_STATES
_TAGS = itertools.count()


# ---- the kernels ------------------------------------------------------------------------------

def _check_logs(logpsi: torch.Tensor, logphi: torch.Tensor):
    if not (logpsi.is_cuda and logphi.is_cuda):
        raise RuntimeError("the overlap-penalty kernels run on the GPU (HIP kernels); got a CPU tensor")
    if logpsi.is_complex():
        logpsi = torch.view_as_real(logpsi)
    if logphi.is_complex():
        logphi = torch.view_as_real(logphi)
    logpsi, logphi = logpsi.contiguous().float(), logphi.contiguous().float()
    if logpsi.dim() != 2 or logpsi.shape[1] != 2 or logphi.dim() != 3 or logphi.shape[1:] != logpsi.shape:
        raise ValueError("log psi must be [B, 2] (re, im) or complex [B], log phi [K, B, 2] or complex [K, B]")
    if not 1 <= logphi.shape[0] <= MAX_STATES:
        raise ValueError(f"1 to {MAX_STATES} states, got {logphi.shape[0]}")
    return logpsi, logphi


def ortho_partial(logpsi: torch.Tensor, logphi: torch.Tensor) -> torch.Tensor:
    """dh_ortho_partial: float64 [K, DH_NFID], row k = (m, S re, S im, S2, n) of these walkers
    against state k (``pretrain.fidelity_partial`` on state k, bit for bit), on the device."""
    logpsi, logphi = _check_logs(logpsi, logphi)
    K, B = logphi.shape[0], logpsi.shape[0]
    part = torch.empty(K, _lib.DH_NFID, dtype=torch.float64, device=logpsi.device)
    _lib.check(_lib.load().dh_ortho_partial(_ptr(logpsi), _ptr(logphi), B, K, _ptr(part), _stream(logpsi.device)))
    return part


def ortho_residual(logpsi: torch.Tensor, logphi: torch.Tensor, total: torch.Tensor, weight: torch.Tensor,
                   e_l: torch.Tensor | None = None) -> torch.Tensor:
    """dh_ortho_residual: out_b = (e_l_b or 0) - sum_k weight_k (1 - n_k e^{d_kb - m_k} / S_k),
    float32 [B, 2], from the (combined) sums ``total`` float64 [K, DH_NFID] and ``weight`` float64
    [K]; NaN for a walker invalid for any state, all NaN when a state has n = 0, S = 0 or a
    non-finite weight."""
    logpsi, logphi = _check_logs(logpsi, logphi)
    K, B = logphi.shape[0], logpsi.shape[0]
    total = total.to(device=logpsi.device, dtype=torch.float64).contiguous()
    weight = weight.to(device=logpsi.device, dtype=torch.float64).contiguous()
    if tuple(total.shape) != (K, _lib.DH_NFID) or tuple(weight.shape) != (K,):
        raise ValueError(f"total must be [{K}, {_lib.DH_NFID}] and weight [{K}]")
    if e_l is not None:
        e_l = e_l.to(device=logpsi.device, dtype=torch.float32).contiguous()
        if e_l.shape != logpsi.shape:
            raise ValueError(f"e_l must be [{B}, 2]")
    out = torch.empty(B, 2, dtype=torch.float32, device=logpsi.device)
    _lib.check(_lib.load().dh_ortho_residual(_ptr(logpsi), _ptr(logphi), B, K, _ptr(total), _ptr(weight), _ptr(e_l),
                                             _ptr(out), _stream(logpsi.device)))
    return out


def gather_state_partials(part: torch.Tensor) -> torch.Tensor:
    """This rank's [K, DH_NFID] -> [world size, K, DH_NFID]: one all-gather of K x DH_NFID doubles per rank."""
    if constants.world_size() == 1:
        return part.unsqueeze(0)
    parts = [torch.empty_like(part) for _ in range(constants.world_size())]
    dist.all_gather(parts, part)
    return torch.stack(parts)


def combine_state_partials(parts: torch.Tensor):
    """``pretrain.combine_partials`` for every state at once: ``parts`` float64 [R, K, DH_NFID] (or
    [K, DH_NFID]) -> (total [K, DH_NFID], F [K]), its formulas along the rank axis with the state
    axis carried beside it.  Pure torch on the tensor's own device, no host read."""
    p = parts.reshape(-1, parts.shape[-2], _lib.DH_NFID).to(torch.float64)
    m, n = p[..., 0], p[..., 4]
    live = n > 0
    ninf = torch.full_like(m, float("-inf"))
    zero = torch.zeros_like(m)
    M = torch.where(live, m, ninf).max(dim=0).values
    shift = torch.where(live, m - M, zero)
    w1 = torch.where(live, torch.exp(shift), zero)
    w2 = torch.where(live, torch.exp(2.0 * shift), zero)
    s_re = (torch.where(live, p[..., 1], zero) * w1).sum(dim=0)
    s_im = (torch.where(live, p[..., 2], zero) * w1).sum(dim=0)
    s2 = (torch.where(live, p[..., 3], zero) * w2).sum(dim=0)
    nn = torch.where(live, n, zero).sum(dim=0)
    fidelity = (s_re * s_re + s_im * s_im) / (nn * s2)
    return torch.stack([M, s_re, s_im, s2, nn], dim=-1), fidelity


# ---- frozen states ------------------------------------------------------------------------------

class FrozenPsiformer:
    """A Psiformer with fixed parameters as a parameter-free state: ``apply(_, data)`` is its log
    psi.  The network's spec carries a ``handle_tag``, so the native handle is this state's alone
    and the parameters, copied once per device into a flat tree that nobody updates, are packed
    into it once."""

    def __init__(self, network, params):
        net = resolve_network(network)
        self.network = net.with_system()
        self.network.spec = dataclasses.replace(net.spec, handle_tag=f"frozen-{next(_TAGS)}")
        self._source = params
        self._params: dict = {}

    def params_on(self, device) -> ParamTree:
        device = torch.device(device)
        if device not in self._params:
            spec = self.network.spec
            flat = flat_params(spec, self._source, device)
            if isinstance(self._source, ParamTree) and flat is getattr(self._source, "flat", None):
                flat = flat.clone()  # the source may go on training
            self._params[device] = ParamTree.view_of(spec, flat)
        return self._params[device]

    def apply(self, params, data: torch.Tensor) -> torch.Tensor:
        del params
        return self.network.apply(self.params_on(data.device), data)

    __call__ = apply

    def release(self):
        """Give the native handles (a packed copy of the weights and the workspaces, per device) and
        the device copies of the parameters back.  The handle cache keeps every spec it has seen,
        and this state's tag is its alone, so nothing else would; dropping the state calls this.
        A later ``apply`` builds them again."""
        spec = self.network.spec
        for key in [k for k in psiformer._HANDLES if k[0] == spec]:
            del psiformer._HANDLES[key]
        self._params.clear()

    def __del__(self):
        try:
            self.release()
        except Exception:  # noqa: BLE001  (interpreter teardown)
            pass


def frozen_psiformer(network, params) -> FrozenPsiformer:
    """``params`` (a ParamTree or {Flax path: tensor}) frozen into a state of ``network``'s architecture."""
    return FrozenPsiformer(network, params)


def resolve_checkpoint(path) -> Path:
    """A checkpoint file itself, or the newest ``ckpt_<step>.npz`` of a directory: the largest step
    number, whatever its padding (files whose name holds no number are not checkpoints of this
    library and are passed over).  ``ValueError`` when there is none."""
    p = Path(path)
    if p.is_dir():
        found = [(int(m.group(1)), f) for f in p.glob("ckpt_*.npz") if (m := re.fullmatch(r"ckpt_(\d+)\.npz", f.name))]
        if not found:
            raise ValueError(f"no ckpt_*.npz in {p}")
        return max(found)[1]
    if not p.is_file():
        raise ValueError(f"checkpoint {p} does not exist")
    return p


def load_checkpoint_params(path, spec) -> ParamTree:
    """The ``params/<name>`` arrays of a checkpoint as a ParamTree of ``spec`` on the host.
    ``ValueError`` naming the file when it cannot be read, the tensor when one is missing or mis-shaped."""
    path = resolve_checkpoint(path)
    try:
        with np.load(path, allow_pickle=False) as f:
            arrays = {k: np.asarray(f[k]) for k in f.files if k.startswith("params/")}
    except Exception as e:  # noqa: BLE001  (not an npz, truncated, unreadable)
        raise ValueError(f"checkpoint {path} cannot be read: {e}") from e
    tree = ParamTree.zeros(spec, "cpu")
    for name, shape in param_shapes(spec).items():
        key = f"params/{name}"
        if key not in arrays:
            raise ValueError(f"checkpoint {path}: tensor {key} is missing")
        a = arrays[key]
        if tuple(a.shape) != tuple(shape) or a.dtype.kind not in "fiu":
            raise ValueError(f"checkpoint {path}: tensor {key} has shape {tuple(a.shape)} ({a.dtype}), "
                             f"this architecture needs {tuple(shape)}")
        tree[name].copy_(torch.as_tensor(a.astype(np.float32)))
    return tree


def _optimizer_name(cfg: Config) -> OptimizerName:
    name = cfg.optim.optimizer
    return OptimizerName(getattr(name, "value", name)) if name is not None else OptimizerName.none


def _penalty(value, where: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{where}: penalty must be a number, got {value!r}") from e
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{where}: penalty must be finite and >= 0, got {value!r}")
    return v


def _checkpoint_state(cfg: Config, entry: dict, where: str):
    extra = set(entry) - {"type", "checkpoint", "psiformer", "orbital"}
    if extra:
        raise ValueError(f"{where}: a checkpoint entry takes checkpoint, psiformer, orbital and penalty, got {sorted(extra)}")
    try:
        sub = dataclasses.replace(cfg.network.psiformer, **(entry.get("psiformer") or {}))
        network = dataclasses.replace(cfg.network, type=NetworkType.psiformer, psiformer=sub,
                                      orbital=entry.get("orbital", cfg.network.orbital))
        net = make_network(cfg.system, network)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{where}: {e}") from e
    try:
        params = load_checkpoint_params(entry["checkpoint"], net.spec)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from e
    return frozen_psiformer(net, params)


def _trial_state(cfg: Config, entry: dict, c: int, where: str):
    from .netobs.observables.subspace import state_network

    try:
        net = state_network(cfg, entry, c)
    except ValueError as e:
        raise ValueError(str(e).replace("subspace:", "optim.orthogonal:", 1)) from e
    # dh_create is host code: the refusal a device handle would meet later (pretrain.make_reference)
    lib = _lib.load()
    h = C.c_void_p()
    if net.spec.create(lib, h) != 0:
        raise ValueError(f"{where}: no {entry['type']} trial state at N = {sum(cfg.system.nspins)}, "
                         f"flux = {cfg.system.flux}: {lib.dh_last_error().decode(errors='replace')}")
    lib.dh_destroy(h)
    return net


def make_states(cfg: Config):
    """``(states, penalties)`` of ``cfg.optim.orthogonal``: the frozen states in the configuration's
    order and lambda_k of each (the entry's ``penalty``, else ``optim.orthogonal.penalty``).

    An entry is a trial state in the ``subspace`` estimator's form, ``{type: laughlin | jain |
    pfaffian | halperin | quasihole, <sub-configs>}``, built at the run's own system, or a Psiformer
    checkpoint ``{checkpoint: <file or directory>, psiformer: {...}?, orbital: ...?}`` — a directory
    means its newest ``ckpt_*.npz`` — of the run's own architecture unless the entry overrides it.
    ``ValueError``, from host checks only: more than 16 states, a negative or non-finite penalty,
    an unknown type, ``type: psiformer`` without ``checkpoint``, an unreadable checkpoint or one
    with a missing or mis-shaped tensor, a trial state that does not exist at this N and flux, a
    ``network.type`` other than psiformer, optimizer ``none``."""
    orth = cfg.optim.orthogonal
    entries = tuple(orth.states or ())
    if _optimizer_name(cfg) == OptimizerName.none:
        raise ValueError("optim.orthogonal needs an optimizer (adam, kfac or minsr), not 'none'")
    run_type = str(getattr(cfg.network.type, "value", cfg.network.type))
    if run_type != NetworkType.psiformer.value:
        raise ValueError(f"optim.orthogonal trains a Psiformer; network.type is {run_type!r}, which has no parameters")
    if len(entries) > MAX_STATES:
        raise ValueError(f"optim.orthogonal: at most {MAX_STATES} states, got {len(entries)}")
    default = _penalty(orth.penalty, "optim.orthogonal")
    states, penalties = [], []
    for c, entry in enumerate(entries):
        where = f"optim.orthogonal: state {c}"
        if not isinstance(entry, dict):
            raise ValueError(f"{where} must be a dict of type or checkpoint, got {entry!r}")
        entry = dict(entry)
        penalties.append(_penalty(entry.pop("penalty"), where) if "penalty" in entry else default)
        ntype = str(getattr(entry.get("type"), "value", entry.get("type")))
        if "checkpoint" in entry:
            if "type" in entry and ntype != "psiformer":
                raise ValueError(f"{where}: a checkpoint entry is a psiformer, not {ntype!r}")
            states.append(_checkpoint_state(cfg, entry, where))
        elif ntype == "psiformer":
            raise ValueError(f"{where}: type psiformer needs a checkpoint (a file or a directory of ckpt_*.npz)")
        else:
            states.append(_trial_state(cfg, entry, c, where))
    return states, penalties


# ---- the residual -------------------------------------------------------------------------------

def make_orthogonal_residual(network, states, penalties, energy: bool = True):
    """``residual(params, data) -> (R [B, 2], obs [B, 8])`` for ``make_loss_fn(..., residual=)``:
    R_b = E_L,b - sum_k lambda_k F_k eps_kb of this rank's walkers against ``states`` (parameter-free
    networks of this library or ``FrozenPsiformer``s), normalised with the sums of every rank's
    walkers.  Per call: one dh_local_energy of the trained network, whose ``obs[:, 6:8]`` is log psi
    (no second forward pass), one log psi per state, dh_ortho_partial, dh_ortho_residual.  The hook
    is marked ``keeps_energy``: the loss reports E_L's statistics and centres with R's.

    ``energy=False``: the repulsion alone, R_b = -sum_k lambda_k F_k eps_kb with ``obs`` zero except
    log psi, unmarked — ``pretrain.make_fidelity_residual``'s protocol with the sign of descent; this
    form alone also sets ``last_fidelity``, which that protocol reports as ``stats["fidelity"]``: the
    [K] tensor where the fidelity hook's is a scalar.

    After a call: ``last_fidelities`` [K] float64, ``last_penalty`` = sum_k lambda_k F_k (0-d
    float64), both on the device, and ``last_energy`` = (e_l, obs) of the unpenalised local energy
    (None without it)."""
    net = resolve_network(network)
    states = list(states)
    if not 1 <= len(states) <= MAX_STATES:
        raise ValueError(f"1 to {MAX_STATES} states, got {len(states)}")
    lam = [_penalty(v, f"state {k}") for k, v in enumerate(penalties)]
    if len(lam) != len(states):
        raise ValueError(f"{len(states)} states but {len(lam)} penalties")
    lam_on: dict = {}

    def residual(params, data: torch.Tensor):
        if energy:
            e_l, obs = _run_local_energy(net, params, data)
            logpsi = obs[:, 6:8].contiguous()
        else:
            e_l = None
            logpsi = torch.view_as_real(net.apply(params, data)).contiguous()
            obs = torch.zeros(data.shape[0], 8, dtype=torch.float32, device=data.device)
            obs[:, 6:8] = logpsi
        logphi = torch.stack([torch.view_as_real(s.apply({}, data)) for s in states]).float().contiguous()
        total, fid = combine_state_partials(gather_state_partials(ortho_partial(logpsi, logphi)))
        if data.device not in lam_on:
            lam_on[data.device] = torch.tensor(lam, dtype=torch.float64, device=data.device)
        weight = lam_on[data.device] * fid
        r = ortho_residual(logpsi, logphi, total, weight, e_l)
        residual.last_fidelities = fid
        if not energy:  # the unmarked protocol reports ``last_fidelity``: here the [K] tensor, not a scalar
            residual.last_fidelity = fid
        residual.last_penalty = weight.sum()
        residual.last_energy = (e_l, obs) if energy else None
        return r, obs

    residual.network = net
    residual.states = states
    residual.penalties = tuple(lam)
    residual.keeps_energy = bool(energy)
    residual.last_fidelities = residual.last_penalty = residual.last_energy = None
    if not energy:
        residual.last_fidelity = None
    return residual


__all__ = ["ortho_partial", "ortho_residual", "gather_state_partials", "combine_state_partials", "FrozenPsiformer",
           "frozen_psiformer", "resolve_checkpoint", "load_checkpoint_params", "make_states",
           "make_orthogonal_residual", "MAX_STATES"]
