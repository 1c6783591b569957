"""Fidelity pretraining: pull the randomly initialised Psiformer onto an analytic trial state
before the energy minimisation (not in the reference; FermiNet and Psiformer pretrain on
Hartree-Fock, here the native Laughlin, Jain, Moore-Read, Halperin and quasihole states play that role).

Walkers x_b come from |psi|^2 (the existing dh_mcmc_step); phi is the trial state,
d_b = log phi(x_b) - log psi(x_b), r_b = e^{d_b}:

    F = |<phi|psi>|^2 / (<phi|phi> <psi|psi>) = |mean r|^2 / mean |r|^2
    d(-log F)/dp = 2 Re mean(conj(d log psi / dp) eps),      eps_b = 1 - r_b / mean(r)

which is the energy gradient's shape with eps in the place of E_L - <E_L>.  So eps is handed to
the energy chain as if it were a local energy (``make_loss_fn(..., residual=...)``):
dh_energy_stats, dh_loss_diff (centring, IQR clip), dh_grad_cotangent, dh_logpsi_vjp /
dh_kfac_vjp, and MinSR / SPRING's residual — every optimizer applies as it is, and their Fisher
/ Gram matrices stay defined on |psi|^2 samples because the sampling stays there.

The sums run in csrc/fidelity.hip (dh_fidelity_partial, dh_fidelity_residual) in double with the
largest Re d taken out first: trial states carry no normalisation.  Across ranks the partial
sums of the shards are combined after one all-gather of DH_NFID doubles per rank.
"""

from __future__ import annotations

import ctypes as C
import dataclasses
import logging

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, constants
from .config import Config, NetworkType, OptimizerName
from .mcmc import resolve_network, update_mcmc_width
from .networks import make_network
from .networks.psiformer import _ptr, _stream

logger = logging.getLogger("deephall_amd")

REFERENCES = ("laughlin", "jain", "pfaffian", "halperin", "quasihole")


def _check_logs(logpsi: torch.Tensor, logphi: torch.Tensor):
    if not (logpsi.is_cuda and logphi.is_cuda):
        raise RuntimeError("the fidelity kernels run on the GPU (HIP kernels); got a CPU tensor")
    if logpsi.is_complex():
        logpsi = torch.view_as_real(logpsi)
    if logphi.is_complex():
        logphi = torch.view_as_real(logphi)
    logpsi, logphi = logpsi.contiguous().float(), logphi.contiguous().float()
    if logpsi.dim() != 2 or logpsi.shape[1] != 2 or logphi.shape != logpsi.shape:
        raise ValueError("log psi and log phi must both be [B, 2] (re, im) or complex [B]")
    return logpsi, logphi


def fidelity_partial(logpsi: torch.Tensor, logphi: torch.Tensor) -> torch.Tensor:
    """dh_fidelity_partial: float64 [DH_NFID] = (m, S re, S im, S2, n) of these walkers, on the
    device.  ``logpsi``, ``logphi``: float32 [B, 2] (re, im) or complex [B]."""
    logpsi, logphi = _check_logs(logpsi, logphi)
    part = torch.empty(_lib.DH_NFID, dtype=torch.float64, device=logpsi.device)
    _lib.check(_lib.load().dh_fidelity_partial(_ptr(logpsi), _ptr(logphi), logpsi.shape[0], _ptr(part),
                                               _stream(logpsi.device)))
    return part


def combine_partials(parts: torch.Tensor):
    """The partial sums of several shards as one: ``parts`` float64 [R, DH_NFID] (or [DH_NFID]) ->
    (total float64 [DH_NFID], F 0-d float64).  M = max m_r, S = sum S_r e^{m_r - M},
    S2 = sum S2_r e^{2 (m_r - M)}, n = sum n_r over the shards with n_r > 0, and
    F = |S|^2 / (n S2) (NaN when no shard has a valid walker).  Pure torch on the tensor's own
    device, no host read."""
    p = parts.reshape(-1, _lib.DH_NFID).to(torch.float64)
    m, n = p[:, 0], p[:, 4]
    live = n > 0
    ninf = torch.full_like(m, float("-inf"))
    zero = torch.zeros_like(m)
    M = torch.where(live, m, ninf).max()
    shift = torch.where(live, m - M, zero)
    w1 = torch.where(live, torch.exp(shift), zero)
    w2 = torch.where(live, torch.exp(2.0 * shift), zero)
    s_re = (torch.where(live, p[:, 1], zero) * w1).sum()
    s_im = (torch.where(live, p[:, 2], zero) * w1).sum()
    s2 = (torch.where(live, p[:, 3], zero) * w2).sum()
    nn = torch.where(live, n, zero).sum()
    fidelity = (s_re * s_re + s_im * s_im) / (nn * s2)
    return torch.stack([M, s_re, s_im, s2, nn]), fidelity


def fidelity_residual(logpsi: torch.Tensor, logphi: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
    """dh_fidelity_residual: eps_b = 1 - n e^{d_b - m} / S, float32 [B, 2], from the (combined)
    sums ``total`` float64 [DH_NFID]; NaN for invalid walkers, all NaN when n = 0 or S = 0."""
    logpsi, logphi = _check_logs(logpsi, logphi)
    total = total.to(device=logpsi.device, dtype=torch.float64).contiguous()
    if total.numel() != _lib.DH_NFID:
        raise ValueError(f"total must hold {_lib.DH_NFID} doubles")
    resid = torch.empty(logpsi.shape[0], 2, dtype=torch.float32, device=logpsi.device)
    _lib.check(_lib.load().dh_fidelity_residual(_ptr(logpsi), _ptr(logphi), logpsi.shape[0], _ptr(total), _ptr(resid),
                                                _stream(logpsi.device)))
    return resid


def gather_partials(part: torch.Tensor) -> torch.Tensor:
    """This rank's partial -> [world size, DH_NFID]: one all-gather of DH_NFID doubles per rank."""
    if constants.world_size() == 1:
        return part.view(1, -1)
    parts = [torch.empty_like(part) for _ in range(constants.world_size())]
    dist.all_gather(parts, part)
    return torch.stack(parts)


def make_fidelity_residual(network, reference):
    """``residual(params, data) -> (e_l [B, 2], obs [B, 8])`` for ``make_loss_fn(..., residual=)``:
    eps of this rank's walkers against the trial state ``reference`` (a parameter-free network of
    this library), normalised with the sums of every rank's walkers, in the place of the local
    energy; ``obs`` is zero except log psi in columns 6-7.  ``residual.last_fidelity`` is the
    fidelity of the whole batch (0-d float64 on the device)."""
    net = resolve_network(network)
    ref = resolve_network(reference)

    def residual(params, data: torch.Tensor):
        logpsi = torch.view_as_real(net.apply(params, data)).contiguous()
        logphi = torch.view_as_real(ref.apply({}, data)).contiguous()
        total, fidelity = combine_partials(gather_partials(fidelity_partial(logpsi, logphi)))
        eps = fidelity_residual(logpsi, logphi, total)
        obs = torch.zeros(data.shape[0], 8, dtype=torch.float32, device=data.device)
        obs[:, 6:8] = logpsi
        residual.last_fidelity = fidelity
        return eps, obs

    residual.network = net
    residual.reference = ref
    residual.last_fidelity = None
    return residual


def _optimizer_name(cfg: Config) -> OptimizerName:
    name = cfg.optim.optimizer
    return OptimizerName(getattr(name, "value", name)) if name is not None else OptimizerName.none


def make_reference(cfg: Config):
    """The trial state of ``cfg.optim.pretrain.reference`` for the run's system, built as the
    overlap estimator builds it.  ``ValueError`` — from host checks only, before any device call
    — when the optimizer is ``none``, the network is not a Psiformer, or the trial state does not
    exist at this N and flux (the library's own dh_create refuses it)."""
    pre = cfg.optim.pretrain
    if _optimizer_name(cfg) == OptimizerName.none:
        raise ValueError("optim.pretrain needs an optimizer (adam, kfac or minsr), not 'none'")
    ntype = str(getattr(cfg.network.type, "value", cfg.network.type))
    if ntype != NetworkType.psiformer.value:
        raise ValueError(f"optim.pretrain trains a Psiformer; network.type is {ntype!r}, which has no parameters")
    name = str(getattr(pre.reference, "value", pre.reference))
    if name not in REFERENCES:
        raise ValueError(f"optim.pretrain.reference must be one of {REFERENCES}, got {name!r}")
    where = f"N = {sum(cfg.system.nspins)}, flux = {cfg.system.flux}"
    try:
        ref = make_network(cfg.system, dataclasses.replace(cfg.network, type=NetworkType(name)))
    except ValueError as e:
        raise ValueError(f"optim.pretrain: no {name} trial state at {where}: {e}") from e
    # dh_create is host code: the same refusal a device handle would meet later
    lib = _lib.load()
    h = C.c_void_p()
    rc = ref.spec.create(lib, h)
    if rc != 0:
        raise ValueError(f"optim.pretrain: no {name} trial state at {where}: "
                         f"{lib.dh_last_error().decode(errors='replace')}")
    lib.dh_destroy(h)
    return ref


def _pretrain_config(cfg: Config) -> Config:
    """``cfg`` with ``optim.pretrain.lr`` (when given) as the chosen optimizer's schedule."""
    lr = cfg.optim.pretrain.lr
    if lr is None:
        return cfg
    name = _optimizer_name(cfg).value
    sub = dataclasses.replace(getattr(cfg.optim, name), lr=lr)
    return dataclasses.replace(cfg, optim=dataclasses.replace(cfg.optim, **{name: sub}))


def pretrain(cfg: Config, model, state, mcmc_step, key, writer=None):
    """``cfg.optim.pretrain.iterations`` iterations of fidelity ascent towards the trial state:
    ``mcmc_step`` (walkers from |psi|^2), the chosen optimizer's training step with eps as the
    residual, ``update_mcmc_width``.  Returns ``(state, key, history)``; ``history`` has one row
    per iteration (step, pmove, fidelity, variance of eps), also written to ``writer``
    (log.StatsWriter) when given.

    The optimizer state is created here (its schedule starts at t = 0) and returned in ``state``;
    the caller re-creates it for the energy minimisation, so Adam moments, KFAC factors and
    SPRING's previous direction do not carry over, while the walkers and the MCMC width do.
    Pretraining is not resumable: it runs only on a fresh start, a checkpoint restore skips it,
    and a run killed during it starts it over."""
    from .optimizers import make_optimizer_step
    from .types import CheckpointState

    pre = cfg.optim.pretrain
    reference = make_reference(cfg)
    residual = make_fidelity_residual(model, reference)
    opt_init, training_step = make_optimizer_step(_pretrain_config(cfg), model, residual=residual)
    params, data, _, width = state
    state = CheckpointState(params, data, opt_init(params, None, data), width)
    steps = cfg.mcmc.steps
    pmoves = np.zeros(cfg.mcmc.adapt_frequency)
    history = []
    for t in range(int(pre.iterations)):
        new_data, _ = mcmc_step(state.params, state.data, key, state.mcmc_width, reduce=False)
        n_accept = mcmc_step.last_n_accept
        key = key.advance(steps)
        state = state._replace(data=new_data)
        state, stats = training_step(state, None, n_accept=n_accept, steps=steps)
        pmove = float(stats["pmove"])
        new_width, pmoves = update_mcmc_width(t, state.mcmc_width, cfg.mcmc.adapt_frequency, pmove, pmoves)
        state = state._replace(mcmc_width=new_width)
        row = {"step": t, "pmove": pmove, "fidelity": float(stats["fidelity"]), "variance": float(stats["variance"])}
        history.append(row)
        if writer is not None:
            writer.log(step=str(t), pmove=f"{pmove:.2f}", fidelity=f"{row['fidelity']:.6f}",
                       variance=f"{row['variance']:.6f}")
    if history:
        logger.info("Pretraining on the %s state complete: %d iterations, fidelity %.4f -> %.4f",
                    pre.reference, len(history), history[0]["fidelity"], history[-1]["fidelity"])
    return state, key, history


__all__ = ["fidelity_partial", "combine_partials", "fidelity_residual", "gather_partials", "make_fidelity_residual",
           "make_reference", "pretrain", "REFERENCES"]
