"""Optimizer steps — mirror of deephall/optimizers/ (__init__.py:25-35, adam.py:24-43,
none.py:22-35).

``make_optimizer_step(cfg, network) -> (init, step)`` with
``step(state, key) -> (state, stats)`` over a ``CheckpointState``.  The gradient is
the loss of ``make_loss_fn(..., ENERGY_GRAD)`` (reverse mode in the HIP library,
averaged over ranks by the second all-reduce of the iteration — the reference's Adam
path omits that average, SURVEY.md finding 9); the Adam update is one HIP kernel over
the flat parameter buffer (``dh_adam_update``, optax.adam semantics).  KFAC
(optimizers/kfac.py:195-241 on kfac_jax, the reference's default) runs on the dh_kfac_*
kernels: the Fisher statistics come out of the gradient's forward pass and share its
all-reduce, the EMA / damped inverses / preconditioned, norm-constrained update run on the
device with no host sync (the algorithm is restated in oracle/kfac.py).
MinSR (not in the reference) takes the exact natural-gradient step in sample
space: the per-walker gradient Gram matrix comes from the dh_ntk kernels, the 2B x 2B solve
is float64 torch.linalg on the device, the update direction one more dh_logpsi_vjp.  Across
ranks (``optim.minsr.sharded``) every rank computes its share of the Gram matrix of the gathered
walkers (dh_ntk_part) and the solve matrix comes from one kernel (dh_minsr_matrix).
``optim.minsr.momentum`` turns the step into SPRING: the same solve with the previous direction's
per-walker Jacobian-vector products (dh_ntk_jvp, in the Gram matrix's reverse walk) on its
right-hand side.
"""

from __future__ import annotations

import logging

import torch
import torch.distributed as dist

from . import _lib, constants
from .config import Config, LearningRate, OptimizerName
from .loss import LossMode, grad_cotangent, make_loss_fn
from .networks.psiformer import ParamTree, _ptr, _stream
from .types import CheckpointState

logger = logging.getLogger(__name__)


def lr_schedule(lr: LearningRate, t: int) -> float:
    """rate * (1 / (1 + t / delay)) ** decay (config.py:125-137)."""
    return float(lr.rate * (1.0 / (1.0 + (t / lr.delay))) ** lr.decay)


class AdamState:
    """optax ScaleByAdamState (count, mu, nu) + the schedule's count, on the device."""

    def __init__(self, params: ParamTree):
        self.mu = torch.zeros_like(params.flat)
        self.nu = torch.zeros_like(params.flat)
        self.count = 0

    def state_dict(self):
        return {"mu": self.mu, "nu": self.nu, "count": self.count}

    def load_state_dict(self, d):
        self.mu.copy_(torch.as_tensor(d["mu"]))
        self.nu.copy_(torch.as_tensor(d["nu"]))
        self.count = int(d["count"])


def adam_update(params: ParamTree, grads: ParamTree, state: AdamState, lr: float, b1=0.9, b2=0.999, eps=1e-8):
    """One optax.adam step in place on ``params.flat`` (dh_adam_update)."""
    p = params.flat
    if not (p.is_cuda and grads.flat.shape == p.shape):
        raise ValueError("params and grads must be matching flat device buffers")
    _lib.check(
        _lib.load().dh_adam_update(_ptr(p), _ptr(grads.flat), _ptr(state.mu), _ptr(state.nu), p.numel(), float(lr),
                                   float(b1), float(b2), float(eps), int(state.count), _stream(p.device))
    )
    state.count += 1


def make_adam_training_step(cfg: Config, network, residual=None):
    loss_grad_fn = make_loss_fn(network, cfg.system, LossMode.ENERGY_GRAD, residual=residual)
    net = loss_grad_fn.network

    def init(params, key=None, data=None):
        del key, data
        return AdamState(params)

    def step(state: CheckpointState, key=None, **stat_kw):
        params, data, opt_state, width = state
        stats, grads = loss_grad_fn(params, data, **stat_kw)
        adam_update(params, grads, opt_state, lr_schedule(cfg.optim.adam.lr, opt_state.count))
        net.invalidate()  # the kernel wrote the flat buffer behind torch's version counter
        return CheckpointState(params, data, opt_state, width), stats

    return init, step


# kfac_jax.Optimizer settings of optimizers/kfac.py:203-218, 230-236
KFAC_CURVATURE_EMA = 0.95
KFAC_DAMPING = 1e-3
KFAC_NORM_CONSTRAINT = 1e-3


class KfacState:
    """The curvature EMA (raw factor sums and their weight) and the step counter of the
    kfac_jax optimizer state; P g and the step info live beside it on the device."""

    def __init__(self, network, params: ParamTree):
        dev = params.flat.device
        lay = network.kfac_layout(dev)
        self.raw = torch.zeros(lay["nstats"], dtype=torch.float32, device=dev)
        self.weight = 0.0
        self.step = 0
        self.pgrad = torch.zeros_like(params.flat)
        self.info = torch.zeros(4, dtype=torch.float64, device=dev)

    def state_dict(self):
        return {"raw": self.raw, "weight": self.weight, "step": self.step}

    def load_state_dict(self, d):
        self.raw.copy_(torch.as_tensor(d["raw"]))
        self.weight = float(d["weight"])
        self.step = int(d["step"])


def make_kfac_training_step(cfg: Config, network, residual=None):
    """optimizers/kfac.py:195-241: kfac_jax.Optimizer(l2_reg 0, norm_constraint 1e-3,
    curvature_ema 0.95, inverse_update_period 1, estimation_mode fisher_exact, multi_device)
    stepped with momentum 0 and damping 1e-3 at the schedule's learning rate."""
    loss_grad_fn = make_loss_fn(network, cfg.system, LossMode.ENERGY_GRAD, curvature=True, residual=residual)
    net = loss_grad_fn.network
    if str(getattr(cfg.network.orbital, "value", cfg.network.orbital)) == "sparse":
        # kfac.py:127-133, 175-181 (oracle/kfac.py header): the lll_weight block's statistics assume
        # kfac_jax's matcher tags the axis-1 DenseGeneral as repeated_dense_complex_no_bias
        logger.warning("KFAC with sparse orbitals: the lll_weight curvature block follows oracle/kfac.py's "
                       "restatement of kfac_jax, parity unpinned against the reference (kfac_jax is absent)")

    def init(params, key=None, data=None):
        del key, data
        return KfacState(net, params)

    def step(state: CheckpointState, key=None, **stat_kw):
        params, data, opt_state, width = state
        stats, grads = loss_grad_fn(params, data, **stat_kw)
        opt_state.weight = KFAC_CURVATURE_EMA * opt_state.weight + 1.0
        lr = lr_schedule(cfg.optim.kfac.lr, opt_state.step)
        net.kfac_step(opt_state.raw, loss_grad_fn.curvature, KFAC_CURVATURE_EMA, opt_state.weight, grads, params, lr,
                      KFAC_DAMPING, KFAC_NORM_CONSTRAINT, opt_state.pgrad, opt_state.info)
        opt_state.step += 1
        net.invalidate()  # the kernel wrote the flat buffer behind torch's version counter
        return CheckpointState(params, data, opt_state, width), stats

    return init, step


class MinsrState:
    """MinSR keeps no curvature or momentum between steps: the step counter (the learning-rate
    schedule's argument) is the whole state.  SPRING (``optim.minsr.momentum`` > 0) adds ``prev``,
    the previous step's unscaled direction phi, float32 [nref] on the device."""

    def __init__(self, prev: torch.Tensor | None = None):
        self.step = 0
        self.prev = prev

    def state_dict(self):
        if self.prev is None:
            return {"step": self.step}
        return {"step": self.step, "prev": self.prev}

    def load_state_dict(self, d):
        self.step = int(d["step"])
        if self.prev is not None:
            self.prev.copy_(torch.as_tensor(d["prev"]))


def _flat_direction(prev):
    return prev.flat if hasattr(prev, "flat") else prev


def minsr_direction(net, params: ParamTree, data: torch.Tensor, diff: torch.Tensor, damping: float,
                    prev=None, momentum: float = 0.0) -> ParamTree:
    """The linear-algebra half of a MinSR step for given clipped energy differences ``diff``
    [B, 2] float32 (re, im; NaN = walker dropped):

        delta = 2 O~^T (O~ O~^T + damping I)^-1 eps~  =  (O~^T O~ + damping I)^-1 2 O~^T eps~

    O~ [2B, P]: the rows d Re log psi_b / dp, then d Im log psi_b / dp, centred over the valid
    walkers v (non-NaN diff, finite log psi; n of them) and divided by sqrt(n); eps~ =
    [Re diff; Im diff] / sqrt(n), zero outside v.  O~ O~^T is the centred dh_ntk Gram matrix of
    [data; data] with cotangents (1, 0) | (0, 1); the solve runs in float64 on the device; the
    product with O~^T is dh_logpsi_vjp with the solution as cotangents.

    SPRING (``prev`` = the previous direction phi_prev, a ParamTree or a flat [nref] tensor, and
    ``momentum`` = mu != 0): the damping pulls towards mu phi_prev instead of towards 0,

        phi = mu phi_prev + 2 O~^T (O~ O~^T + damping I)^-1 (eps~ - (mu / 2) O~ phi_prev)
            = (O~^T O~ + damping I)^-1 (2 O~^T eps~ + damping mu phi_prev)

    with O~ phi_prev = C jv / sqrt(n), jv the per-walker Jacobian-vector products that come out of
    the Gram matrix's own reverse walk (``net.ntk_jvp``, dh_ntk_jvp), taken to float64; the matrix
    is then dh_minsr_matrix's on the device.  Without ``prev`` or with mu = 0 this is the MinSR
    path above, bit for bit."""
    B = data.shape[0]
    dev = data.device
    spring = prev is not None and momentum != 0
    ct = torch.zeros(2 * B, 2, dtype=torch.float32, device=dev)
    ct[:B, 0] = 1.0
    ct[B:, 1] = 1.0
    lp = torch.empty(2 * B, 2, dtype=torch.float32, device=dev)
    if spring:
        T, jv = net.ntk_jvp(params, torch.cat([data, data]), ct, _flat_direction(prev), logpsi=lp)
    else:
        T = net.ntk(params, torch.cat([data, data]), ct, logpsi=lp)
    diff = diff.to(device=dev, dtype=torch.float64)
    valid = ~torch.isnan(diff).any(dim=1) & torch.isfinite(lp[:B]).all(dim=1)
    v = valid.double()
    n = v.sum().clamp(min=1.0)

    def centre(a):  # C a over the last axis [.., B]: a - mean_v(a) on v, 0 outside
        a = a * v
        return a - v * (a.sum(-1, keepdim=True) / n)

    if spring and T.is_cuda:
        A = minsr_matrix(T, valid, damping)
    else:
        T = T.double()
        T4 = centre(T.view(2, B, 2, B))                              # columns
        T4 = centre(T4.permute(2, 3, 0, 1)).permute(2, 3, 0, 1)      # rows
        Tbar = T4.reshape(2 * B, 2 * B) / n
        A = Tbar + float(damping) * torch.eye(2 * B, dtype=torch.float64, device=dev)
    eps = (torch.nan_to_num(diff, nan=0.0) * v[:, None]).t().reshape(2 * B) / n.sqrt()
    if spring:
        eps = eps - (0.5 * float(momentum)) * centre(jv.double().view(2, B)).reshape(2 * B) / n.sqrt()
    L, info = torch.linalg.cholesky_ex(A)
    if int(info) == 0:
        y = torch.cholesky_solve(eps[:, None], L)[:, 0]
    else:
        y = torch.linalg.solve(A, eps)
    ct2 = (2.0 * centre(y.view(2, B)) / n.sqrt()).t().contiguous().float()
    delta = net.vjp(params, data, ct2)
    if spring:
        delta.flat.add_(_flat_direction(prev).to(delta.flat.dtype), alpha=float(momentum))
    return delta


def minsr_matrix(T: torch.Tensor, valid: torch.Tensor, damping: float) -> torch.Tensor:
    """dh_minsr_matrix: A = C T C / n + damping I, float64 [2B, 2B], from the symmetric float32
    Gram matrix ``T`` [2B, 2B] of the doubled batch and the walkers' ``valid`` flags [B] (bool);
    C centres each half over the valid walkers (n of them, at least 1) and zeroes the others.
    What ``minsr_direction`` assembles in torch, in one kernel: T read twice, A written once."""
    M = T.shape[0]
    B = M // 2
    if not (T.is_cuda and T.dtype == torch.float32 and tuple(T.shape) == (2 * B, 2 * B) and B >= 1):
        raise ValueError("T must be a float32 [2B, 2B] device matrix")
    if tuple(valid.shape) != (B,):
        raise ValueError(f"valid must be [{B}]")
    T = T.contiguous()
    v = valid.to(device=T.device, dtype=torch.bool).contiguous().view(torch.uint8)
    lib = _lib.load()
    A = torch.empty(M, M, dtype=torch.float64, device=T.device)
    ws = torch.empty(lib.dh_minsr_matrix_workspace_bytes(B) // 8, dtype=torch.float64, device=T.device)
    _lib.check(lib.dh_minsr_matrix(_ptr(T), _ptr(v), B, float(damping), _ptr(A), _ptr(ws), ws.numel() * 8,
                                   _stream(T.device)))
    return A


def minsr_direction_sharded(net, params: ParamTree, data: torch.Tensor, diff: torch.Tensor, damping: float,
                            keep: dict | None = None, prev=None, momentum: float = 0.0) -> ParamTree:
    """``minsr_direction`` over the walkers of every rank: ``data`` [B, N, 2] and
    ``diff`` [B, 2] are this rank's shard, the direction is that of the gathered batch of
    B_g = world size x B walkers, identical on every rank.

    No activations travel: the walkers and diffs are all-gathered (one small collective), every
    rank runs the forward / reverse pass over all 2 B_g walkers of the doubled batch and the Gram
    products of the rows it owns (dh_ntk_part), one all-reduce SUM puts T together — exact, every
    entry has one owner — and dh_ntk_mirror, dh_minsr_matrix and the float64 solve run redundantly
    on every rank.  The centred solution's slice for this rank's walkers goes through
    dh_logpsi_vjp; the all-reduce SUM of the results is the direction.  World size 1: the same
    kernels, no collectives.  Shards must be equal (``ValueError``).
    ``keep``: a dict that receives T, A and the solution y (tests).
    ``prev``, ``momentum``: SPRING, as in ``minsr_direction``.  jv over all 2 B_g walkers comes out
    of the same dh_ntk_jvp(part = rank, nparts = R) call complete and identical on every rank, and
    phi_prev is identical on every rank because the direction is: no further collective.  ``keep``
    then receives jv as well."""
    spring = prev is not None and momentum != 0
    R, rank = constants.world_size(), constants.rank()
    B = data.shape[0]
    dev = data.device
    diff = diff.to(device=dev, dtype=torch.float32)
    if R > 1:
        sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(R)]
        dist.all_gather(sizes, torch.tensor([B], dtype=torch.int64, device=dev))
        sizes = [int(s) for s in sizes]
        if sizes != [B] * R:
            raise ValueError(f"sharded MinSR needs equal walker shards on every rank, got {sizes}")
        mine = torch.cat([data.reshape(B, -1).float(), diff], dim=1).contiguous()
        parts = [torch.empty_like(mine) for _ in range(R)]
        dist.all_gather(parts, mine)
        allx = torch.cat(parts)
        data_g = allx[:, :-2].reshape(R * B, *data.shape[1:]).contiguous()
        diff_g = allx[:, -2:]
    else:
        data_g, diff_g = data, diff
    Bg = R * B
    ct = torch.zeros(2 * Bg, 2, dtype=torch.float32, device=dev)
    ct[:Bg, 0] = 1.0
    ct[Bg:, 1] = 1.0
    lp = torch.empty(2 * Bg, 2, dtype=torch.float32, device=dev)
    if spring:
        T, jv = net.ntk_jvp(params, torch.cat([data_g, data_g]), ct, _flat_direction(prev), logpsi=lp, part=rank,
                            nparts=R, mirror=False)
    else:
        T = net.ntk(params, torch.cat([data_g, data_g]), ct, logpsi=lp, part=rank, nparts=R, mirror=False)
    if R > 1:
        dist.all_reduce(T)
    net.ntk_mirror(T)
    diff_g = diff_g.double()
    valid = ~torch.isnan(diff_g).any(dim=1) & torch.isfinite(lp[:Bg]).all(dim=1)
    A = minsr_matrix(T, valid, damping)
    if keep is not None:
        keep["T"], keep["A"] = T, A.clone()
    del T
    v = valid.double()
    n = v.sum().clamp(min=1.0)
    eps = (torch.nan_to_num(diff_g, nan=0.0) * v[:, None]).t().reshape(2 * Bg) / n.sqrt()
    if spring:
        j2 = jv.double().view(2, Bg) * v
        j2 = j2 - v * (j2.sum(-1, keepdim=True) / n)
        eps = eps - (0.5 * float(momentum)) * j2.reshape(2 * Bg) / n.sqrt()
        if keep is not None:
            keep["jv"] = jv
    L, info = torch.linalg.cholesky_ex(A)
    if int(info) == 0:
        y = torch.cholesky_solve(eps[:, None], L)[:, 0]
    else:
        y = torch.linalg.solve(A, eps)
    del L, A
    if keep is not None:
        keep["y"] = y
    y2 = y.view(2, Bg) * v
    y2 = y2 - v * (y2.sum(-1, keepdim=True) / n)
    ct2 = (2.0 * y2 / n.sqrt()).t()[rank * B:(rank + 1) * B].contiguous().float()
    delta = net.vjp(params, data, ct2)
    if R > 1:
        dist.all_reduce(delta.flat)  # a sum: every row carries the global 1 / sqrt(n)
    if spring:
        delta.flat.add_(_flat_direction(prev).to(delta.flat.dtype), alpha=float(momentum))
    return delta


def make_minsr_training_step(cfg: Config, network, residual=None):
    """MinSR (Chen & Heyl 2024; Rende et al. 2024): stochastic reconfiguration solved in sample
    space, delta = (S + damping I)^-1 g with S the centred 2B-sample Fisher matrix — exact, where
    KFAC approximates — then KFAC's norm constraint against the ENERGY_GRAD gradient g:
    c = min(1, sqrt(norm_constraint / (lr^2 <delta, g>))), params -= lr c delta.
    ``optim.minsr.sharded``: the direction over the walkers of every rank
    (minsr_direction_sharded) and g averaged over ranks as the Adam step's.
    ``optim.minsr.momentum`` = mu > 0: SPRING (Goldshlager, Abrahamsen, Lin 2024), delta = phi of
    ``minsr_direction`` with the previous step's phi — unscaled by lr and c, non-finite entries
    zeroed — kept in the state; the first step's phi_prev is 0."""
    mu = float(cfg.optim.minsr.momentum)
    if not 0.0 <= mu < 1.0:
        raise ValueError(f"optim.minsr.momentum must be in [0, 1), got {mu}")
    sharded = bool(cfg.optim.minsr.sharded)
    if constants.world_size() > 1 and not sharded:
        raise NotImplementedError("MinSR on more than one rank needs each rank to compute a share of the gathered "
                                  "walkers' Gram matrix: set optim.minsr.sharded (every rank then holds the whole "
                                  "batch's activations and matrices), or run it on a single rank")
    loss_fn = make_loss_fn(network, cfg.system, LossMode.ENERGY_DIFF, residual=residual)
    net = loss_fn.network
    if net is None or not hasattr(net, "ntk"):
        raise TypeError("MinSR needs a Psiformer of this library")
    opt = cfg.optim.minsr

    def init(params, key=None, data=None):
        del key, data
        return MinsrState(torch.zeros_like(params.flat) if mu > 0 else None)

    def step(state: CheckpointState, key=None, **stat_kw):
        params, data, opt_state, width = state
        stats, diff = loss_fn(params, data, **stat_kw)
        diff = torch.view_as_real(diff).contiguous()
        nvalid = (~torch.isnan(diff).any(dim=1)).sum().float().view(1)
        grad = net.vjp(params, data, grad_cotangent(diff, nvalid, 0))
        if sharded:
            constants.pmean_(grad.flat)
            delta = minsr_direction_sharded(net, params, data, diff, opt.damping, prev=opt_state.prev, momentum=mu)
        else:
            delta = minsr_direction(net, params, data, diff, opt.damping, prev=opt_state.prev, momentum=mu)
        step.last_diff, step.last_direction = diff, delta  # what the direction was solved from (tests)
        lr = lr_schedule(opt.lr, opt_state.step)
        d = torch.nan_to_num(delta.flat, nan=0.0, posinf=0.0, neginf=0.0)
        if opt_state.prev is not None:
            opt_state.prev.copy_(d)
        sq = (lr * lr) * torch.dot(d.double(), torch.nan_to_num(grad.flat).double())
        c = torch.where(sq > opt.norm_constraint, torch.sqrt(opt.norm_constraint / sq.clamp(min=1e-300)),
                        torch.ones_like(sq))
        params.flat.sub_((lr * c).float() * d)
        opt_state.step += 1
        net.invalidate()
        return CheckpointState(params, data, opt_state, width), stats

    return init, step


def make_inference_step(cfg: Config, network):
    loss_fn = make_loss_fn(network, cfg.system, LossMode.ENERGY_DIFF)

    def init(params, key=None, data=None):
        return None

    def step(state: CheckpointState, key=None, **stat_kw):
        stats, _ = loss_fn(state.params, state.data, **stat_kw)
        return state, stats

    return init, step


def make_optimizer_step(cfg: Config, network, residual=None):
    """optimizers/__init__.py:25-35.  ``residual`` (pretrain.make_fidelity_residual): the hook of
    ``make_loss_fn`` that puts a per-walker residual in the local energy's place; every training
    step takes it, the inference step has nothing to train (``ValueError``)."""
    name = cfg.optim.optimizer
    name = OptimizerName(getattr(name, "value", name)) if name is not None else OptimizerName.none
    if name == OptimizerName.adam:
        return make_adam_training_step(cfg, network, residual=residual)
    if name == OptimizerName.none:
        if residual is not None:
            raise ValueError("a residual hook needs an optimizer (adam, kfac or minsr), not 'none'")
        return make_inference_step(cfg, network)
    if name == OptimizerName.kfac:
        return make_kfac_training_step(cfg, network, residual=residual)
    if name == OptimizerName.minsr:
        return make_minsr_training_step(cfg, network, residual=residual)
    raise ValueError(f"Optimizer {name} is not implemented!")
