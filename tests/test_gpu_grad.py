"""GPU parity of the parameter gradient and the Adam step (§8f-2).

The HIP reverse mode (dh_logpsi_vjp, through the C ABI) against torch autograd of the
float64 restatement (oracle.reference.logpsi_param_grad = the reference's
jax.grad of network(params, x).real / .imag contracted with loss_prod's weights,
loss.py:53-64).  Tolerance: per parameter tensor, max |g - g_ref| <= 3e-5 * max |g_ref|
(f32 forward + backward; the weights ct are O(1), the walkers O(10)).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd import config
from deephall_amd.loss import LossMode, make_loss_fn
from deephall_amd.networks.psiformer import ParamTree, flat_params
from deephall_amd.optimizers import AdamState, adam_update, lr_schedule
from helpers import (FLOOR_X_MAX, GRAD_CASES, grad_case_inputs, grad_f32_errors, grad_tensor_errors, make_params,
                     make_walkers, oracle_config, to_device_params)
from oracle import reference as R
from test_gpu_parity import build, phase_err

pytestmark = pytest.mark.gpu
TOL_G = 3e-5
GRAD_CHUNK = 512  # kGradChunk (csrc/dh_internal.h): rows one partial sum of the reverse pass covers


def grad_errors(g_dev, g_ref, floor=1e-3):
    """max |g - g_ref| / max(max |g_ref|, floor * G) per tensor, G = the largest gradient
    entry of the whole tree: tensors whose exact gradient vanishes (the key biases: softmax
    is invariant to a per-row shift) are compared at the f32 noise level of the tree."""
    errs = grad_tensor_errors(g_dev, g_ref, floor)
    print({k.split("/", 1)[-1]: f"{v:.1e}" for k, v in errs.items()})
    return errs


@pytest.mark.parametrize("name,B,orbital", [("C1", 8, "full"), ("C2", 6, "full"), ("MIX", 8, "full"),
                                            ("C1", 6, "sparse"), ("MIX", 6, "sparse")])
def test_vjp_matches_autograd(cuda, name, B, orbital):
    ocfg = oracle_config(name, orbital=orbital)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    x = make_walkers(B, ocfg.nelec, seed=21)
    ct = np.random.default_rng(5).standard_normal((B, 2)).astype(np.float32)
    xd = torch.tensor(x, device=cuda)
    lp = torch.empty(B, 2, device=cuda)
    g = model.vjp(params, xd, torch.tensor(ct, device=cuda), logpsi=lp)
    ref = R.logpsi_param_grad(p64, ocfg, torch.tensor(x, dtype=torch.float64), ct.astype(np.float64))
    errs = grad_errors(g, ref)
    worst = max(errs, key=errs.get)
    assert errs[worst] < TOL_G, (worst, errs[worst])
    # the VJP's own forward pass returns log psi too
    lp_ref = R.batch_logpsi(p64, ocfg, torch.tensor(x, dtype=torch.float64))
    assert np.max(np.abs(lp[:, 0].cpu().numpy() - lp_ref.real.numpy()) / np.maximum(1, np.abs(lp_ref.real.numpy()))) < 2e-5


@pytest.mark.parametrize("name,B,orbital,seed", GRAD_CASES[1:])
def test_vjp_matches_autograd_edges(cuda, name, B, orbital, seed):
    """The reverse pass at the sizes the project trains at and at its untested edges: N = 10 and 20,
    unequal spin blocks, two determinants at N = 10, three layers, D = 384, D = 16 with unequal
    blocks, and batches of more than 512 rows (two partial sums per weight gradient).  The oracle's
    own float32 run is outside TOL_G on most of these (test_grad_floor_host.py), so each tensor is
    held to max(TOL_G, FLOOR_X_MAX * e32[k]), e32 = that run's error on the same inputs.
    Measured on the MI355X (e32 from the float32 torch run on that machine's CPU; it differs
    from one CPU to another): the largest err, and the largest err / e32 among the tensors above TOL_G
        C4    B = 4   1.85e-05  (none above TOL_G)      C4L3       B = 4   1.18e-05  (none)
        C5    B = 3   8.07e-05  3.18                    W384       B = 6   1.51e-05  (none)
        C4U   B = 4   1.67e-05  (none)                  MIX32      B = 8   2.16e-05  (none)
        C4K2  B = 4   4.81e-05  1.29                    MIX32 sp.  B = 8   1.85e-05  (none)
        C5    B = 27  3.36e-05  1.22    C4  B = 53  5.94e-05  0.88    C2  B = 90  2.68e-05  (none)
    C5, B = 3 at 3.18: a layer-2 key bias, whose exact gradient vanishes and which is therefore
    judged at 1e-3 of the tree's largest entry; its err is the sum of N^2 = 400 cancelling softmax
    terms per head in f32, as in the float32 run (7.0e-05 there on another CPU).
    C2, B = 90 has walkers of its own (helpers.GRAD_CASES): with seed 21 one walker's orbital
    matrix has condition number 1.9e+03, Re log psi from this pass is off by 3.69e-05 there (bound
    2e-05 below; every other walker within 1.8e-05, median 4.3e-07), and the oracle's float32 run
    on that walker errs by 3.8e-05 in the median and 1.2e-04 at most over 40 rounding histories."""
    ocfg = oracle_config(name, orbital=orbital)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    x, ct = grad_case_inputs(B, ocfg.nelec, seed)
    lp = torch.empty(B, 2, device=cuda)
    g = model.vjp(params, torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda), logpsi=lp)
    ref = R.logpsi_param_grad(p64, ocfg, torch.tensor(x, dtype=torch.float64), ct.astype(np.float64))
    errs = grad_errors(g, ref)
    e32 = grad_f32_errors(p64, ocfg, x, ct, ref=ref)
    over = {k: errs[k] / max(TOL_G, FLOOR_X_MAX * e32[k]) for k in errs}
    worst = max(over, key=over.get)
    ratio = max((errs[k] / e32[k] for k in errs if errs[k] > TOL_G), default=0.0)
    print(f"vjp {name} {orbital} B = {B} ({B * ocfg.nelec} rows): largest err {max(errs.values()):.2e}, largest err / e32 "
          f"above TOL_G {ratio:.2f}; nearest its gate ({over[worst]:.2f} of it): {worst}, err = {errs[worst]:.2e}, "
          f"e32 = {e32[worst]:.2e}, err / e32 = {errs[worst] / e32[worst]:.2f}")
    assert all(np.isfinite(v) for v in errs.values())
    assert over[worst] <= 1.0, (worst, errs[worst], e32[worst], errs[worst] / e32[worst])
    lp_ref = R.batch_logpsi(p64, ocfg, torch.tensor(x, dtype=torch.float64))
    lpn = lp.cpu().numpy()
    lp_err = np.abs(lpn[:, 0] - lp_ref.real.numpy()) / np.maximum(1, np.abs(lp_ref.real.numpy()))
    assert lp_err.max() < 2e-5, (int(lp_err.argmax()), lp_err.max())
    if name in ("W384", "C4L3"):  # no forward test elsewhere
        assert phase_err(lpn[:, 1], lp_ref.imag.numpy()) < 1e-4


@pytest.mark.parametrize("name,B", [("C5", 27), ("C2", 90)])
def test_row_chunks_sum_like_one(cuda, name, B):
    """More than kGradChunk = 512 rows in one launch: the weight gradients are reduced from two
    partial sums (at C5 the boundary falls inside walker 25 and the second partial has 28 rows).
    The gradient equals the sum of the two half batches' gradients, each within one partial, to
    the bound test_vjp_chunking_and_linearity holds sums taken in another order to."""
    ocfg = oracle_config(name)
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    rows, h = B * ocfg.nelec, (B + 1) // 2
    assert rows > GRAD_CHUNK and h * ocfg.nelec <= GRAD_CHUNK
    x, ct = grad_case_inputs(B, ocfg.nelec)
    x, ct = torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda)
    g = model.vjp(params, x, ct).flat.clone()
    ga = model.vjp(params, x[:h], ct[:h]).flat.clone()
    gb = model.vjp(params, x[h:], ct[h:]).flat.clone()
    scale = g.abs().max().item()
    err = (g - (ga + gb)).abs().max().item()
    print(f"row chunks {name}: {rows} rows, err / max|g| = {err / scale:.2e}")
    assert torch.isfinite(g).all() and scale > 0
    assert err <= 2e-6 * scale, err / scale


def test_vjp_chunking_and_linearity(cuda):
    """Walker chunks accumulate into the same gradient; the VJP is linear in ct."""
    from deephall_amd.networks import psiformer as pf

    ocfg = oracle_config("C2")
    system, model = build(ocfg)
    params = model.init(3, device=cuda)
    B = 40
    x = torch.tensor(make_walkers(B, ocfg.nelec, seed=8), device=cuda)
    ct = torch.tensor(np.random.default_rng(1).standard_normal((B, 2)), dtype=torch.float32, device=cuda)
    g1 = model.vjp(params, x, ct).flat.clone()
    g2 = model.vjp(params, x, 2 * ct).flat.clone()
    h = model.prepare(params, x.device)
    old = pf.VJP_WORKSPACE_BYTES
    try:
        pf.VJP_WORKSPACE_BYTES = h.lib.dh_vjp_workspace_bytes(h.h, 7)  # chunks of <= 7 walkers
        g3 = model.vjp(params, x, ct).flat.clone()
    finally:
        pf.VJP_WORKSPACE_BYTES = old
    scale = g1.abs().max().item()
    assert (g2 - 2 * g1).abs().max().item() <= 1e-6 * scale
    assert (g3 - g1).abs().max().item() <= 2e-6 * scale
    # zero cotangents give an exactly zero gradient
    g0 = model.vjp(params, x, torch.zeros_like(ct)).flat
    assert g0.abs().max().item() == 0.0


def test_param_tree_upload_paths_agree(cuda):
    """A ParamTree (flat buffer, uploaded as is) and a dict of separate tensors give
    bit-identical log psi; the library's on-device packing (folds Wo Wl, W0 Wqkv) is
    what both go through."""
    ocfg = oracle_config("C2")
    system, model = build(ocfg)
    tree = model.init(11, device=cuda)
    assert isinstance(tree, ParamTree) and tree.is_packed_view(model.spec)
    loose = {k: v.clone() for k, v in tree.items()}
    x = torch.tensor(make_walkers(16, ocfg.nelec, seed=2), device=cuda)
    a = model.apply(tree, x)
    b = model.apply(loose, x)
    assert torch.equal(a, b)
    assert torch.equal(flat_params(model.spec, loose, cuda), tree.flat)
    # in-place update through a view is seen (shared version counter)
    tree["PsiformerLayers_0/Dense_1/kernel"].mul_(0.5)
    c = model.apply(tree, x)
    assert not torch.equal(a, c)


def test_energy_grad_loss_matches_oracle(cuda):
    """make_loss_fn(ENERGY_GRAD) end to end: E_L -> stats -> clipped diff -> weights ->
    reverse mode, against the oracle's loss.py:66-106 on the same walkers."""
    ocfg = oracle_config("C1")
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    B = 12
    x = make_walkers(B, ocfg.nelec, seed=4)
    loss = make_loss_fn(model, system, LossMode.ENERGY_GRAD)
    stats, grad = loss(params, torch.tensor(x, device=cuda))
    xt = torch.tensor(x, dtype=torch.float64)
    el, obs = R.local_energy(p64, ocfg, xt)
    el = el.detach().numpy()
    o = {k: v.detach().numpy() for k, v in obs.items()}
    st = R.loss_stats(el, o, penalties=True)
    diff = R.loss_diff(el, o, st)
    n = np.sum(~np.isnan(diff))
    ct = np.stack([2 * diff.real / n, 2 * diff.imag / n], -1)
    ref = R.logpsi_param_grad(p64, ocfg, xt, ct)
    errs = grad_errors(grad, ref)
    worst = max(errs, key=errs.get)
    # the diff weights carry the E_L error (f32 Hessian-level), hence the looser bound
    assert errs[worst] < 2e-4, (worst, errs[worst])
    assert float(stats["energy"].real) == pytest.approx(float(np.mean(el.real)), rel=1e-5)


def test_adam_matches_optax_semantics(cuda):
    ocfg = oracle_config("C1")
    system, model = build(ocfg)
    params = model.init(1, device=cuda)
    p0 = {k: v.detach().double().cpu().clone() for k, v in params.items()}
    st = AdamState(params)
    lr = config.LearningRate(rate=0.05, decay=1.0, delay=3.0)
    rng = np.random.default_rng(0)
    seq = []
    for t in range(4):
        g = ParamTree.zeros(model.spec, cuda)
        g.flat.copy_(torch.tensor(rng.standard_normal(g.flat.numel()), dtype=torch.float32))
        if t == 2:
            g.flat[5] = float("nan")  # nan_to_num (loss.py:64)
        seq.append({k: v.detach().double().cpu() for k, v in g.items()})
        adam_update(params, g, st, lr_schedule(lr, st.count))
    ref = R.adam_reference(p0, seq, lambda t: lr_schedule(lr, t))
    for k in ref:
        got = params[k].detach().double().cpu()
        assert torch.allclose(got, ref[k], rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("name,pair", [("C1", (1, 0)), ("C4U", (7, 6))], ids=["C1", "C4U"])
def test_singular_walker_does_not_poison_gradient(cuda, name, pair):
    """a walker with two coincident electrons has psi = 0 (two equal orbital
    rows), a NaN E_L and therefore a zero cotangent (nanmean / nan_to_num drop it,
    loss.py:59-64).  The reverse pass must skip it — its inverse is inf and 0 * inf would
    put NaN into every weight gradient — so the gradient equals the one without it.
    At C4U (6 up, 4 down) the pair lies inside the second spin block."""
    ocfg = oracle_config(name)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    x = make_walkers(6, ocfg.nelec, seed=8)
    x[2, pair[0]] = x[2, pair[1]]  # coincident electrons
    ct = np.random.default_rng(9).standard_normal((6, 2)).astype(np.float32)
    ct[2] = 0.0
    lp = torch.empty(6, 2, device=cuda)
    g_all = model.vjp(params, torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda), logpsi=lp)
    assert not np.isfinite(lp[2, 0].item())  # psi = 0 for the coincident walker
    keep = [0, 1, 3, 4, 5]
    g_ref = model.vjp(params, torch.tensor(x[keep], device=cuda), torch.tensor(ct[keep], device=cuda))
    assert torch.isfinite(g_all.flat).all()
    scale = g_ref.flat.abs().max().item()
    assert (g_all.flat - g_ref.flat).abs().max().item() <= 1e-6 * scale
    # through the loss: E_L of that walker is NaN, the gradient stays finite
    _, grad = make_loss_fn(model, system, LossMode.ENERGY_GRAD)(params, torch.tensor(x, device=cuda))
    assert torch.isfinite(grad.flat).all()
