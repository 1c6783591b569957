"""dh_ntk_jvp, the per-walker Jacobian-vector product jv[b] = <g_b, v> (include/deephall_amd.h,
csrc/ntk.hip "The Jacobian-vector product"), on the MI355X against the float64 oracle's
explicit Jacobian.

Batch: B = dh_ntk_tile_walkers + 3 walkers: one full walker tile and a partial one.  Metric:
e = max_b |jv_b - J64_b . v| / (|J64_b| |v|); e0 is the same for the float32 rows dh_logpsi_vjp
gives with one-hot cotangents, dotted with v in float64; the gate is test_gpu_ntk's allowance for
an f32 kernel against the VJP's own rows, e <= GATE_X e0.

Measured values: test_matches_float64_oracle's docstring.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd.networks.psiformer import ParamTree
from helpers import make_params, make_walkers, oracle_config, to_device_params
from test_gpu_ntk import GATE_X, NAMES, jacobian32, jacobian64
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
_cases = {}


def case(name, cuda):
    """Everything the tests of one config share, computed once and left unchanged."""
    if name in _cases:
        return _cases[name]
    ocfg = oracle_config(name)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    keys = sorted(p64)
    tw = model.ntk_tile_walkers(cuda)
    B = tw + 3
    x = make_walkers(B, ocfg.nelec, seed=37)
    ct = np.random.default_rng(19).standard_normal((B, 2)).astype(np.float32)
    xd, ctd = torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda)
    # a random normal direction written into a zero tree: the layout's padding stays 0
    v = ParamTree.zeros(model.spec, cuda)
    g = torch.Generator().manual_seed(41)
    for k in keys:
        v[k].copy_(torch.randn(v[k].shape, generator=g))
    v64 = torch.cat([v[k].reshape(-1) for k in keys]).double().cpu()
    jv = model.jvp(params, xd, ctd, v)
    c = dict(ocfg=ocfg, p64=p64, model=model, params=params, keys=keys, tw=tw, B=B, x=x, ct=ct, xd=xd, ctd=ctd, v=v,
             v64=v64, jv=jv)
    _cases[name] = c
    return c


@pytest.mark.parametrize("name", NAMES)
def test_matches_float64_oracle(cuda, name):
    """e <= 4 e0 per config.  Measured on the MI355X (the kernel contracts the batch-mean-centred
    rows):
        C1  (N = 3, D = 256, B = 45):  e = 8.887e-08, e0 = 8.836e-08  (e / e0 = 1.01)
        C2  (N = 6, D = 256, B = 24):  e = 2.550e-08, e0 = 2.864e-08  (0.89)
        MIX (N = 4, D = 16,  B = 35):  e = 4.445e-07, e0 = 4.493e-07  (0.99)
        C4  (N = 10, D = 256, B = 15): e = 3.091e-08, e0 = 2.951e-08  (1.05)
        C5  (N = 20, D = 256, B = 9):  e = 1.089e-08, e0 = 1.114e-08  (0.98)
        MIX32 (N = 3 + 2, D = 16, B = 28): e = 6.299e-08, e0 = 6.063e-08  (1.04)
    The worst walker is the f32 rows' worst in every config: the error is the forward and reverse
    passes', not the product's.  A build that contracts the raw rows instead (DH_NTK_JVP_RAW)
    shows no difference at these sizes."""
    c = case(name, cuda)
    J64 = jacobian64(c["p64"], c["ocfg"], c["x"], c["ct"])
    J32 = jacobian32(c["model"], c["params"], c["xd"], c["ctd"], c["keys"])
    v64 = c["v64"]
    ref = J64 @ v64
    scale = J64.norm(dim=1) * v64.norm()
    err = (c["jv"].double().cpu() - ref).abs() / scale
    err0 = (J32.double() @ v64 - ref).abs() / scale
    e, e0 = float(err.max()), float(err0.max())
    print(f"jvp {name}: B = {c['B']}, tile walkers = {c['tw']}, e = {e:.3e}, e0 = {e0:.3e}, e / e0 = {e / e0:.2f}; "
          f"worst walker {int(err.argmax())} (the f32 rows' {int(err0.argmax())}); medians {float(err.median()):.2e}, "
          f"{float(err0.median()):.2e}")
    assert torch.isfinite(c["jv"]).all() and float(ref.abs().max()) > 0
    assert e <= GATE_X * e0, (e, e0)


@pytest.mark.parametrize("name", NAMES)
def test_exactness(cuda, name):
    """Linear in v to the bit for a power of two, reproducible, the same jv with and without T
    and on every part, and T the bits of dh_ntk / dh_ntk_part."""
    c = case(name, cuda)
    model, params, xd, ctd, v, jv = c["model"], c["params"], c["xd"], c["ctd"], c["v"], c["jv"]
    assert torch.equal(model.jvp(params, xd, ctd, v), jv)
    assert torch.equal(model.jvp(params, xd, ctd, 2.0 * v.flat), 2.0 * jv)
    T, jv_T = model.ntk_jvp(params, xd, ctd, v)
    assert torch.equal(jv_T, jv)
    assert torch.equal(T, model.ntk(params, xd, ctd))
    for part in range(2):
        Tp, jv_p = model.ntk_jvp(params, xd, ctd, v, part=part, nparts=2, mirror=False)
        assert torch.equal(jv_p, jv), part
        assert torch.equal(Tp, model.ntk(params, xd, ctd, part=part, nparts=2, mirror=False)), part


@pytest.mark.parametrize("name", NAMES)
def test_zero_cotangents(cuda, name):
    """Zero cotangents on three walkers, one of them in the partial tile: exactly 0 there, every
    other entry bit-identical."""
    c = case(name, cuda)
    B, tw = c["B"], c["tw"]
    zero = [1, tw - 2, tw + 1]
    ct0 = c["ctd"].clone()
    ct0[zero] = 0
    jv0 = c["model"].jvp(c["params"], c["xd"], ct0, c["v"])
    keep = torch.ones(B, dtype=torch.bool, device=jv0.device)
    keep[zero] = False
    assert (jv0[zero] == 0).all()
    assert torch.equal(jv0[keep], c["jv"][keep]) and (c["jv"][zero] != 0).all()


def test_singular_walker(cuda):
    """A walker with two coincident electrons (psi = 0, log psi = -inf) and a nonzero cotangent:
    jv = 0 there, finite elsewhere (as its row of T, test_gpu_ntk.test_singular_walker)."""
    c = case("C1", cuda)
    x = make_walkers(6, c["ocfg"].nelec, seed=8)
    x[2, 1] = x[2, 0]
    ct = np.random.default_rng(9).standard_normal((6, 2)).astype(np.float32)
    lp = torch.empty(6, 2, device=cuda)
    jv = c["model"].jvp(c["params"], torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda), c["v"], logpsi=lp)
    assert not np.isfinite(lp[2, 0].item())
    assert torch.isfinite(jv).all()
    assert jv[2] == 0 and (jv[[0, 1, 3, 4, 5]] != 0).all()
