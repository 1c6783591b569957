"""dh_ntk, the per-walker gradient Gram matrix T[b][b'] = <g_b, g_b'> (include/deephall_amd.h,
csrc/ntk.hip), on the MI355X against the float64 oracle's explicit Jacobian.

Batch: B = 2 * dh_ntk_tile_walkers + 3 walkers, so every launch has two full tiles and a
partial one in each direction.  Metric: e = max |T - T64| / sqrt(T64_bb T64_b'b').  The gate
is relative to what the float32 forward / backward passes already carry: e0 is the same
metric for the Gram matrix of the float32 Jacobian rows that dh_logpsi_vjp gives with one-hot
cotangents (rows multiplied in float64), and dh_ntk must stay within 4 e0 — the factor allows
for the Gram kernel's f32 accumulation over rows^2 products where the VJP reduces its
partials in double.

Measured values: test_matches_float64_oracle's docstring.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
GATE_X = 4.0
NAMES = ["C1", "C2", "MIX", "C4", "C5", "MIX32"]
_cases = {}


def jacobian64(p64, ocfg, x, ct):
    """Row b: the oracle's gradient of ct[b] . (Re, Im) log psi_b, leaves flattened in sorted order."""
    keys = sorted(p64)
    rows = []
    for b in range(x.shape[0]):
        g = R.logpsi_param_grad(p64, ocfg, torch.tensor(x[b:b + 1], dtype=torch.float64), ct[b:b + 1].astype(np.float64))
        rows.append(torch.cat([g[k].reshape(-1) for k in keys]))
    return torch.stack(rows)


def jacobian32(model, params, xd, ctd, keys):
    """Row b from dh_logpsi_vjp with the cotangent of walker b alone (float32 rows)."""
    B = xd.shape[0]
    rows = []
    for b in range(B):
        one = torch.zeros_like(ctd)
        one[b] = ctd[b]
        g = model.vjp(params, xd, one)
        rows.append(torch.cat([g[k].reshape(-1) for k in keys]).cpu())
    return torch.stack(rows)


def gram64(J, step=1 << 16):
    """J J^T in float64, a block of columns at a time (J may be float32 and large)."""
    T = torch.zeros(J.shape[0], J.shape[0], dtype=torch.float64)
    for c0 in range(0, J.shape[1], step):
        blk = J[:, c0:c0 + step].double()
        T += blk @ blk.t()
    return T


def gram_err(T, T64):
    d = torch.sqrt(torch.diagonal(T64))
    return float(((T.double() - T64).abs() / torch.outer(d, d)).max())


def case(name, cuda, tiles=2):
    """Everything the tests of one config share, computed once: walkers, cotangents, T, the
    float64 Gram matrix and e0 (B = tiles * tile walkers + 3; the cases of tiles = 2 are the
    ones kept under their config's name)."""
    key = name if tiles == 2 else (name, tiles)
    if key in _cases:
        return _cases[key]
    ocfg = oracle_config(name)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    tw = model.ntk_tile_walkers(cuda)
    B = tiles * tw + 3
    x = make_walkers(B, ocfg.nelec, seed=31)
    ct = np.random.default_rng(17).standard_normal((B, 2)).astype(np.float32)
    xd, ctd = torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda)
    lp = torch.empty(B, 2, device=cuda)
    T = model.ntk(params, xd, ctd, logpsi=lp)
    T64 = gram64(jacobian64(p64, ocfg, x, ct))
    T32 = gram64(jacobian32(model, params, xd, ctd, sorted(p64)))
    e0 = gram_err(T32, T64)
    c = dict(T32=T32, ocfg=ocfg, p64=p64, model=model, params=params, tw=tw, B=B, x=x, ct=ct, xd=xd, ctd=ctd, lp=lp, T=T,
             T64=T64, e0=e0)
    _cases[key] = c
    return c


@pytest.mark.parametrize("name", NAMES)
def test_matches_float64_oracle(cuda, name):
    """e <= 4 e0 per config.  Measured on the MI355X:
        C1  (N = 3, D = 256, B = 87):  e = 3.002e-04, e0 = 8.049e-05  (e / e0 = 3.73)
        C2  (N = 6, D = 256, B = 45):  e = 1.609e-05, e0 = 1.613e-05  (1.00)
        MIX (N = 4, D = 16,  B = 67):  e = 6.501e-06, e0 = 6.486e-06  (1.00)
        C4  (N = 10, D = 256, B = 27): e = 3.735e-05, e0 = 3.758e-05  (0.99)
        C5  (N = 20, D = 256, B = 15): e = 6.081e-05, e0 = 6.045e-05  (1.01)
        MIX32 (N = 3 + 2, D = 16, B = 53): e = 2.924e-05, e0 = 2.943e-05  (0.99)
    C1's worst entry is the diagonal of one ill-conditioned walker (its phase differs by 2e-4
    between the library's two float32 forward passes); the medians are 3e-7 for both.  Without
    the centring of ntk.hip ("Precision") C1 measured e = 6.1e-04 (7.6 e0) and failed."""
    check_against_oracle(case(name, cuda), name)


def test_matches_float64_oracle_two_partials(cuda):
    """C5 with B = 4 * tile walkers + 3 = 27 walkers, 540 rows: more than the 512 rows of one
    partial sum, so the batch mean that every dense map's input rows are centred on (ntk.hip
    "Precision") is reduced from two partials.  Same gate.  Measured on the MI355X:
        C5  (N = 20, D = 256, B = 27): e = 4.815e-04, e0 = 2.505e-04  (e / e0 = 1.92)
    (The identity the centring rests on holds for any row m: a wrong mean would cost this case
    precision, which the gate measures, not exactness.)"""
    c = case("C5", cuda, tiles=4)
    assert c["B"] * c["ocfg"].nelec > 512
    check_against_oracle(c, "C5, 4 tiles")


def check_against_oracle(c, name):
    """e <= GATE_X e0 for one case; prints where the worst entries are."""
    e = gram_err(c["T"].cpu(), c["T64"])
    print(f"ntk {name}: B = {c['B']}, tile walkers = {c['tw']}, e = {e:.3e}, e0 = {c['e0']:.3e}, e / e0 = {e / c['e0']:.2f}")
    d = torch.sqrt(torch.diagonal(c["T64"]))
    rel = (c["T"].cpu().double() - c["T64"]).abs() / torch.outer(d, d)
    i, j = divmod(int(rel.argmax()), c["B"])
    rel0 = (c["T32"] - c["T64"]).abs() / torch.outer(d, d)
    i0, j0 = divmod(int(rel0.argmax()), c["B"])
    print(f"  worst pair ({i}, {j}); the f32 rows' worst pair ({i0}, {j0}); medians {rel.median():.2e}, {rel0.median():.2e}; "
          f"against the f32 rows' Gram matrix {gram_err(c['T'].cpu(), c['T32']):.3e}")
    assert torch.isfinite(c["T"]).all()
    assert e <= GATE_X * c["e0"], (e, c["e0"])


@pytest.mark.parametrize("name", NAMES)
def test_symmetric_and_reproducible(cuda, name):
    c = case(name, cuda)
    assert torch.equal(c["T"], c["T"].t())
    again = c["model"].ntk(c["params"], c["xd"], c["ctd"])
    assert torch.equal(again, c["T"])


@pytest.mark.parametrize("name", NAMES)
def test_scaling_and_zero_cotangents(cuda, name):
    c = case(name, cuda)
    T, B, tw = c["T"], c["B"], c["tw"]
    # a power of two on one walker's cotangent: its row and column scale exactly
    b = tw + 1
    ct2 = c["ctd"].clone()
    ct2[b] *= 2
    T2 = c["model"].ntk(c["params"], c["xd"], ct2)
    s = torch.ones(B, device=T.device)
    s[b] = 2
    assert torch.equal(T2, T * s[:, None] * s[None, :])
    # zero cotangents on three walkers (one in the partial tile): exactly zero rows and
    # columns, every other entry bit-identical
    zero = [1, tw + 2, 2 * tw + 1]
    ct0 = c["ctd"].clone()
    ct0[zero] = 0
    T0 = c["model"].ntk(c["params"], c["xd"], ct0)
    keep = torch.ones(B, dtype=torch.bool, device=T.device)
    keep[zero] = False
    assert (T0[zero] == 0).all() and (T0[:, zero] == 0).all()
    assert torch.equal(T0[keep][:, keep], T[keep][:, keep])


def test_singular_walker(cuda):
    """A walker with two coincident electrons (psi = 0, log psi = -inf) and a NONZERO cotangent:
    its row and column are zero, the rest is finite and is the Gram matrix of the batch
    without it (to the gate of the oracle test)."""
    c = case("C1", cuda)
    model, params = c["model"], c["params"]
    x = make_walkers(6, c["ocfg"].nelec, seed=8)
    x[2, 1] = x[2, 0]
    ct = np.random.default_rng(9).standard_normal((6, 2)).astype(np.float32)
    lp = torch.empty(6, 2, device=cuda)
    T = model.ntk(params, torch.tensor(x, device=cuda), torch.tensor(ct, device=cuda), logpsi=lp)
    assert not np.isfinite(lp[2, 0].item())
    assert torch.isfinite(T).all()
    assert (T[2] == 0).all() and (T[:, 2] == 0).all()
    keep = [0, 1, 3, 4, 5]
    Tk = model.ntk(params, torch.tensor(x[keep], device=cuda), torch.tensor(ct[keep], device=cuda))
    e = gram_err(T[keep][:, keep].cpu(), Tk.double().cpu())
    print(f"ntk singular walker: e = {e:.3e}, gate {GATE_X * c['e0']:.3e}")
    assert e <= GATE_X * c["e0"]


@pytest.mark.parametrize("name", NAMES)
def test_logpsi_output(cuda, name):
    """The forward pass's log psi against model.apply, at the bound and on the part (Re) that
    test_gpu_grad.py::test_vjp_matches_autograd holds dh_logpsi_vjp's same output to."""
    c = case(name, cuda)
    ref = c["model"].apply(c["params"], c["xd"])
    re = (c["lp"][:, 0] - ref.real).abs() / ref.real.abs().clamp(min=1)
    assert re.max().item() < 2e-5
