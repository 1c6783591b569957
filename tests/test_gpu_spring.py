"""SPRING (optim.minsr.momentum; optimizers.minsr_direction with ``prev``) on the MI355X: the
step's linear algebra against a float64 parameter-space solve of the oracle's Jacobian, the
sharded path on one rank against the unsharded one, and the reference's integration run
(tests/test_gpu_train.py) with optimizer = "minsr" and momentum 0.9, with checkpoints.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd import train
from deephall_amd.networks import make_network
from deephall_amd.networks.psiformer import ParamTree, ref_offsets
from deephall_amd.optimizers import minsr_direction, minsr_direction_sharded
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_ntk import GATE_X, case
from test_gpu_parity import build
from test_gpu_train import logs, make_cfg, read_csv  # noqa: F401  (logs: fixture)

pytestmark = pytest.mark.gpu
MU = 0.9
_setup = {}


def setup(cuda):
    """test_gpu_minsr.py::test_direction_matches_parameter_space_solve's problem (MIX with one
    layer, B = 12, one NaN diff, lambda = mean diag), the float64 solves and a random float32
    ``prev`` of MinSR's own norm; computed once."""
    if _setup:
        return _setup
    ocfg = oracle_config("MIX", num_layers=1)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    B = 12
    x = make_walkers(B, ocfg.nelec, seed=5)
    diff = np.random.default_rng(23).standard_normal((B, 2)).astype(np.float32)
    diff[7] = np.nan
    keys = sorted(p64)
    xt = torch.tensor(x, dtype=torch.float64)

    def rows(c):
        out = []
        for b in range(B):
            g = R.logpsi_param_grad(p64, ocfg, xt[b:b + 1], np.array([c], dtype=np.float64))
            out.append(torch.cat([g[k].reshape(-1) for k in keys]))
        return torch.stack(out)

    v = torch.ones(B, dtype=torch.float64)
    v[7] = 0
    n = v.sum()
    Cm = torch.diag(v) - torch.outer(v, v) / n
    Ot = torch.cat([Cm @ rows((1.0, 0.0)), Cm @ rows((0.0, 1.0))]) / n.sqrt()
    d64 = torch.nan_to_num(torch.tensor(diff, dtype=torch.float64))
    eps = torch.cat([d64[:, 0] * v, d64[:, 1] * v]) / n.sqrt()
    lam = float(torch.diagonal(Ot @ Ot.t()).mean())
    P = Ot.shape[1]
    S = Ot.t() @ Ot + lam * torch.eye(P, dtype=torch.float64)
    minsr64 = torch.linalg.solve(S, 2 * Ot.t() @ eps)
    prev = ParamTree.zeros(model.spec, cuda)
    g = torch.Generator().manual_seed(47)
    for k in keys:
        prev[k].copy_(torch.randn(prev[k].shape, generator=g))
    prev.flat.mul_(float(minsr64.norm()) / float(prev.flat.double().norm()))
    prev64 = torch.cat([prev[k].reshape(-1) for k in keys]).double().cpu()
    ref = torch.linalg.solve(S, 2 * Ot.t() @ eps + lam * MU * prev64)
    _setup.update(model=model, params=to_device_params(p64), keys=keys, x=torch.tensor(x, device=cuda),
                  diff=torch.tensor(diff, device=cuda), lam=lam, P=P, prev=prev, ref=ref, minsr64=minsr64)
    return _setup


def test_direction_matches_parameter_space_solve(cuda):
    """phi64 = (S + lambda I)^-1 (2 O~^T eps~ + lambda mu phi_prev) from the oracle's float64 rows,
    mu = 0.9, |phi_prev| = |delta_MinSR|, at the MinSR test's gate:

        |phi - phi64|_inf / |phi64|_inf <= 25 * 4 e0 + 3e-5

    Measured on the MI355X: 9.49e-07 (gate 6.79e-04); phi64 differs from MinSR's delta64 by 0.39
    of max |phi64|."""
    s = setup(cuda)
    phi = minsr_direction(s["model"], s["params"], s["x"], s["diff"], s["lam"], prev=s["prev"], momentum=MU)
    got = torch.cat([phi[k].reshape(-1) for k in s["keys"]]).double().cpu()
    ref = s["ref"]
    err = float((got - ref).abs().max() / ref.abs().max())
    moved = float((ref - s["minsr64"]).abs().max() / ref.abs().max())
    gate = 25 * GATE_X * case("MIX", cuda)["e0"] + 3e-5
    print(f"spring direction: err = {err:.3e}, gate = {gate:.3e}, lambda = {s['lam']:.3e}, P = {s['P']}; "
          f"|phi64 - delta64_MinSR| / |phi64| = {moved:.3e}")
    assert moved > 0.05  # the momentum term is no rounding matter here
    assert err <= gate


def test_sharded_on_one_rank_is_identical(cuda):
    s = setup(cuda)
    a = minsr_direction(s["model"], s["params"], s["x"], s["diff"], s["lam"], prev=s["prev"], momentum=MU)
    keep = {}
    b = minsr_direction_sharded(s["model"], s["params"], s["x"], s["diff"], s["lam"], keep=keep, prev=s["prev"],
                                momentum=MU)
    assert torch.isfinite(a.flat).all() and float(a.flat.abs().max()) > 0
    assert torch.equal(a.flat, b.flat)
    assert set(keep) == {"T", "A", "y", "jv"} and keep["jv"].shape == (24,)


def spring_cfg(tmp_path, iterations):
    cfg = make_cfg(tmp_path, iterations, optimizer="minsr")
    cfg.optim.minsr.momentum = MU
    return cfg


def test_training(cuda, tmp_path, logs):  # noqa: F811
    """100 SPRING iterations (mu = 0.9) of the reference's integration problem (E = N / 2 = 1.5
    exactly): the energy of the last 30 iterations within the Adam and MinSR tests' 0.05, the
    variance falling, the previous direction in the checkpoint.  Measured on the MI355X:
    E = 1.5000, variance 9.90 (first 5) -> below the log's 1e-4 resolution (last 30)."""
    cfg = spring_cfg(tmp_path, 100)
    nref = ref_offsets(make_network(cfg.system, cfg.network).spec)[-1]
    train(cfg)
    rows = read_csv(tmp_path / "train_stats.csv")
    assert len(rows) == 100
    e = np.array([float(r["energy"]) for r in rows])
    var = np.array([float(r["variance"]) for r in rows])
    print(f"spring training: E(last 30) = {np.mean(e[-30:]):.4f}, variance first 5 = {np.mean(var[:5]):.4e}, "
          f"last 30 = {np.mean(var[-30:]):.4e}")
    assert abs(np.mean(e[-30:]) - 1.5) < 0.05, e[-30:]
    assert np.mean(var[-30:]) < np.mean(var[:5])
    with np.load(tmp_path / "ckpt_000099.npz", allow_pickle=False) as f:
        assert "opt_state/step" in f.files and int(f["opt_state/step"]) >= 99
        prev = f["opt_state/prev"]
        assert prev.shape == (nref,) and np.all(np.isfinite(prev)) and np.abs(prev).max() > 0


def test_checkpoint(cuda, tmp_path, logs):  # noqa: F811
    train(spring_cfg(tmp_path, 1))
    assert (tmp_path / "ckpt_000000.npz").exists()
    logs.clear()
    train(spring_cfg(tmp_path, 2))
    assert any("Restored checkpoint" in m for m in logs)
    with np.load(tmp_path / "ckpt_000001.npz", allow_pickle=False) as f:
        assert int(f["opt_state/step"]) >= 1
        prev = f["opt_state/prev"]
        assert np.all(np.isfinite(prev)) and np.abs(prev).max() > 0
