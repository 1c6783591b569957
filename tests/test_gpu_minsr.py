"""The MinSR optimizer (optimizers.py make_minsr_training_step) on the MI355X: the step's
linear algebra against a float64 parameter-space solve of the oracle's Jacobian, and the
reference's integration run (tests/test_gpu_train.py) with optimizer = "minsr".
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd import train
from deephall_amd.optimizers import minsr_direction
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_ntk import GATE_X, case
from test_gpu_parity import build
from test_gpu_train import logs, make_cfg, read_csv  # noqa: F401  (logs: fixture)

pytestmark = pytest.mark.gpu


def test_direction_matches_parameter_space_solve(cuda):
    """MIX with one layer (P about 5 k), B = 12, lambda = mean diag(T~): the condition number of
    T~ + lambda I is at most 2 B + 1 = 25, so the direction carries about 25 x the Gram error
    (gated at 4 e0 of MIX) plus the VJP's 3e-5:

        |delta - delta64|_inf / |delta64|_inf <= 25 * 4 e0 + 3e-5

    delta64 = (S + lambda I)^-1 2 O~^T eps~ with S = O~^T O~ from the oracle's float64 rows, centred
    over the walkers with a non-NaN diff.  Measured on the MI355X: 6.41e-07 (gate 6.79e-04)."""
    ocfg = oracle_config("MIX", num_layers=1)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    B = 12
    x = make_walkers(B, ocfg.nelec, seed=5)
    rng = np.random.default_rng(23)
    diff = rng.standard_normal((B, 2)).astype(np.float32)
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
    ref = torch.linalg.solve(Ot.t() @ Ot + lam * torch.eye(P, dtype=torch.float64), 2 * Ot.t() @ eps)

    params = to_device_params(p64)
    delta = minsr_direction(model, params, torch.tensor(x, device=cuda), torch.tensor(diff, device=cuda), lam)
    got = torch.cat([delta[k].reshape(-1) for k in keys]).double().cpu()
    err = float((got - ref).abs().max() / ref.abs().max())
    gate = 25 * GATE_X * case("MIX", cuda)["e0"] + 3e-5
    print(f"minsr direction: err = {err:.3e}, gate = {gate:.3e}, lambda = {lam:.3e}, P = {P}")
    assert err <= gate


def test_training(cuda, tmp_path, logs):  # noqa: F811
    """100 MinSR iterations of the reference's integration problem (filled lowest Landau level,
    E = N / 2 = 1.5 exactly): the energy of the last 30 iterations within the Adam test's 0.05,
    the variance falling, the step counter in the checkpoint.  Measured on the MI355X: E = 1.5004,
    variance 9.96 (first 5) -> below the log's 1e-4 resolution (last 30); Adam on the same seed
    ends at 2.1e-3, KFAC at 1.9e-2."""
    train(make_cfg(tmp_path, 100, optimizer="minsr"))
    rows = read_csv(tmp_path / "train_stats.csv")
    assert len(rows) == 100
    e = np.array([float(r["energy"]) for r in rows])
    var = np.array([float(r["variance"]) for r in rows])
    print(f"minsr training: E(last 30) = {np.mean(e[-30:]):.4f}, variance first 5 = {np.mean(var[:5]):.4e}, "
          f"last 30 = {np.mean(var[-30:]):.4e}")
    assert abs(np.mean(e[-30:]) - 1.5) < 0.05, e[-30:]
    assert np.mean(var[-30:]) < np.mean(var[:5])
    with np.load(tmp_path / "ckpt_000099.npz", allow_pickle=False) as f:
        assert "opt_state/step" in f.files and int(f["opt_state/step"]) >= 99


def test_checkpoint(cuda, tmp_path, logs):  # noqa: F811
    train(make_cfg(tmp_path, 1, optimizer="minsr"))
    assert (tmp_path / "ckpt_000000.npz").exists()
    logs.clear()
    train(make_cfg(tmp_path, 2, optimizer="minsr"))
    assert any("Restored checkpoint" in m for m in logs)
    with np.load(tmp_path / "ckpt_000001.npz", allow_pickle=False) as f:
        assert int(f["opt_state/step"]) >= 1
