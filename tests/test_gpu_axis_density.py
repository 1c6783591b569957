"""The histogram about an axis on the GPU (csrc/impurity.hip, dh_axis_histogram) against the numpy
restatement tests/impurity_ref.py, exactly, and the axis_density estimator through netobs.evaluate on
a pinned-quasihole state."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import impurity_ref as IR
from deephall_amd.config import Config
from deephall_amd.netobs import ESTIMATORS, DeepHallAdaptor, evaluate
from deephall_amd.netobs._native import axis_histogram
from deephall_amd.train import train

pytestmark = pytest.mark.gpu

# (nspins, B, axis, bins, seed): N = 2, 6, 6, 20; one block and several; 1, odd, 4096 bins; both poles
CASES = [((1, 1), 1, (1.1, 2.8), 1, 1), ((1, 1), 129, (0.0, 0.0), 7, 2), ((3, 3), 127, (2.3, -1.9), 50, 3),
         ((3, 3), 600, (math.pi, 0.0), 16, 4), ((6, 0), 128, (0.4, 0.3), 4096, 5), ((10, 10), 600, (1.7, 5.1), 50, 6),
         ((0, 6), 600, (1.3, 1.0), 33, 7), ((10, 10), 4100, (2.9, -0.2), 64, 8)]


@pytest.mark.parametrize("nspins,B,axis,bins,seed", CASES, ids=[f"{c[0]}-B{c[1]}-bins{c[3]}" for c in CASES])
def test_counts_against_the_restatement(cuda, nspins, B, axis, bins, seed):
    xn = IR.walkers(B, sum(nspins), seed)
    want, flagged = IR.histogram(xn, nspins, axis, bins)
    assert flagged == 0  # no u within 1e-12 of a bin edge: the seeds are chosen so
    x = torch.tensor(xn, device=cuda)
    got = axis_histogram(x, nspins, axis, bins)
    assert got.dtype == torch.int64 and got.shape == (2, bins)
    assert np.array_equal(got.cpu().numpy(), want)
    assert got[0].sum().item() == B * nspins[0] and got[1].sum().item() == B * nspins[1]
    assert torch.equal(axis_histogram(x, nspins, axis, bins), got)  # two calls into zeroed counts


def test_north_pole_is_numpy_histogram_of_cos_theta(cuda):
    xn = IR.walkers(600, 6, seed=9)
    _, flagged = IR.histogram(xn, (4, 2), (0.0, 0.0), 64)
    assert flagged == 0
    got = axis_histogram(torch.tensor(xn, device=cuda), (4, 2), (0.0, 0.0), 64).cpu().numpy()
    c = np.cos(xn[..., 0].astype(np.float64))
    for row, sl in ((0, slice(0, 4)), (1, slice(4, 6))):
        want, _ = np.histogram(c[:, sl], bins=64, range=(-1.0, 1.0))  # ascending in u: bin 63 first
        assert np.array_equal(got[row], want[::-1])


def test_second_call_doubles_and_nan_is_dropped(cuda):
    from deephall_amd import _lib
    from deephall_amd.networks.psiformer import _ptr, _stream

    xn = IR.walkers(300, 5, seed=11).copy()
    xn[3, 1, 0] = np.nan
    xn[4, 4, 1] = np.inf
    want, flagged = IR.histogram(xn, (3, 2), (1.0, 0.5), 20)
    assert flagged == 0 and want[0].sum() == 899 and want[1].sum() == 599
    x = torch.tensor(xn, device=cuda)
    counts = torch.zeros(2, 20, dtype=torch.int32, device=cuda)
    for times in (1, 2):
        _lib.check(_lib.load().dh_axis_histogram(_ptr(x), 300, 3, 2, 1.0, 0.5, 20, _ptr(counts), _stream(cuda)))
        assert np.array_equal(counts.cpu().numpy(), times * want)


HOLE = (1.1, 2.8)


def test_axis_density_through_evaluate(cuda, tmp_path):
    """Laughlin 1/3, N = 4, flux 10 with one hole at (1.1, 2.8) (the quasihole tests' smallest size), a
    zero-strength impurity on the hole so that ``impurity: 0`` names its axis: the density in the bin on
    the hole is below 1, Q(pi) = 0, and ``impurity: 0`` equals the explicit axis."""
    cfg = Config.from_dict({
        "batch_size": 1024, "seed": 11,
        "system": {"nspins": (4, 0), "flux": 10, "impurities": [[HOLE[0], HOLE[1], 0.0, "gaussian", 1.0]]},
        "network": {"type": "quasihole", "halperin": {"exponents": [3, 3, 0]}, "quasihole": {"holes": [list(HOLE)]}},
        "mcmc": {"burn_in": 20},
        "optim": {"iterations": 2, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    ckpt = sorted(tmp_path.glob("ckpt_*.npz"))[-1]
    run = lambda opts: evaluate(DeepHallAdaptor(), ESTIMATORS["axis_density"], ckpt, 10, burn_in=10, seed=5,  # noqa: E731
                                estimator_options=opts)[0]
    out = run({"impurity": 0, "bins": 16})
    same = run({"axis": list(HOLE), "bins": 16})
    assert out["walkers"] == 10 * 1024 and out["counts"].shape == (2, 16)
    assert out["counts"].sum().item() == 10 * 1024 * 4 and out["counts"][1].sum().item() == 0
    for k in ("counts", "theta", "density", "density_err", "excess", "excess_err"):
        assert torch.equal(torch.as_tensor(out[k]).cpu(), torch.as_tensor(same[k]).cpu()), k
    d = out["density"][2]
    print("density", [f"{v:.3f}" for v in d.tolist()], "\nexcess", [f"{v:.3f}" for v in out["excess"].tolist()])
    assert d[0].item() < 1.0  # the hole
    assert abs(out["excess"][-1].item()) < 1e-12 and out["excess"][0].item() < 0
    assert abs(d.mean().item() - 1.0) < 1e-12
