"""Renyi-2 swap estimator on MI355X (csrc/swap.hip, netobs/observables/renyi2.py).

* classify, scan and gather against the numpy restatement (tests/renyi2_ref.py), exactly: they
  produce integers and copied floats;
* the edges: no matched pair at all (M = 0), one angle without a matched pair;
* the reduction against the restatement (float64) and bitwise against itself;
* a real network: the trivial regions (nobody / everybody in A) give purity 1, the full product
  matches the restatement fed by the float64 oracle;
* the physics pin: the filled lowest Landau level against entanglement.filled_lll_cap;
* the driver on a checkpoint.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import renyi2_ref as RR
from deephall_amd import Config, make_mcmc_step, train
from deephall_amd.netobs import DeepHallAdaptor, HallSystem, evaluate
from deephall_amd.netobs._native import swap_classify, swap_compact, swap_purity, swap_reduce
from deephall_amd.netobs.entanglement import filled_lll_cap
from deephall_amd.netobs.observables import renyi2
from deephall_amd.random import Key
from deephall_amd.train import init_guess
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_parity import build
from test_oracle_kat import engineered_params

pytestmark = pytest.mark.gpu

EDGE_ANGLES = [0.0, 0.7, math.pi / 2, 2.4, 3.2]  # at 0 nobody is in A, at 3.2 everybody


def uniform(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


class _Adaptor:
    """The adaptor surface the estimator uses: model, call_network."""

    def __init__(self, model, cfg=None):
        self.model, self.cfg = model, cfg

    def call_network(self, params, x, system=None):
        return self.model.apply(params, x)


class _RecordingApply:
    """A stand-in wavefunction (smooth in the coordinates) that keeps what it was asked and answered."""

    def __init__(self):
        self.rows, self.logs = [], []

    def __call__(self, rows):
        w = torch.arange(1, rows.shape[1] + 1, device=rows.device, dtype=torch.float32)
        lp = torch.complex((torch.sin(rows[..., 0] * w) * 0.4).sum(-1), (rows[..., 1] * w).sum(-1) * 0.3)
        self.rows.append(rows.clone())
        self.logs.append(lp.clone())
        return lp


def as_complex(t):
    return t.cpu().numpy().astype(np.complex128)


# P = 257 crosses a 256-thread block; (20, 0) is the widest system; B = 7 leaves an odd walker out
@pytest.mark.parametrize("nspins,B", [((3, 0), 10), ((2, 1), 514), ((20, 0), 66), ((2, 2), 7)])
def test_classify_scan_gather_match_restatement(cuda, nspins, B):
    x = uniform(B, sum(nspins), seed=B)
    sector_ref, counts_ref = RR.classify(x, EDGE_ANGLES, nspins)
    M_ref, start_ref, pair_ref, xs_ref = RR.compact(x, EDGE_ANGLES, nspins, sector_ref)
    P = B // 2
    assert (sector_ref[0] == 0).all() and (sector_ref[-1] >= 0).all()  # the trivial regions match every pair
    assert 2 * P < M_ref < 5 * P                                      # and some pair in between does not
    xd = torch.tensor(x, device=cuda)
    sector, counts = swap_classify(xd, EDGE_ANGLES, nspins)
    M, start, pair, xs = swap_compact(xd, EDGE_ANGLES, nspins, sector)
    assert torch.equal(sector.cpu(), torch.tensor(sector_ref))
    assert torch.equal(counts.cpu().long(), torch.tensor(counts_ref))
    assert M == M_ref
    assert torch.equal(start.cpu(), torch.tensor(start_ref))
    assert torch.equal(pair.cpu(), torch.tensor(pair_ref))
    assert torch.equal(xs.cpu(), torch.tensor(xs_ref))
    assert counts.sum().item() == 2 * P * len(EDGE_ANGLES)


def test_no_matched_pair_at_all(cuda):
    """One walker all-north, its partner all-south, the equator as the cut: M = 0."""
    x = torch.tensor([[[0.3, 0.1], [0.5, -2.0], [0.9, 1.0]], [[2.2, 0.4], [2.8, 2.0], [1.9, -1.0]]], device=cuda)
    thetas, nspins = [math.pi / 2], (3, 0)
    sector, counts = swap_classify(x, thetas, nspins)
    M, start, pair, xs = swap_compact(x, thetas, nspins, sector)
    assert M == 0 and pair.numel() == 0 and xs.shape == (0, 3, 2)
    assert sector.cpu().tolist() == [[-1]] and start.cpu().tolist() == [0, 0]
    assert counts.cpu().tolist() == [[1, 0, 0, 1]]
    lp = torch.zeros(2, 2, device=cuda)
    sums = swap_reduce(lp, None, nspins, 0, pair, sector, start)
    assert torch.equal(sums.cpu(), torch.zeros(1, 4, dtype=torch.complex128))
    f = _RecordingApply()
    sums, counts = swap_purity(f, x, thetas, nspins)
    assert len(f.rows) == 1  # no second wavefunction call
    assert torch.equal(sums.cpu(), torch.zeros(1, 4, dtype=torch.complex128))
    assert counts.dtype == torch.int64 and counts.cpu().tolist() == [[1, 0, 0, 1]]


def test_one_angle_without_a_matched_pair(cuda):
    """Counts in the caps 0.4 / 1.5 / 3.2: pair 0 = (1, 1) / (1, 2) / (2, 2), pair 1 = (0, 0) / (2, 1) / (2, 2)."""
    x = torch.tensor([[[0.2, 0.3], [2.0, -1.0]], [[0.5, 1.0], [1.0, 2.5]],
                      [[0.3, -0.7], [1.2, 0.2]], [[0.6, 1.4], [2.9, -2.0]]], device=cuda)
    thetas, nspins = [0.4, 1.5, 3.2], (2, 0)
    f = _RecordingApply()
    sums, counts = swap_purity(f, x, thetas, nspins)
    assert len(f.rows) == 2 and f.rows[1].shape == (8, 2, 2)
    sector_ref, counts_ref = RR.classify(x.cpu().numpy(), thetas, nspins)
    assert (sector_ref[1] == -1).all() and (sector_ref[[0, 2]] >= 0).all()
    assert torch.equal(counts.cpu(), torch.tensor(counts_ref))
    assert torch.equal(sums[1].cpu(), torch.zeros(3, dtype=torch.complex128))
    # the other angles: as if the empty one had not been asked for (bitwise), and right
    g = _RecordingApply()
    sums2, _ = swap_purity(g, x, [0.4, 3.2], nspins)
    assert torch.equal(sums[[0, 2]], sums2)
    M, _, pair_ref, xs_ref = RR.compact(x.cpu().numpy(), thetas, nspins, sector_ref)
    assert torch.equal(f.rows[1].cpu(), torch.tensor(xs_ref))
    ref, mags = RR.reduce(as_complex(f.logs[0]), as_complex(f.logs[1]), nspins, pair_ref, sector_ref)
    assert (mags[[0, 2]].sum(-1) > 0).all()
    assert (np.abs(sums.cpu().numpy() - ref) <= 1e-12 * mags).all()


def test_reduce_matches_restatement_and_is_deterministic(cuda):
    """Synthetic float32 logs, real parts in +-30: the device sums differ from numpy's float64
    sums in the order of summation (and the last bits of exp / sincos) only."""
    nspins, B = (2, 1), 514
    x = uniform(B, 3, seed=B)
    xd = torch.tensor(x, device=cuda)
    sector, _ = swap_classify(xd, EDGE_ANGLES, nspins)
    M, start, pair, _ = swap_compact(xd, EDGE_ANGLES, nspins, sector)
    rng = np.random.default_rng(7)
    lp = np.stack([rng.uniform(-30, 30, B), rng.uniform(-np.pi, np.pi, B)], -1).astype(np.float32)
    lps = np.stack([rng.uniform(-30, 30, 2 * M), rng.uniform(-np.pi, np.pi, 2 * M)], -1).astype(np.float32)
    args = (torch.tensor(lp, device=cuda), torch.tensor(lps, device=cuda), nspins, M, pair, sector, start)
    got = swap_reduce(*args)
    again = swap_reduce(*args)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(again))
    c = lambda a: a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64)  # noqa: E731
    ref, mags = RR.reduce(c(lp), c(lps), nspins, pair.cpu().numpy(), sector.cpu().numpy())
    err = np.abs(got.cpu().numpy() - ref)
    filled = mags > 0
    print("reduce: max err / sum|terms| =", np.max(err[filled] / mags[filled]), " sectors filled:", filled.sum())
    assert (mags > 0).sum() >= 12  # 5 angles x 6 sectors, the trivial regions fill one each
    assert (err <= 1e-12 * mags).all()


@pytest.fixture(scope="module")
def c2():
    """The small C2 Psiformer of test_one_rdm_product_matches_oracle and 8 walkers."""
    ocfg = oracle_config("C2")
    _, model = build(ocfg)
    p64 = make_params(ocfg, seed=11)
    return ocfg, model, p64, to_device_params(p64), make_walkers(8, ocfg.nelec, seed=6)


def test_trivial_regions_give_unit_purity(cuda, c2):
    """theta = 0: nobody in A, R' = R.  theta = 3.2: everybody, R1' = R2 and R2' = R1.  The value
    is exp(0) up to dh_logpsi evaluating the same configuration at another batch position."""
    ocfg, model, p64, params, x = c2
    xd = torch.tensor(x, device=cuda)
    sector, _ = swap_classify(xd, [0.0, 3.2], (6, 0))
    M, start, pair, xs = swap_compact(xd, [0.0, 3.2], (6, 0), sector)
    assert M == 8 and start.cpu().tolist() == [0, 4, 8]
    assert sector.cpu().tolist() == [[0] * 4, [6] * 4]
    rows = xs.reshape(2, 4, 2, 6, 2)  # [angle, pair, member]
    assert torch.equal(rows[0, :, 0], xd[:4]) and torch.equal(rows[0, :, 1], xd[4:])
    assert torch.equal(rows[1, :, 0], xd[4:]) and torch.equal(rows[1, :, 1], xd[:4])
    sums, _ = swap_purity(lambda r: model.apply(params, r), xd, [0.0, 3.2], (6, 0))
    purity = (sums.sum(-1) / 4).cpu().numpy()
    print("trivial regions: purity - 1 =", purity - 1)
    assert np.max(np.abs(purity - 1.0)) < 1e-4


def test_swap_product_matches_oracle(cuda, c2):
    """The sums of a random Psiformer against the restatement with the oracle's float64 logs."""
    ocfg, model, p64, params, x = c2
    thetas = [0.9, math.pi / 2, 2.2]
    logpsi64 = lambda rows: R.batch_logpsi(p64, ocfg, torch.tensor(rows, dtype=torch.float64)).numpy()  # noqa: E731
    ref, counts_ref, M = RR.swap_sums(logpsi64, x, thetas, (6, 0))
    sector_ref, _ = RR.classify(x, thetas, (6, 0))
    assert ((sector_ref >= 0).sum(-1) >= 1).all()  # the seed: at least one matched pair at each angle
    sums, counts = swap_purity(lambda r: model.apply(params, r), torch.tensor(x, device=cuda), thetas, (6, 0))
    assert torch.equal(counts.cpu(), torch.tensor(counts_ref))
    err = np.max(np.abs(sums.cpu().numpy() - ref))
    print("swap product: max err", err, " max |ref|", np.max(np.abs(ref)), " M", M)
    assert err < 2e-4 * np.max(np.abs(ref))


def test_filled_lll_cap_purity(cuda):
    """N = 2Q + 1 = 3 fills the lowest Landau level: free fermions, entanglement.filled_lll_cap
    is exact.  20 steps x 2048 pairs; the gate is 10 x 0.49 / sqrt(20 x 2048) = 0.024 with 0.49
    the per-pair standard deviation of the swap value (measured on a CPU sampler of this state)
    and the factor 10 for the correlation between successive steps.  A wrong denominator gives
    about 0.7 and a broken bijection sign noise: both far outside."""
    ocfg = oracle_config("C1", interaction_strength=0.0)
    _, model = build(ocfg)
    params = to_device_params(engineered_params(ocfg))
    B, nsteps = 4096, 20
    thetas = [math.pi / 3, math.pi / 2, 2 * math.pi / 3]
    x = init_guess(Key(3), B, 3, cuda, network=model)
    step = make_mcmc_step(model, batch_per_device=B, steps=10)
    key = Key(5)
    for _ in range(30):
        x, _ = step(params, x, key, 0.3)
        key = key.advance(10)
    est = renyi2.Renyi2Estimator(_Adaptor(model), HallSystem([3, 0], flux=2), {"thetas": thetas}, {})
    values, state = est.empty_val_state(nsteps)
    for i in range(nsteps):
        x, _ = step(params, x, key, 0.3)
        key = key.advance(10)
        v, state = est.evaluate(i, params, None, x, None, state, None)
        values["purity"][i] = v["purity"].mean(0)
    out = est.digest(values, state)
    exact, exact_sector, exact_number = filled_lll_cap(2, thetas)
    gate = 10 * 0.49 / math.sqrt(nsteps * (B // 2))
    purity = out["purity"].numpy()
    print("filled LLL purity:", purity, " exact:", exact, " imag:", out["purity_imag"].numpy(),
          " err:", (out["renyi2_err"] * out["purity"]).numpy())
    print("sector purity:\n", out["sector_purity"].numpy(), "\nexact:\n", exact_sector)
    print("P(n):\n", out["number_distribution"].numpy(), "\nexact:\n", exact_number)
    assert state["pairs"] == nsteps * (B // 2) and state["counts"].sum().item() == nsteps * B * 3
    assert np.max(np.abs(purity - exact)) < gate
    assert np.max(np.abs(out["purity_imag"].numpy())) < gate
    assert np.max(np.abs(out["number_distribution"].numpy() - exact_number)) < 0.01
    assert np.max(np.abs(out["sector_purity"].numpy() - exact_sector)) < gate
    assert np.allclose(out["renyi2"].numpy(), -np.log(purity))


def test_driver_on_a_checkpoint(cuda, tmp_path):
    cfg = Config.from_dict({
        "batch_size": 64, "seed": 3,
        "system": {"nspins": (3, 0), "flux": 6, "interaction_strength": 0.0},
        "network": {"psiformer": {"num_layers": 1, "num_heads": 1, "heads_dim": 4}},
        "mcmc": {"burn_in": 5},
        "optim": {"iterations": 3, "optimizer": "adam"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    ckpt = sorted(tmp_path.glob("ckpt_*.npz"))[-1]
    steps = 4
    out, vals = evaluate(DeepHallAdaptor(), renyi2.DEFAULT, ckpt, steps, burn_in=3, estimator_options={"thetas": 5})
    assert vals["purity"].shape == (steps, 5, 4)
    assert out["renyi2"].shape == (5,) and out["renyi2_err"].shape == (5,)
    assert torch.isfinite(out["sector_purity"]).all() and out["sector_purity"].shape == (5, 4)
    assert torch.allclose(out["number_distribution"].sum(-1), torch.ones(5, dtype=torch.float64))
    assert out["counts"].sum().item() == steps * 64 * 5 and out["pairs"] == steps * 32
