"""Landau-level-resolved one-body density matrix on MI355X (csrc/rdm.hip, netobs/observables/ll_rdm.py).

* the harmonics Y_{Q,Q+n,m} against the float64 restatement (oracle/netobs.py:monopole_harm), the
  level-0 block against dh_monopole_orbitals, and their orthonormality under a Gauss-Legendre x
  uniform-phi rule;
* dh_rdm_accumulate on synthetic log-amplitudes against a numpy restatement in float64, with
  dropped samples, bitwise against itself, by spin, and additive over the points;
* dh_rdm_displace against the torch construction of one_rdm.product;
* a Psiformer with Landau-level mixing: the estimator against the oracle's float64 log-amplitudes,
  its level-0 block against one_rdm;
* the physics pin: the filled lowest Landau level is diag(1, 1, 1, 0, ...);
* the driver on a checkpoint.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd import Config, make_mcmc_step, train
from deephall_amd.netobs import ESTIMATORS, DeepHallAdaptor, HallSystem, evaluate
from deephall_amd.netobs._native import monopole_harmonics, monopole_orbitals, rdm_accumulate, rdm_displace
from deephall_amd.netobs.observables import ll_rdm, one_rdm
from deephall_amd.random import Key
from deephall_amd.train import init_guess
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import netobs as O
from oracle import reference as R
from test_gpu_parity import build
from test_oracle_kat import engineered_params

pytestmark = pytest.mark.gpu


def uniform(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


def harmonics_ref(pts, flux, levels):
    """[..., norb] complex128 from float32 points: level-major, m ascending (oracle/netobs.py)."""
    Q = flux / 2
    pts = np.asarray(pts, dtype=np.float64)
    return np.stack([O.monopole_harm(Q, Q + n, m, pts) for n in range(levels)
                     for m in np.arange(-(Q + n), Q + n + 1)], -1)


class _Adaptor:
    """The adaptor surface the estimator uses: model, call_network."""

    def __init__(self, model, cfg=None):
        self.model, self.cfg = model, cfg

    def call_network(self, params, x, system=None):
        return self.model.apply(params, x)


@pytest.mark.parametrize("flux", [1, 2, 15, 57])
def test_harmonics_match_oracle(cuda, flux):
    levels = 3
    pts = uniform(256, 1, flux)[:, 0]
    pts[:4, 0] = [0.0, 1e-3, np.pi - 1e-3, np.pi]  # the clipped poles
    pd = torch.tensor(pts, device=cuda)
    y = monopole_harmonics(pd, flux, levels).cpu().numpy()
    y_ref = harmonics_ref(pts, flux, levels)
    assert y.shape == y_ref.shape == (256, levels * (flux + 1) + levels * (levels - 1))
    gate = 2e-6 * max(1.0, np.max(np.abs(y_ref)))
    print("harmonics: flux", flux, " max err", np.max(np.abs(y - y_ref)), " gate", gate)
    assert np.max(np.abs(y - y_ref)) < gate
    y0 = monopole_orbitals(pd, flux).cpu().numpy()
    assert np.max(np.abs(y[:, :flux + 1] - y0)) < gate


@pytest.mark.parametrize("flux", [1, 2, 15, 57])
def test_harmonics_are_orthonormal(cuda, flux):
    """96 Gauss-Legendre nodes in cos theta (the largest 0.99969: inside the clip) x 2 l_max + 3
    uniform phi integrate every product of two basis functions exactly (degree <= 2 l_max in
    cos theta after the common powers, |m - m'| <= 2 l_max in phi).  The values are float32 of
    double arithmetic with max |Y| <= 2.2: 2e-5."""
    levels = 3
    xs, ws = np.polynomial.legendre.leggauss(96)
    nphi = flux + 2 * (levels - 1) + 3  # 2 l_max + 3
    phis = -np.pi + 2 * np.pi * np.arange(nphi) / nphi
    pts = np.stack(np.broadcast_arrays(np.arccos(xs)[:, None], phis[None, :]), -1).reshape(-1, 2).astype(np.float32)
    w = np.repeat(ws * 2 * np.pi / nphi, nphi)
    y = monopole_harmonics(torch.tensor(pts, device=cuda), flux, levels).cpu().numpy().astype(np.complex128)
    G = np.einsum("p,pi,pj->ij", w, y.conj(), y)
    print("orthonormality: flux", flux, " max |G - 1|", np.max(np.abs(G - np.eye(G.shape[0]))))
    assert np.max(np.abs(G - np.eye(G.shape[0]))) <= 2e-5


# ---- dh_rdm_accumulate on synthetic log-amplitudes ---------------------------------------------------

def synthetic(B, N, P, seed):
    """Walkers, points and float32 log-amplitudes (Re uniform in [-2, 2], a uniform phase); sample
    (p, b) = (0, 1) has a NaN and (P - 1, 3) a +inf among its displaced log-amplitudes."""
    rng = np.random.default_rng(seed)
    x = uniform(B, N, seed)
    rp = uniform(P * B, 1, seed + 1)[:, 0].reshape(P, B, 2)

    def log(n):
        return np.stack([rng.uniform(-2, 2, n), rng.uniform(-np.pi, np.pi, n)], -1).astype(np.float32)

    lp, lpp = log(B), log(P * B * N)
    lpp[(0 * B + 1) * N + 0, 0] = np.nan
    lpp[((P - 1) * B + 3) * N + N - 1, 0] = np.inf
    return x, rp, lp, lpp


def accumulate_ref(x, rp, lp, lpp, n_up, flux, levels, by_spin):
    """(rho[S, norb, norb] complex128: the sum over the kept samples, the number kept)."""
    B, N, _ = x.shape
    P = rp.shape[0]
    c = lambda a: a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.exp(c(lpp).reshape(P, B, N) - c(lp)[None, :, None])
    keep = np.isfinite(ratio).all(-1) & np.isfinite(c(lp))[None, :]          # [P, B]
    ratio = np.where(keep[..., None], ratio, 0.0)
    phi = harmonics_ref(x, flux, levels)                                     # [B, N, norb]
    phip = harmonics_ref(rp, flux, levels)                                   # [P, B, norb]
    spins = [slice(0, n_up), slice(n_up, N)] if by_spin else [slice(0, N)]
    rho = np.stack([4 * np.pi * np.einsum("pba,bai,pbj->ij", ratio[..., s], phi[:, s], np.conj(phip)) for s in spins])
    return rho, int(keep.sum())


CASES = [(5, 3, 2, 2, 3, 1, True), (257, 6, 6, 15, 3, 2, False), (33, 4, 1, 57, 3, 1, True), (64, 1, 1, 1, 4, 3, False)]


def on_device(cuda, *arrays):
    return [torch.tensor(a, device=cuda) for a in arrays]


@pytest.mark.parametrize("B,N,n_up,flux,levels,P,by_spin", CASES)
def test_accumulate_matches_restatement(cuda, B, N, n_up, flux, levels, P, by_spin):
    """Identical float32 inputs and double arithmetic on both sides: 1e-9 max |rho_ref|."""
    x, rp, lp, lpp = synthetic(B, N, P, seed=B)
    ref, kept = accumulate_ref(x, rp, lp, lpp, n_up, flux, levels, by_spin)
    assert kept == P * B - 2
    xd, rpd, lpd, lppd = on_device(cuda, x, rp, lp, lpp)
    rho, nvalid = rdm_accumulate(xd, rpd, lpd, lppd, n_up, flux, levels, by_spin)
    assert nvalid == kept and rho.shape == ref.shape and rho.dtype == torch.complex128
    err, scale = np.max(np.abs(rho.cpu().numpy() - ref)), np.max(np.abs(ref))
    print("accumulate: max err / max |ref| =", err / scale, " max |ref|", scale)
    assert err <= 1e-9 * scale
    again, nvalid2 = rdm_accumulate(xd, rpd, lpd, lppd, n_up, flux, levels, by_spin)
    assert nvalid2 == nvalid and torch.equal(torch.view_as_real(rho), torch.view_as_real(again))
    # up + down = the unresolved matrix
    both, _ = rdm_accumulate(xd, rpd, lpd, lppd, n_up, flux, levels, True)
    total, _ = rdm_accumulate(xd, rpd, lpd, lppd, n_up, flux, levels, False)
    assert (both.sum(0) - total[0]).abs().max().item() <= 1e-12 * scale
    if n_up == N:
        assert torch.equal(torch.view_as_real(both[1]), torch.zeros_like(torch.view_as_real(both[1])))
    if P == 2:  # the sum over points is the sum of the calls on each point
        parts = [rdm_accumulate(xd, rpd[p:p + 1], lpd, lppd[p * B * N:(p + 1) * B * N], n_up, flux, levels, by_spin)
                 for p in range(P)]
        assert sum(n for _, n in parts) == nvalid
        assert (parts[0][0] + parts[1][0] - rho).abs().max().item() <= 1e-12 * scale


def test_displace_matches_torch(cuda):
    B, N, P = 5, 3, 2
    x, rp = on_device(cuda, uniform(B, N, 1), uniform(P * B, 1, 2)[:, 0].reshape(P, B, 2))
    xp = rdm_displace(x, rp)
    assert xp.shape == (P, B, N, N, 2)
    idx = torch.arange(N, device=cuda)
    for p in range(P):
        ref = x.unsqueeze(1).repeat(1, N, 1, 1)  # one_rdm.product's construction
        ref[:, idx, idx, :] = rp[p][:, None, :]
        assert torch.equal(xp[p], ref)


# ---- a network --------------------------------------------------------------------------------------------

def test_estimator_matches_oracle(cuda):
    """The C2 Psiformer (random parameters: all levels mixed), 8 walkers, levels 2, a given r'."""
    ocfg = oracle_config("C2")
    _, model = build(ocfg)
    p64 = make_params(ocfg, seed=11)
    params = to_device_params(p64)
    x = make_walkers(8, ocfg.nelec, seed=4)
    rp = uniform(8, 1, 9)[:, 0]
    system = HallSystem([6, 0], flux=15)
    est = ll_rdm.LLRDMEstimator(_Adaptor(model), system, {"levels": 2}, {})
    xd, rpd = on_device(cuda, x, rp)
    rho, nvalid = est.accumulate(params, xd, rpd[None])
    assert nvalid == 8 and rho.shape == (1, 34, 34)
    got = (rho[0] / nvalid).cpu().numpy()
    lp = R.batch_logpsi(p64, ocfg, torch.tensor(x, dtype=torch.float64)).numpy()
    xp = np.repeat(x[:, None], 6, 1).astype(np.float64)
    for a in range(6):
        xp[:, a, a] = rp
    lpp = R.batch_logpsi(p64, ocfg, torch.tensor(xp.reshape(-1, 6, 2))).numpy().reshape(8, 6)
    ratio = np.exp(lpp - lp[:, None])
    ref = 4 * np.pi * np.einsum("ba,bai,bj->ij", ratio, harmonics_ref(x, 15, 2), np.conj(harmonics_ref(rp, 15, 2))) / 8
    err, scale = np.max(np.abs(got - ref)), np.max(np.abs(ref))
    print("estimator vs oracle: max err", err, " max |ref|", scale)
    assert err < 2e-4 * scale
    lll = one_rdm.OneRDMEstimator(_Adaptor(model), system, {}, {}).product(params, xd, rpd).mean(0).cpu().numpy()
    assert np.max(np.abs(got[:16, :16] - lll)) < 2e-4 * scale


def test_filled_lll_is_the_lowest_level_identity(cuda):
    """N = 2Q + 1 = 3 fills the lowest Landau level: rho = diag(1, 1, 1, 0, 0, 0, 0, 0) at levels 2.
    A float64 CPU restatement of this case at the same sample size (20 steps x 4096 walkers) gave a
    per-entry standard error of 0.006 and a largest deviation of 0.018: 0.05 is about 8 sigma, and
    the gate of test_filled_lll_one_rdm_is_identity."""
    ocfg = oracle_config("C1", interaction_strength=0.0)
    _, model = build(ocfg)
    params = to_device_params(engineered_params(ocfg))
    B, nsteps = 4096, 20
    x = init_guess(Key(3), B, 3, cuda, network=model)
    step = make_mcmc_step(model, batch_per_device=B, steps=10)
    key = Key(5)
    for _ in range(30):
        x, _ = step(params, x, key, 0.3)
        key = key.advance(10)
    est = ll_rdm.LLRDMEstimator(_Adaptor(model), HallSystem([3, 0], flux=2), {"levels": 2}, {})
    values, state = est.empty_val_state(nsteps)
    for i in range(nsteps):
        x, _ = step(params, x, key, 0.3)
        key = key.advance(10)
        v, state = est.evaluate(i, params, Key(1000 + i), x, None, state, None)
        values["ll_rdm"][i] = v["ll_rdm"].mean(0)
    out = est.digest(values, state)
    rho = out["ll_rdm"][0].numpy()
    print("filled LLL, levels 2:\n", np.round(rho, 3), "\noccupations", out["occupations"].numpy(),
          "+-", out["occupations_err"].numpy(), " residual", out["residual"].item())
    assert state["samples"] == nsteps * B
    assert np.max(np.abs(rho - np.diag([1.0, 1, 1, 0, 0, 0, 0, 0]))) < 0.05
    assert np.max(np.abs(out["occupations"].numpy() - [[3.0, 0.0]])) < 0.05


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
    out, vals = evaluate(DeepHallAdaptor(), ESTIMATORS["ll_rdm"], ckpt, steps, burn_in=3,
                         estimator_options={"levels": 2, "points": 2})
    assert vals["ll_rdm"].shape == (steps, 1, 16, 16)
    assert out["occupations"].shape == (1, 2) and out["occupations_err"].shape == (1, 2)
    for name in ("ll_rdm", "occupations", "occupations_err", "lll_weight", "residual", "natural_occupations",
                 "hermiticity", "lz_offdiag"):
        assert torch.isfinite(torch.view_as_real(out[name]) if out[name].is_complex() else out[name]).all(), name
    print("driver: occupations", out["occupations"].numpy(), " residual", out["residual"].item())
    assert abs(out["occupations"].sum().item() + out["residual"].item() - 3.0) < 1e-12
    assert out["samples"] == steps * 64 * 2
    assert "ll_rdm" not in list(ESTIMATORS)
