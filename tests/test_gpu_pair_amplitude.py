"""Pair amplitudes on MI355X (csrc/pairamp.hip, netobs/observables/pair_amplitude.py).

* dh_pair_displace against torch indexing, exactly;
* dh_pair_kernel against the float64 closed form (pairamp_ref.py), with poles, coincident electrons,
  coincident points and the primed pair on the unprimed one;
* dh_pair_accumulate on synthetic log-amplitudes against the numpy restatement, with dropped
  samples, bitwise against itself, by class;
* the physics pins on the native walk: the filled lowest level, Laughlin 1/3 (with the Coulomb and
  harmonic energies from the pseudopotentials against the potential of the same walkers) and
  Halperin (3, 3, 1);
* the C2 Psiformer: its dh_logpsi values against the oracle's float64 logs through the same
  accumulation.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pairamp_ref as PR
from deephall_amd import PRNGKey, config, make_mcmc_step, make_network
from deephall_amd.netobs import ESTIMATORS, DeepHallAdaptor, HallSystem
from deephall_amd.netobs._native import (_log_pairs, pair_accumulate, pair_amplitude_sums, pair_displace,
                                         pair_kernel)
from deephall_amd.hamiltonian import make_potential
from deephall_amd.random import Key
from deephall_amd.train import init_guess
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_parity import build
from test_oracle_kat import engineered_params

pytestmark = pytest.mark.gpu


def on_device(cuda, *arrays):
    return [torch.tensor(a, device=cuda) for a in arrays]


def bits(t):
    return torch.view_as_real(t)


# ---- 1. dh_pair_displace ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N", [(5, 3), (257, 6), (5, 6), (257, 3)])
def test_displace_matches_torch(cuda, B, N):
    P, npairs = 2, N * (N - 1) // 2
    x, r1, r2 = on_device(cuda, PR.uniform(B, N, 1), PR.uniform(P * B, 1, 2)[:, 0].reshape(P, B, 2),
                          PR.uniform(P * B, 1, 3)[:, 0].reshape(P, B, 2))
    ref = x[None, None].repeat(npairs, P, 1, 1, 1)
    for q, (i, j) in enumerate(PR.pair_list(N)):
        ref[q, :, :, i] = r1
        ref[q, :, :, j] = r2
    xp = pair_displace(x, r1, r2)
    assert xp.shape == (npairs, P, B, N, 2) and torch.equal(xp, ref)
    part = pair_displace(x, r1, r2, 1, npairs - 1)  # a window that is not the whole set
    assert part.shape == (npairs - 2, P, B, N, 2) and torch.equal(part, ref[1:npairs - 1])


# ---- 2. dh_pair_kernel -----------------------------------------------------------------------------------

def special_quadruples(flux):
    """64 quadruples [64, 4, 2] float32: random ones, then 0: electrons at the poles, 1: r1 = r2,
    2: r1' = r2', 3: the primed pair on the unprimed pair, 4: all of these at once at a pole."""
    pts = PR.uniform(64, 4, seed=flux)
    pts[0, 0, 0], pts[0, 1, 0], pts[0, 2, 0] = 0.0, np.pi, 0.0
    pts[1, 1] = pts[1, 0]
    pts[2, 3] = pts[2, 2]
    pts[3, 2:] = pts[3, :2]
    pts[4, :, 0] = 0.0
    pts[4, :, 1] = pts[4, 0, 1]
    return pts


@pytest.mark.parametrize("flux", [1, 2, 15, 57, 126])
def test_kernel_matches_closed_form(cuda, flux):
    """Identical float32 points and double arithmetic on both sides: 1e-9 (2Q + 1)^2 per entry, the
    scale of K_L (its sum over L at coincident pairs is (2Q + 1)^2)."""
    pts = special_quadruples(flux)
    got = pair_kernel(torch.tensor(pts, device=cuda), flux).cpu().numpy()
    ref = PR.pair_kernel(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux)
    assert got.shape == ref.shape == (64, flux + 1) and np.isfinite(got.view(np.float64)).all()
    gate = 1e-9 * (flux + 1) ** 2
    print("kernel: flux", flux, " max err", np.max(np.abs(got - ref)), " gate", gate, " max |K|", np.max(np.abs(ref)))
    assert np.max(np.abs(got - ref)) <= gate
    # r1 = r2 or r1' = r2': d = 0 exactly, only L = 2Q is left, n_2Q p_2Q
    for row in (1, 2, 4):
        assert (got[row, :flux] == 0).all()
        a, b, _ = PR.geometry(*pts[row])
        want = PR.norms(flux)[flux] * PR.p_recurrence(a, b, 0.0, flux)[flux]
        assert abs(got[row, flux] - want) <= gate
    # the primed pair on the unprimed one: real and not negative
    assert np.max(np.abs(got[3].imag)) <= gate and np.min(got[3].real) >= -gate


def test_kernel_marks_a_bad_point(cuda):
    pts = special_quadruples(9)
    pts[7, 2, 1] = np.nan
    pts[9, 0, 0] = np.inf
    got = pair_kernel(torch.tensor(pts, device=cuda), 9).cpu().numpy()
    bad = np.isnan(got.real).all(-1) & np.isnan(got.imag).all(-1)
    assert bad.tolist() == [k in (7, 9) for k in range(64)] and np.isfinite(got[~bad].view(np.float64)).all()


# ---- 3. dh_pair_accumulate on synthetic log-amplitudes ----------------------------------------------------

def synthetic(B, N, P, seed):
    """Walkers, points and float32 log-amplitudes (Re uniform in [-2, 2], a uniform phase); sample
    (p, b) = (0, 1) has a NaN in the log of its first pair and (P - 1, 3) a +inf in that of its last."""
    rng = np.random.default_rng(seed)
    npairs = N * (N - 1) // 2
    x = PR.uniform(B, N, seed)
    r1 = PR.uniform(P * B, 1, seed + 1)[:, 0].reshape(P, B, 2)
    r2 = PR.uniform(P * B, 1, seed + 2)[:, 0].reshape(P, B, 2)

    def log(n):
        return np.stack([rng.uniform(-2, 2, n), rng.uniform(-np.pi, np.pi, n)], -1).astype(np.float32)

    lp, lpp = log(B), log(npairs * P * B)
    lpp[(0 * P + 0) * B + 1, 0] = np.nan
    lpp[((npairs - 1) * P + P - 1) * B + 3, 0] = np.inf
    return x, r1, r2, lp, lpp


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [5, 33, 257])
@pytest.mark.parametrize("N,n_up,flux", [(3, 3, 2), (4, 2, 5), (6, 3, 15)])
def test_accumulate_matches_restatement(cuda, N, n_up, flux, B, P):
    """Identical float32 inputs and double arithmetic on both sides: 1e-9 max |A_ref|.  The classes
    against the total is a relative bound too, 1e-12 max |A_ref|: the two are sums of the same
    thousands of terms of size up to e^4 (2Q + 1)^2 in different orders."""
    x, r1, r2, lp, lpp = synthetic(B, N, P, seed=B + N)
    ref, kept = PR.accumulate(x, r1, r2, lp, lpp, n_up, flux)
    assert kept == P * B - 2
    dev = on_device(cuda, x, r1, r2, lp, lpp)
    A, nvalid = pair_accumulate(*dev, n_up, flux)
    assert nvalid == kept and A.shape == ref.shape == (3, flux + 1) and A.dtype == torch.complex128
    err, scale = np.max(np.abs(A.cpu().numpy() - ref)), np.max(np.abs(ref))
    print("accumulate: max err / max |ref| =", err / scale, " max |ref|", scale)
    assert err <= 1e-9 * scale
    again, nvalid2 = pair_accumulate(*dev, n_up, flux)
    assert nvalid2 == nvalid and torch.equal(bits(A), bits(again))
    # the classes add up to all pairs, which is the up-up class when every slot is up
    total, _ = pair_accumulate(*dev, N, flux)
    assert (A.sum(0) - total[0]).abs().max().item() <= 1e-12 * scale
    assert torch.equal(bits(total[1:]), torch.zeros_like(bits(total[1:])))
    if n_up == N:
        assert torch.equal(bits(A[1:]), torch.zeros_like(bits(A[1:])))


def test_accumulate_with_every_sample_invalid(cuda):
    x, r1, r2, lp, lpp = synthetic(33, 3, 1, seed=4)
    lp[:, 0] = np.nan
    A, nvalid = pair_accumulate(*on_device(cuda, x, r1, r2, lp, lpp), 2, 4)
    assert nvalid == 0 and torch.equal(bits(A), torch.zeros_like(bits(A)))


def test_sums_take_whole_pairs_in_windows(cuda):
    """A wavefunction that is a product of one-body factors: the windows of max_rows change nothing."""
    B, N, P, flux = 33, 4, 2, 5
    x, r1, r2 = on_device(cuda, PR.uniform(B, N, 5), PR.uniform(P * B, 1, 6)[:, 0].reshape(P, B, 2),
                          PR.uniform(P * B, 1, 7)[:, 0].reshape(P, B, 2))
    calls = []

    def apply(rows):
        calls.append(rows.shape[0])
        return torch.complex(torch.cos(rows[..., 0]).sum(-1), rows[..., 1].sum(-1))

    whole, n0 = pair_amplitude_sums(apply, x, r1, r2, 2, flux)
    assert calls == [B, 6 * P * B] and n0 == P * B
    calls.clear()
    parts, n1 = pair_amplitude_sums(apply, x, r1, r2, 2, flux, max_rows=2 * P * B + 1)
    assert calls == [B] + [2 * P * B] * 3 and n1 == n0 and torch.equal(bits(whole), bits(parts))
    calls.clear()
    pair_amplitude_sums(apply, x, r1, r2, 2, flux, max_rows=1)  # at least one pair per call
    assert calls == [B] + [P * B] * 6


# ---- 4. physics on the native walk ------------------------------------------------------------------------

CAP = {2: 0.03, 5: 0.08, 9: 0.08}  # the largest standard error a bound may pass with, by 2Q


def _network(kind, nspins, flux, itype="coulomb", exponents=None):
    net = config.Network()
    net.type = config.NetworkType(kind)
    if exponents:
        net.halperin.exponents = exponents
    system = config.System(nspins=nspins, flux=flux, interaction_type=config.InteractionType(itype))
    return system, make_network(system, net)


def _adaptor(system, model):
    """A DeepHallAdaptor as ``restore`` leaves it, without a checkpoint."""
    adaptor = DeepHallAdaptor()
    adaptor.cfg, adaptor.model = SimpleNamespace(system=system), model
    Q = system.flux / 2
    adaptor.potential_energy = make_potential(system.interaction_type, Q, system.radius or math.sqrt(Q))
    adaptor.external_energy = None
    return adaptor


def _measure(cuda, system, model, params, x, width, *, steps=20, burn=40, walk_steps=40, tune=True, options=None):
    """netobs.evaluate's loop without the checkpoint: burn in (tuning the move width to an acceptance of
    0.5 .. 0.55 where asked), then steps x (walk, evaluate, the adaptor's potential), then the digest.
    Returns (digest, step values, the mean potential of the walkers the estimator saw)."""
    B = x.shape[0]
    adaptor = _adaptor(system, model)
    walk = make_mcmc_step(model, batch_per_device=B, steps=walk_steps)
    key = Key(29)
    for _ in range(burn):
        x, pmove = walk(params, x, key, width)
        key = key.advance(walk_steps)
        if tune:
            width *= 1.1 if float(pmove) > 0.55 else (1 / 1.1 if float(pmove) < 0.5 else 1.0)
    hall = HallSystem(spins=list(system.nspins), flux=system.flux)
    est = ESTIMATORS["pair_amplitude"](adaptor, hall, options, {})
    values, state = est.empty_val_state(steps)
    pot = []
    for i in range(steps):
        x, pmove = walk(params, x, key, width)
        key = key.advance(walk_steps)
        vals, state = est.evaluate(i, params, Key(1000 + i), x, hall, state, None)
        values["pair_amplitude"][i] = vals["pair_amplitude"].mean(0)
        pot.append(adaptor.call_local_potential_energy(params, None, x).double().mean().item())
    assert state["samples"] == steps * B * est.points
    out = est.digest(values, state)
    print(f"  width {width:.2f}, acceptance {float(pmove):.2f}, imag {out['imag'].item():.4f}, "
          f"forbidden {out['forbidden'].item():.4f}, pairs_in_lll {out['pairs_in_lll'].item():.4f}")
    return out, values["pair_amplitude"], float(np.mean(pot))


def _close(label, got, err, exact, cap):
    """|estimate - exact| <= 5 err with err <= cap: the cap keeps noise from hiding a failure."""
    print(f"  {label} = {got:.5f}, exact {exact:.5f}, err {err:.5f} (cap {cap}): {abs(got - exact) / err:.2f} err")
    assert err <= cap and abs(got - exact) <= 5 * err


def _close_amp(out, c, L, exact, flux, label):
    _close(f"{label} A[{'uu ud dd'.split()[c]}][L={L}]", out["amplitudes"][c, L].item(),
           out["amplitudes_err"][c, L].item(), exact, CAP[flux])


def _close_sum(out, steps, exact, flux, label):
    """sum_L A_L over the classes, its error from the steps' sums, under the same cap as one A_L."""
    sums = steps.real.sum(dim=(1, 2))
    err = sums.std(unbiased=True).item() / math.sqrt(sums.shape[0])
    assert abs(sums.mean().item() - out["total"].sum().item()) < 1e-12
    _close(f"{label} sum_L A_L", sums.mean().item(), err, exact, CAP[flux])
    return err


def test_filled_level_has_all_pairs_at_relative_momentum_one(cuda):
    """N = 2Q + 1 = 3 fills the lowest Landau level (the Psiformer with engineered parameters, as in
    test_gpu_ll_rdm.py): a Vandermonde state, every pair at m = 1, A = (0, 3, 0)."""
    ocfg = oracle_config("C1", interaction_strength=0.0)
    _, model = build(ocfg)
    params = to_device_params(engineered_params(ocfg))
    x = init_guess(Key(3), 4096, 3, cuda, network=model)
    system = config.System(nspins=(3, 0), flux=2, interaction_strength=0.0)
    out, steps, _ = _measure(cuda, system, model, params, x, 0.3, burn=30, walk_steps=10, tune=False)
    for L, exact in enumerate([0.0, 3.0, 0.0]):
        _close_amp(out, 0, L, exact, 2, "filled")
    _close_sum(out, steps, 3.0, 2, "filled")
    assert out["amplitudes"][1:].abs().max().item() == 0.0 and out["coulomb_energy"].item() == 0.0


@pytest.mark.parametrize("itype", ["coulomb", "harmonic"])
def test_laughlin_third(cuda, itype):
    """nspins (4, 0) at flux 9: no pair below m = 3, so A_9 = A_8 = A_7 = 0 (A_8 by antisymmetry
    already), sum_L A_L = 6, and the energy sum_L V_L A_L is the mean of the adaptor's potential over
    the same walkers: 5 x its own error, which must be under 5 % of the value."""
    system, model = _network("laughlin", (4, 0), 9, itype)
    x = torch.tensor(PR.uniform(4096, 4, seed=17), device=cuda)
    out, steps, pot = _measure(cuda, system, model, model.init(PRNGKey(0), device=cuda), x, 0.3)
    for L in (9, 8, 7):
        _close_amp(out, 0, L, 0.0, 9, "laughlin 1/3")
    err = _close_sum(out, steps, 6.0, 9, "laughlin 1/3")
    _close("laughlin 1/3 pairs_in_lll", out["pairs_in_lll"].item(), err / 6, 1.0, CAP[9] / 6)
    got, e_err = out[f"{itype}_energy"].item(), out[f"{itype}_energy_err"].item()
    _close(f"laughlin 1/3 {itype} energy against the potential", got, e_err, pot, 0.05 * abs(pot))


def test_halperin_331(cuda):
    """nspins (2, 2) at flux 5: up-down pairs start at m = 1 (A_5 = 0), same-species pairs at m = 3
    (A_4 = 0, and A_5, A_3, A_1 by antisymmetry: ``forbidden``)."""
    system, model = _network("halperin", (2, 2), 5, exponents=(3, 3, 1))
    x = torch.tensor(PR.uniform(4096, 4, seed=17), device=cuda)
    out, steps, _ = _measure(cuda, system, model, model.init(PRNGKey(0), device=cuda), x, 0.3)
    _close_amp(out, 1, 5, 0.0, 5, "halperin 331")
    worst = 0.0
    for c in (0, 2):
        _close_amp(out, c, 4, 0.0, 5, "halperin 331")
        for L in (5, 3, 1):  # even m
            _close_amp(out, c, L, 0.0, 5, "halperin 331")
            worst = max(worst, abs(out["amplitudes"][c, L].item()))
    assert out["forbidden"].item() == worst  # each of its entries is within its bound
    _close_sum(out, steps, 6.0, 5, "halperin 331")


# ---- 5. a network -------------------------------------------------------------------------------------------

def test_psiformer_logs_against_the_oracle(cuda):
    """The C2 Psiformer (random parameters), 64 walkers, one point: dh_logpsi's values and the oracle's
    float64 logs of the same rows through the same accumulation; 2e-4 of max |A|, ll_rdm's bound."""
    ocfg = oracle_config("C2")
    _, model = build(ocfg)
    p64 = make_params(ocfg, seed=11)
    params = to_device_params(p64)
    B, N, flux = 64, 6, 15
    x = make_walkers(B, N, seed=4)
    r1, r2 = PR.uniform(B, 1, 9)[:, 0][None], PR.uniform(B, 1, 10)[:, 0][None]
    xd, r1d, r2d = on_device(cuda, x, r1, r2)
    xp = pair_displace(xd, r1d, r2d)
    assert torch.equal(xp.cpu(), torch.tensor(PR.displace(x, r1, r2)))
    rows = xp.reshape(-1, N, 2)
    got, nvalid = pair_accumulate(xd, r1d, r2d, _log_pairs(model.apply(params, xd)),
                                  _log_pairs(model.apply(params, rows)), N, flux)
    lp = R.batch_logpsi(p64, ocfg, torch.tensor(x, dtype=torch.float64))
    lpp = R.batch_logpsi(p64, ocfg, rows.cpu().double())
    ref, nref = pair_accumulate(xd, r1d, r2d, _log_pairs(lp.to(cuda)), _log_pairs(lpp.to(cuda)), N, flux)
    assert nvalid == nref == B
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print("psiformer vs oracle logs: max err", err, " max |A|", scale, " sum_L A_L / pairs",
          (got.real.sum() / nvalid / 15).item())
    assert err < 2e-4 * scale
    # and the estimator's own route, four pairs to a wavefunction call, gives the same numbers within that bound
    est = ESTIMATORS["pair_amplitude"](SimpleNamespace(model=model, call_network=lambda p, rows: model.apply(p, rows)),
                                       HallSystem([6, 0], flux=flux), {"max_rows": 4 * B}, {})
    A, n = est.accumulate(params, xd, r1d, r2d)
    assert n == B and (A - got).abs().max().item() < 2e-4 * scale
