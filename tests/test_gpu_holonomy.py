"""Quasihole overlap matrix and Berry phases on MI355X (csrc/quasihole.hip hole_logs_kernel,
csrc/holes.hip, netobs/observables/hole_overlap.py, netobs/holonomy.py).

(a) hole_logs against the float64 restatement (tests/holonomy_ref.py) on uniform walkers;
(b) hole_logs rounded to float32 against dh_logpsi of a Quasihole handle per configuration: bits;
(c) hole_gram on synthetic logs against numpy, its dropped walkers, its bits, its shift;
(d) zero-variance identities: identical configurations, coincident groups, the three pairings;
(e) the exact coherent-state overlaps through evaluate(ESTIMATORS["hole_overlap"]);
(f) berry_phase on a short open path against the exact links.
"""

from __future__ import annotations

import cmath
import math

import numpy as np
import pytest
import torch

import holonomy_ref as HR
from deephall_amd import Config, train
from deephall_amd.netobs import ESTIMATORS, DeepHallAdaptor, evaluate, holonomy as H
from deephall_amd.netobs._native import hole_gram, hole_logs, hole_table
from deephall_amd.networks import Quasihole

pytestmark = pytest.mark.gpu

RE_BOUND, PHASE_BOUND = 9.6e-15, 9.4e-13  # (a): 10 x the measured maxima, see test_hole_logs_match_restatement


def table_of(system, configs):
    return hole_table(Quasihole(**system, **configs[0]).spec, HR.states(system, configs))


_cache = {}


def case_logs(name, cuda):
    """(x and the kernel's L [B, K] complex128 on the device, the restatement's L in numpy), once per case"""
    if name not in _cache:
        system, _, configs = HR.CASES[name]
        x = torch.tensor(HR.case_walkers(name), device=cuda)
        L = hole_logs(x, table_of(system, configs))
        _cache[name] = (x, L, HR.logs(system, configs, x.cpu().numpy()))
    return _cache[name]


@pytest.mark.parametrize("name", list(HR.CASES))
def test_hole_logs_match_restatement(cuda, name):
    """Re (relative to max(1, |Re|)) and the wrapped phase of L against `QuasiholeCallable` in float64 on
    the same float32 walkers, walkers with a |w| or |s| below 1e-3 excluded (none of these: at most 2 %).

    Measured maximum over the cases on MI355X: Re 9.6e-16 (pfaffian6-pairings), phase 9.4e-14
    (laughlin32-8holes-K16, 1520 phases added per walker).  The bounds are 10 x those, Re 9.6e-15 and phase
    9.4e-13, and no looser than 1e-9."""
    system, B, configs = HR.CASES[name]
    x, L, L_ref = case_logs(name, cuda)
    assert L.shape == (B, len(configs)) and L.dtype == torch.complex128
    keep = HR.smallest_distance(x.cpu().numpy(), configs) >= 1e-3
    assert keep.mean() >= 0.98
    re, im = HR.deviation(L.cpu().numpy()[keep], L_ref[keep])
    print(f"{name}: log psi re {re.max():.2e} phase {im.max():.2e}  ({(~keep).sum()} walkers excluded)")
    assert re.max() < RE_BOUND and im.max() < PHASE_BOUND
    assert np.all(np.abs(L.cpu().numpy().imag) <= math.pi)  # reduced as dh_logpsi reduces it


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(HR.CASES))
def test_hole_logs_round_to_dh_logpsi(cuda, name):
    """L[:, c] rounded to float32 is dh_logpsi of the Quasihole handle of configuration c, bit for bit,
    Re and (already reduced by the same remainder) Im: the two kernels share their functions."""
    system, _, configs = HR.CASES[name]
    x, L, _ = case_logs(name, cuda)
    for c, config in enumerate(configs):
        model = Quasihole(**system, **config)
        lp = torch.view_as_real(model.apply(model.init(0, device=cuda), x))
        assert lp.dtype == torch.float32
        got = torch.view_as_real(L[:, c]).float()
        assert torch.equal(bits(got[:, 0]), bits(lp[:, 0])), (name, c, "re")
        assert torch.equal(bits(got[:, 1]), bits(lp[:, 1])), (name, c, "im")


@pytest.mark.parametrize("B", [5, 257, 1024])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_hole_gram_matches_numpy(cuda, B, K):
    """Synthetic logs, Re in +-10, one NaN walker and one +inf entry: S to 1e-12 of the sum of |terms| (the
    bound of test_gpu_spin_square.py for the same kind of reduction), nvalid = B - 2, two calls the same
    bits, a shift rescales S[c][c'] by exp(-shift_c - shift_c')."""
    rng = np.random.default_rng(100 * B + K)
    L = rng.uniform(-10, 10, (B, K)) + 1j * rng.uniform(-math.pi, math.pi, (B, K))
    L[1, K // 2] = complex(math.nan, 0.3)
    L[B - 2, K - 1] = complex(math.inf, 0.0)
    Ld = torch.tensor(L, device=cuda)
    S, nvalid = hole_gram(Ld)
    S_ref, mag, n_ref = HR.gram(L)
    assert nvalid == n_ref == B - 2
    err = np.abs(S.cpu().numpy() - S_ref) / mag
    print(f"B = {B} K = {K}: gram {err.max():.2e} of the sum of |terms|")
    assert err.max() < 1e-12
    S2, nvalid2 = hole_gram(Ld)
    assert nvalid2 == nvalid and torch.equal(torch.view_as_real(S).cpu().view(torch.int64),
                                             torch.view_as_real(S2).cpu().view(torch.int64))
    shift = rng.uniform(-2, 2, K)
    S3, nvalid3 = hole_gram(Ld, torch.tensor(shift))
    want = S.cpu().numpy() * np.exp(-np.add.outer(shift, shift))
    assert nvalid3 == nvalid
    assert (np.abs(S3.cpu().numpy() - want) / (mag * np.exp(-np.add.outer(shift, shift)))).max() < 1e-12


def test_identical_configurations_overlap_fully(cuda):
    """K = 4 copies of one configuration: every entry of O is 1 to 1e-12."""
    system, _, configs = HR.CASES["pfaffian6-pairings"]
    x = torch.tensor(HR.case_walkers("pfaffian6-pairings"), device=cuda)
    L = hole_logs(x, table_of(system, [configs[1]] * 4))
    S, nvalid = hole_gram(L)
    O = H.overlap_matrix(S)
    assert nvalid == x.shape[0] and (O - 1).abs().max() < 1e-12


@pytest.mark.parametrize("N,p", [(6, 1), (4, 2)])
def test_coincident_groups_are_an_abelian_hole(cuda, N, p):
    """A = {a}, B = {b} at one point against one Abelian hole there (test_quasihole_host.py's identity):
    the ratio is 2^(N/2) on every walker."""
    flux, pt = 2 * p * (N - 1), (1.3, 0.6)
    system = dict(nspins=(N, 0), flux=flux, base="pfaffian", cf_flux=p)
    x = torch.tensor(HR.uniform(64, N, seed=N), device=cuda)
    pair = hole_logs(x, table_of(system, [dict(holes=(pt, pt), pairing=((0,), (1,)))]))[:, 0]
    abel = hole_logs(x, table_of(system, [dict(holes=(pt,))]))[:, 0]
    ratio = torch.exp(pair - abel).cpu()
    err = (ratio - 2.0 ** (N / 2)).abs().max().item() / 2.0 ** (N / 2)
    print(f"N = {N} p = {p}: ratio off 2^(N/2) by {err:.1e}")
    assert err < 1e-10  # the host test's bound for the same identity


RESTATEMENT_LAMBDA_MIN = 3.0e-16  # |lambda_min / lambda_max| of the restatement on the same 257 walkers


def test_three_pairings_span_two_dimensions(cuda):
    """The three pairings of four Moore-Read holes, N = 6, B = 257 uniform walkers: the normalised 3 x 3 Gram
    matrix has one vanishing eigenvalue on any set of walkers.  The restatement gives lambda_min / lambda_max
    = 3.0e-16 on these walkers (and lambda_mid / lambda_max = 0.624); the bound is 10 x that."""
    x, L, L_ref = case_logs("pfaffian6-pairings", cuda)
    ev_ref = HR.normalised_spectrum(HR.gram(L_ref)[0])
    S, nvalid = hole_gram(L.to(cuda))
    ev = HR.normalised_spectrum(S.cpu().numpy())
    print(f"pairings: lambda {ev}, min / max {ev[0] / ev[2]:.2e} (restatement {ev_ref[0] / ev_ref[2]:.2e}), "
          f"mid / max {ev[1] / ev[2]:.3f}")
    assert nvalid == 257
    assert ev[1] / ev[2] > 0.05
    assert abs(ev[0] / ev[2]) < 10 * RESTATEMENT_LAMBDA_MIN


POINTS = [(1.0, 0.0), (1.0, 0.3), (1.0, 0.6)]


def laughlin4(batch, path):
    return Config.from_dict({
        "batch_size": batch, "seed": 11,
        "system": {"nspins": (4, 0), "flux": 10},
        "network": {"type": "quasihole", "halperin": {"exponents": [3, 3, 0]}, "quasihole": {"holes": [list(POINTS[0])]}},
        "mcmc": {"burn_in": 20},
        "optim": {"iterations": 2, "optimizer": "none"},
        "log": {"save_path": str(path)},
    })


def test_exact_overlaps_through_the_estimator(cuda, tmp_path):
    """Laughlin 1/3, N = 4, flux 10, one hole at (1, 0), (1, 0.3), (1, 0.6); B = 4096, 40 steps, a fixed seed:
    every entry of `overlap` within 0.01 of coherent_overlap(n = 4) (a CPU Metropolis run with a quarter of the
    batch and 24 steps was off by at most 3.9e-3; the exact entries differ from 1 by 0.08 to 0.32 and from
    their conjugates by up to 0.6), the berry_links with the exact signs."""
    train(laughlin4(4096, tmp_path))
    ckpt = sorted(tmp_path.glob("ckpt_*.npz"))[-1]
    steps = 40
    out, vals = evaluate(DeepHallAdaptor(), ESTIMATORS["hole_overlap"], ckpt, steps, burn_in=10, seed=5,
                         estimator_options={"configs": [{"holes": [list(p)]} for p in POINTS[1:]]})
    exact = torch.tensor([[H.coherent_overlap(a, b, 4) for b in POINTS] for a in POINTS], dtype=torch.complex128)
    err = (out["overlap"] - exact).abs()
    print("overlap", out["overlap"], "\nexact", exact, "\nerr", err.max().item(), " step scatter", out["overlap_err"].max().item())
    print("berry_links", out["berry_links"].tolist(), "+-", out["berry_links_err"].tolist())
    assert vals["gram"].shape == (steps, 3, 3) and out["walkers"] == steps * 4096
    assert err.max() < 0.01
    links = [cmath.phase(exact[c, c + 1].item()) for c in (0, 1)]
    assert all(abs(want) > 0.05 and got * want > 0 for got, want in zip(out["berry_links"].tolist(), links))
    assert (out["overlap"] - out["overlap"].conj().T).abs().max() < 1e-12
    assert torch.isfinite(out["overlap_err"]).all() and out["shift"].shape == (3,)


def test_berry_phase_chains_the_links(cuda, tmp_path):
    """berry_phase on the 4-step open path (1, 0) .. (1, 0.9) of the same system with B = 1024: the plumbing.
    The phase is the exact discrete -sum arg O[t, t + 1] within 0.05."""
    path = [{"holes": [[1.0, 0.3 * t]]} for t in range(4)]
    out = H.berry_phase(laughlin4(1024, tmp_path), path, steps=10, burn_in=20, seed=3)
    want = -sum(cmath.phase(H.coherent_overlap((1.0, 0.3 * t), (1.0, 0.3 * (t + 1)), 4)) for t in range(3))
    print(f"berry_phase {out['phase']:.4f} +- {out['phase_err']:.4f}, exact {want:.4f}")
    assert out["holonomy"].shape == (1, 1) and len(out["links"]) == 3
    assert abs(math.remainder(out["phase"] - want, 2 * math.pi)) < 0.05
    assert 0.0 < out["phase_err"] < 0.05
