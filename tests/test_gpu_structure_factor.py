"""Static structure factor on MI355X (csrc/sfactor.hip, netobs/observables/structure_factor.py).

* the pair sums against numpy's legval on the same float32 coordinates (tests/sf_ref.py), with the
  rows and walkers whose answer is known exactly;
* the multipoles against closed forms, against the legder route, and against the pair sums through
  the addition theorem at lmax = 64, near-pole walkers included;
* the fused reduction over walkers against the per-walker outputs, bitwise against itself, with
  invalid walkers;
* the estimator on the native trial states against exact structure factors, and on a Psiformer.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import sf_ref as SR
from deephall_amd import PRNGKey, config, make_mcmc_step, make_network
from deephall_amd.netobs import ESTIMATORS, HallSystem
from deephall_amd.netobs._native import sf_accumulate, sf_multipoles, sf_pairs
from deephall_amd.netobs.estimator import _batch_mean
from deephall_amd.netobs.observables.structure_factor import form_factor
from deephall_amd.random import Key

pytestmark = pytest.mark.gpu

SPLITS = [(2, 0), (2, 1), (1, 1), (0, 3), (6, 0), (3, 3), (20, 0), (16, 16)]

# theta = 0, float32(pi) (the nearest float32 lies 8.7e-8 past pi), 1e-6 and pi - 1e-6
SPECIAL = np.array([(0.0, 0.3), (np.pi, 1.0), (1e-6, -2.0), (np.pi - 1e-6, 0.5)], np.float32)


def pole_walkers(N, seed=5):
    """Four walkers of N electrons: electron e < 4 of walker k sits at SPECIAL[(k + e) % 4], the rest uniform."""
    x = SR.uniform(4, N, seed)
    for k in range(4):
        for e in range(min(N, 4)):
            x[k, e] = SPECIAL[(k + e) % 4]
    return x


def bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.cpu().contiguous().view(torch.int64)


# ---- 1. pair sums against numpy ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _walkers(nspins):
    return SR.uniform(1030, sum(nspins), seed=100 * nspins[0] + nspins[1])


@functools.lru_cache(maxsize=None)
def _pair_ref(nspins, B):
    """legval's T[B, 3, 65] of the first B walkers, computed once per size (B = 1 and 67 are cheap;
    lmax < 64 is a slice in L, the upward recurrence being the same at every lmax)."""
    return SR.pair_sums(_walkers(nspins)[:B], nspins[0], 64)


@pytest.mark.parametrize("B", [1, 67, 1030])
@pytest.mark.parametrize("lmax", [0, 1, 7, 64])
@pytest.mark.parametrize("nspins", SPLITS)
def test_pair_sums_match_legval(cuda, nspins, lmax, B):
    """|T - legval| <= 1e-9 absolute, a derived bound: cos gamma carries a few ulp, P_L' is at most
    L (L + 1) / 2 = 2080 at L = 64, so about 2e-12 per pair and about 1e-9 for the 496 pairs of 32
    electrons.  Worst seen on the MI355X: 5.2e-13 ((16, 16), lmax 64, B 1030); (2, 0): 1.6e-14.
    Row L = 0 is the pair counts exactly."""
    n_up, n_dn = nspins
    x = _walkers(nspins)[:B]
    T = sf_pairs(torch.tensor(x, device=cuda), n_up, lmax).cpu().numpy()
    assert T.shape == (B, 3, lmax + 1)
    want = _pair_ref(nspins, B)[:, :, :lmax + 1]
    worst = np.abs(T - want).max()
    print(f"pair sums {nspins} lmax {lmax} B {B}: max |T - legval| = {worst:.2e}")
    assert worst <= 1e-9
    counts = np.array([n_up * (n_up - 1) / 2, n_up * n_dn, n_dn * (n_dn - 1) / 2])
    assert (T[:, :, 0] == counts[None, :]).all()


# ---- 2. rows and walkers with an exact answer ----------------------------------------------------------

def test_coincident_and_antipodal_pairs(cuda):
    """Two electrons at one point: P_L(1) = 1 for every L <= 64, to 1e-12.  Two antipodal electrons:
    (-1)^L.  float32 cannot hold pi, so a float32 pair is antipodal only up to 1 + cos gamma of
    order 4e-15 (more when both angles are rounded), which P_L turns into L (L + 1) / 2 times that:
    the pair's own departure, computed in float64 from its float32 coordinates, is allowed on top
    of the 1e-12 (for the polar pair it is 8e-13 at L = 20: up to there the plain bound is asserted).
    theta = 0, float32(pi) and 1e-6 all occur."""
    f32 = np.float32
    same = [[(1.1, 0.7), (1.1, 0.7)], [(0.0, 0.3), (0.0, 2.0)], [(1e-6, -2.0), (1e-6, -2.0)],
            [(np.pi, 1.0), (np.pi, 1.0)], [(2.9, 3.1), (2.9, 3.1)]]
    anti = [[(0.0, 0.3), (np.pi, 1.0)], [(np.pi, 0.0), (0.0, 0.0)], [(1e-6, -2.0), (f32(np.pi) - f32(1e-6), f32(-2.0) + f32(np.pi))],
            [(1.1, 0.7), (f32(np.pi) - f32(1.1), f32(0.7) - f32(np.pi))], [(np.pi / 2, 0.0), (np.pi / 2, np.pi)]]
    x = np.array(same + anti, dtype=np.float32)                                   # [10, 2, 2]
    L = np.arange(65)
    cg = SR.cos_gamma(x)[:, 0, 1]
    assert (np.abs(cg[:5] - 1) < 1e-15).all() and (np.abs(cg[5:] + 1) < 1e-13).all()
    for n_up, s in ((2, 0), (1, 1), (0, 2)):  # the same pair as uu, ud, dd
        T = sf_pairs(torch.tensor(x, device=cuda), n_up, 64).cpu().numpy()
        other = [k for k in range(3) if k != s]
        assert (T[:, other] == 0).all()
        err_same = np.abs(T[:5, s] - 1.0)
        slack = 0.5 * L * (L + 1) * np.abs(1 + cg[5:, None])
        err_anti = np.abs(T[5:, s] - (-1.0) ** L)
        print(f"n_up {n_up}: coincident max |T - 1| = {err_same.max():.1e}; antipodal max |T - (-1)^L| = "
              f"{err_anti.max():.1e} (polar, L <= 20: {err_anti[:2, :21].max():.1e}), own departure up to {slack.max():.1e}")
        assert (err_same <= 1e-12).all()
        assert (err_anti <= 1e-12 + slack).all()
        assert (err_anti[:2, :21] <= 1e-12).all()  # the polar pairs, where float32(pi) alone enters


# ---- 3. multipoles ------------------------------------------------------------------------------------

def test_low_multipoles_match_closed_forms(cuda):
    """Y_00 .. Y_22 of single-electron walkers (uniform points, the poles, 1e-6 off them) to 1e-13."""
    x = np.concatenate([SR.uniform(60, 1, seed=2), pole_walkers(1)])
    th, ph = x[:, 0, 0].astype(np.float64), x[:, 0, 1].astype(np.float64)
    ct, st, e1 = np.cos(th), np.sin(th), np.exp(1j * ph)
    pi = math.pi
    want = np.stack([np.full_like(th, 0.5 / math.sqrt(pi)) + 0j,
                     math.sqrt(3 / (4 * pi)) * ct + 0j,
                     -math.sqrt(3 / (8 * pi)) * st * e1,
                     math.sqrt(5 / (16 * pi)) * (3 * ct**2 - 1) + 0j,
                     -math.sqrt(15 / (8 * pi)) * st * ct * e1,
                     math.sqrt(15 / (32 * pi)) * st**2 * e1**2], -1)
    for n_up in (1, 0):  # the electron as an up, then as a down one: the other species stays 0
        rho = sf_multipoles(torch.tensor(x, device=cuda), n_up, 2).cpu().numpy()
        assert rho.shape == (64, 2, 6)
        err = np.abs(rho[:, 1 - n_up] - want).max()
        print(f"closed forms (species {1 - n_up}): max |Y - closed form| = {err:.1e}")
        assert err <= 1e-13 and (rho[:, n_up] == 0).all()


# The legder route against the addition theorem on the test's own walkers, both on the CPU (lmax = 12):
# max |(4 pi / (2L+1)) sum_M |rho_LM|^2 - (N + 2 sum T)| = 9.8e-15 (N = 1), 3.2e-14 (N = 3),
# 6.4e-14 (N = 20).  The kernel is allowed 100 x the figure the test
# measures on its own inputs (both are O(L eps) schemes; the factor absorbs the different orderings).
LEGDER_CEILING = 1e-12  # the measured figure itself must stay near what was recorded


@pytest.mark.parametrize("nspins", [(1, 0), (2, 1), (12, 8)])
def test_multipoles_match_the_legder_route(cuda, nspins):
    n_up, N, lmax = nspins[0], sum(nspins), 12
    x = np.concatenate([SR.uniform(63, N, seed=7 + N), pole_walkers(N)])
    ref = SR.multipoles(x, n_up, lmax)
    T_ref = SR.pair_sums(x, n_up, lmax)
    delta = np.abs(SR.addition_lhs(ref.sum(1), lmax) - (N + 2 * T_ref.sum(1))).max()
    assert 0 < delta <= LEGDER_CEILING
    rho = sf_multipoles(torch.tensor(x, device=cuda), n_up, lmax).cpu().numpy()
    err = np.abs(rho - ref).max()
    print(f"legder route {nspins}: reference's own disagreement {delta:.1e}, bound {100 * delta:.1e}, "
          f"max |rho - legder| = {err:.1e}")
    assert err <= 100 * delta


@pytest.mark.parametrize("nspins", [(1, 0), (2, 1), (12, 8)])
def test_addition_theorem_ties_the_two_kernels(cuda, nspins):
    """lmax = 64: (4 pi / (2L+1)) (|rho_L0|^2 + 2 sum_{M>0} |rho_LM|^2), rho = rho^up + rho^dn, equals
    N + 2 (T_uu + T_ud + T_dd) for every walker and L to 1e-9 N (the pair-sum bound), near-pole
    walkers (sin^M theta underflowing) included.  Nothing overflows: every value is finite."""
    n_up, N, lmax = nspins[0], sum(nspins), 64
    x = np.concatenate([SR.uniform(29, N, seed=11 + N), pole_walkers(N)])
    xd = torch.tensor(x, device=cuda)
    rho = sf_multipoles(xd, n_up, lmax).cpu().numpy()
    T = sf_pairs(xd, n_up, lmax).cpu().numpy()
    assert np.isfinite(rho.view(np.float64)).all() and np.isfinite(T).all()
    res = np.abs(SR.addition_lhs(rho.sum(1), lmax) - (N + 2 * T.sum(1)))
    print(f"addition theorem {nspins}: max residual {res.max():.1e} (uniform {res[:29].max():.1e}, "
          f"near-pole {res[29:].max():.1e}); bound {1e-9 * N:.0e}")
    assert (res <= 1e-9 * N).all()
    # the M > 0 columns of an electron on a pole vanish: walker 29 of N = 1 is the electron at theta = 0
    if N == 1:
        m_pos = np.concatenate([np.arange(L * (L + 1) // 2 + 1, L * (L + 1) // 2 + L + 1) for L in range(lmax + 1)])
        assert (rho[29, 0, m_pos] == 0).all()


# ---- 4. the fused reduction ---------------------------------------------------------------------------

def _spoil(x, idx):
    """NaN / Inf into one coordinate of each walker of idx."""
    x = x.copy()
    bad = [np.nan, np.inf, -np.inf]
    for k, b in enumerate(idx):
        x[b, k % x.shape[1], k % 2] = bad[k % 3]
    return x


def _rel(got, terms, keep):
    """max |got - float64 sum of the kept terms| / sum |terms|: relative to what was added."""
    want, scale = terms[keep].sum(0), np.abs(terms[keep]).sum(0)
    return np.max(np.abs(got - want) / np.where(scale > 0, scale, 1.0))


@pytest.mark.parametrize("lmax", [7, 64])
def test_accumulate_matches_the_per_walker_sums(cuda, lmax):
    """B = 1030 (129 workgroups of 8 walkers, the last with 6), N = 6: the sums over the valid walkers of
    the per-walker outputs, to 1e-12 of the sum of the terms' magnitudes; the same bits twice and
    without the multipoles; five invalid walkers dropped exactly."""
    nspins, B = (3, 3), 1030
    x = _walkers(nspins)
    idx = [0, 7, 8, 517, 1029]  # first and last of a workgroup's range, the batch's last walker
    for label, xs, keep in (("clean", x, np.ones(B, bool)), ("spoiled", _spoil(x, idx), ~np.isin(np.arange(B), idx))):
        xd = torch.tensor(xs, device=cuda)
        T = sf_pairs(xd, 3, lmax).cpu().numpy()
        rho = sf_multipoles(xd, 3, lmax).cpu().numpy()
        assert (np.isnan(T).all(axis=(1, 2)) == ~keep).all() and np.isfinite(T[keep]).all()
        assert (np.isnan(rho.real).all(axis=(1, 2)) == ~keep).all() and (np.isnan(rho.imag).all(axis=(1, 2)) == ~keep).all()
        assert np.isfinite(rho[keep].view(np.float64)).all()
        pairs, rsum, nvalid = sf_accumulate(xd, 3, lmax)
        assert nvalid == keep.sum() == (B if label == "clean" else B - 5)
        assert pairs.shape == (3, lmax + 1) and rsum.shape == (2, SR.nlm(lmax))
        err_p = _rel(pairs.cpu().numpy(), T, keep)
        err_r = _rel(rsum.cpu().numpy(), rho, keep)
        print(f"accumulate lmax {lmax} {label}: max err / sum |terms|: pairs {err_p:.1e}, multipoles {err_r:.1e}")
        assert err_p <= 1e-12 and err_r <= 1e-12
        again = sf_accumulate(xd, 3, lmax)
        assert torch.equal(bits(again[0]), bits(pairs)) and torch.equal(bits(again[1]), bits(rsum)) and again[2] == nvalid
        only, none, nvalid0 = sf_accumulate(xd, 3, lmax, multipoles=False)  # rho_sums is a null pointer here
        assert none is None and nvalid0 == nvalid and torch.equal(bits(only), bits(pairs))


def test_accumulate_with_every_walker_invalid(cuda):
    x = SR.uniform(67, 3, seed=3)
    x[:, 1, 0] = np.nan
    x[5, 2, 1] = np.inf
    pairs, rho, nvalid = sf_accumulate(torch.tensor(x, device=cuda), 2, 9)
    assert nvalid == 0 and (pairs == 0).all() and (rho == 0).all()
    pairs, rho, nvalid = sf_accumulate(torch.tensor(x, device=cuda), 2, 9, multipoles=False)
    assert nvalid == 0 and (pairs == 0).all() and rho is None


# ---- 5. physics: the estimator on the native trial states ----------------------------------------------

def _network(kind, nspins, flux, lz=0.0, exponents=None):
    net = config.Network()
    net.type = config.NetworkType(kind)
    if exponents:
        net.halperin.exponents = exponents
    return make_network(config.System(nspins=nspins, flux=flux, lz_center=lz), net)


def _measure(cuda, model, nspins, flux, *, B=4096, steps=20, burn=40, walk_steps=40, options=None, params=None):
    """netobs.evaluate's loop without the checkpoint: burn in (tuning the all-electron move width to
    an acceptance of 0.5 .. 0.55, as training does), then steps x (walk, evaluate), then the digest."""
    N = sum(nspins)
    params = model.init(PRNGKey(0), device=cuda) if params is None else params
    x = torch.tensor(SR.uniform(B, N, seed=17), device=cuda)
    walk = make_mcmc_step(model, batch_per_device=B, steps=walk_steps)
    key, width = Key(29), 0.3
    for _ in range(burn):
        x, pmove = walk(params, x, key, width)
        key = key.advance(walk_steps)
        width *= 1.1 if float(pmove) > 0.55 else (1 / 1.1 if float(pmove) < 0.5 else 1.0)
    system = HallSystem(spins=list(nspins), flux=flux)
    est = ESTIMATORS["structure_factor"](None, system, options, {})
    values, state = est.empty_val_state(steps)
    for i in range(steps):
        x, pmove = walk(params, x, key, width)
        key = key.advance(walk_steps)
        vals, state = est.evaluate(i, params, None, x, system, state, None)
        for name, v in vals.items():
            values[name][i] = _batch_mean(v).to(values[name].dtype)
    out = est.digest(values, state)
    assert state["walkers"] == steps * B
    print(f"  width {width:.2f}, acceptance {float(pmove):.2f}")
    return out


def _close(out, key, L, exact, label):
    """|estimate - exact| <= 5 err with err <= 0.02, the estimator's own error bar at that L."""
    got, err = out[key][L].item(), out["structure_factor_err"][L].item()
    print(f"  {label} {key}({L}) = {got:.5f}, exact {exact:.5f}, err {err:.5f}: {abs(got - exact) / err:.2f} err")
    assert err <= 0.02 and abs(got - exact) <= 5 * err


def test_filled_level(cuda):
    """nspins (5, 0) at flux 4, nu = 1.  The Laughlin kernel takes at least one vortex pair per
    electron, so the Vandermonde state comes from the Halperin kernel as (1, 1, 0) with no down
    electron: the same wavefunction.  S(L) = 1 - F_L for L = 1..6 (1 at L = 5, 6) and the
    guiding-centre structure factor is 0."""
    out = _measure(cuda, _network("halperin", (5, 0), 4, exponents=(1, 1, 0)), (5, 0), 4)
    ff = form_factor(4, 6)
    assert out["structure_factor"].shape == (11,) and out["structure_factor"][0].item() == 5.0
    for L in range(1, 7):
        _close(out, "structure_factor", L, ff[L].item(), "filled")
        _close(out, "guiding_center", L, 0.0, "filled")
    assert ff[5].item() == 1.0 and ff[6].item() == 1.0


def test_laughlin_third(cuda):
    """nspins (4, 0) at flux 9: an L_tot = 0 lowest-level state, S(1) = 1 / (Q + 1) = 2 / 11, S(0) = 4
    exactly; uniform, so the connected part agrees with S at L >= 1 within error."""
    out = _measure(cuda, _network("laughlin", (4, 0), 9), (4, 0), 9)
    assert out["structure_factor"][0].item() == 4.0
    _close(out, "structure_factor", 1, 2 / 11, "laughlin 1/3")
    _close(out, "guiding_center", 1, 0.0, "laughlin 1/3")
    for L in range(1, 9):
        _close(out, "connected", L, out["structure_factor"][L].item(), "laughlin 1/3")


def test_laughlin_quasihole(cuda):
    """nspins (4, 0) at flux 10 with the hole on a pole (excitation_lz = Q1 = 2): L_tot = N / 2 = 2, so
    the guiding-centre S(1) = L_tot (L_tot + 1) / (N (Q + 1)^2) = 6 / (4 36).  Not uniform: <sum cos th>
    = L_z / (Q + 1) = 1 / 3 in magnitude, so S - S_c = (4 pi / (3 N)) (3 / 4 pi) / 9 = 1 / 36 at L = 1, more
    than 5 err; at L = 0 the connected part removes N."""
    out = _measure(cuda, _network("laughlin", (4, 0), 10, lz=2.0), (4, 0), 10)
    _close(out, "guiding_center", 1, 6 / (4 * 36), "quasihole")
    diff = out["structure_factor"] - out["connected"]
    err = out["structure_factor_err"]
    print("  quasihole S - S_c:", [f"{d:.4f}" for d in diff[:6].tolist()], "err", [f"{e:.4f}" for e in err[:6].tolist()])
    assert abs(diff[0].item() - 4.0) <= 1e-12  # rho_00 = N / sqrt(4 pi) on every walker
    assert err[1].item() <= 0.02 and diff[1].item() > 5 * err[1].item()
    assert abs(diff[1].item() - 1 / 36) <= 5 * err[1].item()


def test_halperin_111(cuda):
    """(1, 1, 1) at nspins (2, 2), flux 3: the orbital wavefunction of the filled level, so the total
    S(L) = 1 - F_L; S = S_uu + S_dd + 2 S_ud to 1e-12; S_uu = S_dd within error."""
    out = _measure(cuda, _network("halperin", (2, 2), 3, exponents=(1, 1, 1)), (2, 2), 3)
    ff = form_factor(3, 8)
    for L in range(1, 6):
        _close(out, "structure_factor", L, ff[L].item(), "(1,1,1)")
    uu, ud, dd = out["partial"]
    assert (out["structure_factor"] - (uu + dd + 2 * ud)).abs().max().item() <= 1e-12
    err = out["structure_factor_err"]
    print("  S_uu - S_dd:", [f"{d:.4f}" for d in (uu - dd)[:6].tolist()], "err", [f"{e:.4f}" for e in err[:6].tolist()])
    assert ((uu - dd).abs()[1:6] <= 5 * err[1:6]).all() and (err[1:6] <= 0.02).all()
    assert uu[0].item() == dd[0].item() == 1.0 and ud[0].item() == 1.0  # 1/2 + (2/4) 1, 4/4


# ---- 6. any network ----------------------------------------------------------------------------------

def test_psiformer_runs(cuda):
    """A randomly initialised Psiformer, nspins (2, 1), flux 3, 256 walkers: the estimator needs the walk
    only, and S(0) = N."""
    net = config.Network()
    net.psiformer.num_layers = 2
    model = make_network(config.System(nspins=(2, 1), flux=3), net)
    params = model.init(PRNGKey(7), device=cuda)
    out = _measure(cuda, model, (2, 1), 3, B=256, steps=3, burn=2, walk_steps=5, params=params)
    assert out["structure_factor"].shape == (9,) and out["structure_factor"][0].item() == 3.0
    assert torch.isfinite(out["structure_factor"]).all() and torch.isfinite(out["connected"]).all()
    assert out["multipole_mean"].shape == (2, 45)
