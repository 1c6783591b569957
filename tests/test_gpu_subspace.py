"""The subspace estimator on MI355X (csrc/subspace.hip, netobs/observables/subspace.py, netobs/subspace.py).

(a) dh_subspace_accumulate on synthetic float32 inputs against a numpy complex128 evaluation of the same
    three formulas: every entry of S, H and T, its dropped walkers, its bits, its shift;
(b) the estimator's step values against the numpy reduction of the per-state local energies (plumbing);
(c) one state written three ways: unit overlaps, rank 1 and the energy of state 0;
(d) zero variance without interaction: H = c S within the rounding of the inputs, by Cauchy-Schwarz;
(e) a Psiformer as state 0.
The host side (solver, options, argument checks) is in test_subspace_host.py.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from deephall_amd import Config, make_network
from deephall_amd.hamiltonian import _run_local_energy
from deephall_amd.mcmc import make_mcmc_step
from deephall_amd.netobs import ESTIMATORS, HallSystem, subspace as SS
from deephall_amd.netobs._native import subspace_sums
from deephall_amd.random import PRNGKey
from helpers import make_walkers

pytestmark = pytest.mark.gpu


# ---- (a) the kernel --------------------------------------------------------------------------------

def synthetic(B, K, seed):
    """logs, e_l, ke [K, B, 2] float32: |Re log| <= 30, phases in (-pi, pi), E and KE of order 10."""
    rng = np.random.default_rng(seed)
    logs = np.stack([rng.uniform(-30, 30, (K, B)), rng.uniform(-math.pi, math.pi, (K, B))], axis=-1)
    e_l = rng.normal(scale=10.0, size=(K, B, 2))
    ke = rng.normal(scale=10.0, size=(K, B, 2))
    return logs.astype(np.float32), e_l.astype(np.float32), ke.astype(np.float32)


def reference(logs, e_l, ke, shift=None):
    """(out [3, K, K] complex128, mag [3, K, K]: the sums of |term|, nvalid) in numpy float64 from the same
    float32 inputs; a walker is kept when its 6 K inputs and its K ratios are finite."""
    K, B, _ = logs.shape
    shift = np.zeros(K) if shift is None else np.asarray(shift, dtype=np.float64)
    L = logs[..., 0].astype(np.float64) + 1j * logs[..., 1].astype(np.float64)
    E = e_l[..., 0].astype(np.float64) + 1j * e_l[..., 1].astype(np.float64)
    T = ke[..., 0].astype(np.float64) + 1j * ke[..., 1].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.exp(L - L[:1] - shift[:, None])
    keep = np.isfinite(logs).all(axis=(0, 2)) & np.isfinite(e_l).all(axis=(0, 2)) & np.isfinite(ke).all(axis=(0, 2))
    keep &= np.isfinite(r.real).all(axis=0) & np.isfinite(r.imag).all(axis=0)
    r, E, T = r[:, keep], E[:, keep], T[:, keep]
    w = r.conj()[:, None, :] * r[None, :, :]  # [c, c', b]
    terms = np.stack([w, w * E[None, :, :], w * T[None, :, :]])  # the operator on the ket c'
    return terms.sum(axis=-1), np.abs(terms).sum(axis=-1), int(keep.sum())


def run(logs, e_l, ke, cuda, shift=None):
    out, nvalid = subspace_sums(*(torch.tensor(a, device=cuda) for a in (logs, e_l, ke)),
                                None if shift is None else torch.tensor(shift))
    return out, nvalid


def bits(t):
    return torch.view_as_real(t).cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("B,K", [(1, 1), (257, 3), (1000, 32)])
def test_sums_match_float64(cuda, B, K):
    """Every entry of S, H and T within 1e-12 of the sum of |term|: double sums of identical inputs in another
    order.  H and T are compared entry by entry as complex, non-Hermitian matrices: conj on the bra, E from the
    ket.  Two calls give the same bits, and a shift rescales entry [c][c'] by exp(-shift_c - shift_c')."""
    logs, e_l, ke = synthetic(B, K, seed=1000 * K + B)
    want, mag, n_ref = reference(logs, e_l, ke)
    out, nvalid = run(logs, e_l, ke, cuda)
    assert out.shape == (3, K, K) and out.dtype == torch.complex128 and nvalid == n_ref == B
    got = out.cpu().numpy()
    err = np.abs(got - want) / mag
    print(f"B = {B} K = {K}: S {err[0].max():.2e} H {err[1].max():.2e} T {err[2].max():.2e} of the sum of |terms|")
    assert err.max() < 1e-12
    if K > 1:  # the reference itself tells bra from ket and E_c from E_c': the transposes are far off
        assert (np.abs(want[1] - want[1].conj().T) / mag[1]).max() > 1e-3
        assert (np.abs(got[1] - want[1].conj().T) / mag[1]).max() > 1e-3
    out2, nvalid2 = run(logs, e_l, ke, cuda)
    assert nvalid2 == nvalid and torch.equal(bits(out), bits(out2))
    shift = np.random.default_rng(B + K).uniform(-2, 2, K)
    out3, nvalid3 = run(logs, e_l, ke, cuda, shift)
    scale = np.exp(-np.add.outer(shift, shift))[None]
    assert nvalid3 == nvalid
    assert (np.abs(out3.cpu().numpy() - got * scale) / (mag * scale)).max() < 1e-12


@pytest.mark.parametrize("B,K", [(257, 3), (1000, 32)])
def test_invalid_walkers_are_dropped_whole(cuda, B, K):
    """A NaN log in walker 7, an infinite E in walker 200 and a log whose ratio overflows in walker 100:
    nvalid = B - 3 and the matrices are the reference's over the other walkers, all of which the float64
    reference keeps (checked here on the host: |Re log| <= 30 puts every other ratio below e^60)."""
    logs, e_l, ke = synthetic(B, K, seed=7 * K + B)
    clean = reference(logs, e_l, ke)
    assert clean[2] == B
    logs[K - 1, 7, 1] = math.nan
    e_l[K // 2, 200, 0] = math.inf
    logs[1, 100, 0] = 800.0  # finite in float32, exp(800 - 30) is not in float64
    want, mag, n_ref = reference(logs, e_l, ke)
    assert n_ref == B - 3
    keep = np.ones(B, dtype=bool)
    keep[[7, 100, 200]] = False
    rest = reference(logs[:, keep], e_l[:, keep], ke[:, keep])
    assert rest[2] == B - 3 and np.array_equal(rest[0], want)  # the reference drops exactly these three
    out, nvalid = run(logs, e_l, ke, cuda)
    assert nvalid == B - 3
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want) / mag
    print(f"B = {B} K = {K}: {err.max():.2e} of the sum of |terms| with three walkers dropped")
    assert err.max() < 1e-12
    # no valid walker: zero sums and nvalid = 0
    out0, nvalid0 = run(np.full_like(logs, math.nan), e_l, ke, cuda)
    assert nvalid0 == 0 and (out0.cpu().numpy() == 0).all()


# ---- the estimator ---------------------------------------------------------------------------------

NSPINS, FLUX, B_WALK = (4, 0), 9, 257  # nu = 1/3 with Q1 = 3/2
GROUND = [(0, -1.5), (0, -0.5), (0, 0.5), (0, 1.5)]


def exciton(m_h, M=2):
    """A hole at (0, m_h) and a particle at (1, m_h + M) on the filled level 0."""
    return [list(o) for o in GROUND if o != (0, m_h)] + [[1, m_h + M]]


EXCITONS = [{"type": "jain", "jain": {"occupation": exciton(m_h)}} for m_h in (-1.5, -0.5, 0.5)]


class _Adaptor:
    def __init__(self, cfg):
        self.cfg, self.model = cfg, make_network(cfg.system, cfg.network)


def setup(cuda, network, options, strength=1.0, seed=5):
    """(estimator, params, x): the estimator on an adaptor of ``network`` and B_WALK walkers after a short
    native walk of state 0."""
    cfg = Config.from_dict({"batch_size": B_WALK, "system": {"nspins": NSPINS, "flux": FLUX,
                                                            "interaction_strength": strength}, "network": network})
    adaptor = _Adaptor(cfg)
    est = ESTIMATORS["subspace"](adaptor, HallSystem(list(NSPINS), flux=FLUX), options, {})
    params = adaptor.model.init(PRNGKey(seed), device=cuda)
    x = torch.tensor(make_walkers(B_WALK, sum(NSPINS), seed=seed), device=cuda).contiguous()
    x, pmove = make_mcmc_step(adaptor.model, batch_per_device=B_WALK, steps=30)(params, x, PRNGKey(seed + 1), 0.5)
    assert torch.isfinite(x).all() and 0.0 < float(pmove) <= 1.0
    return est, params, x


def inputs(est, params, x):
    """(L, E, T) [K, B] complex128 in numpy, and the raw float32 (logs, e_l) [K, B, 2]: dh_local_energy of
    every state of the estimator, called directly."""
    logs, e_ls, kes = [], [], []
    for c, net in enumerate(est.networks):
        e_l, obs, _ = _run_local_energy(net, params if c == 0 else {}, x, external=True)
        logs.append(obs[:, 6:8].cpu().numpy())
        e_ls.append(e_l.cpu().numpy())
        kes.append(obs[:, 0:2].cpu().numpy())
    logs, e_ls, kes = np.stack(logs), np.stack(e_ls), np.stack(kes)
    cplx = lambda a: a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)  # noqa: E731
    return cplx(logs), cplx(e_ls), cplx(kes), logs, e_ls


def one_step(est, params, x):
    values, state = est.empty_val_state(1)
    v, state = est.evaluate(0, params, None, x, None, state, None)
    for k in values:
        values[k][0] = v[k][0]
    return v, values, state


def test_plumbing(cuda):
    """The Jain ground occupation and the three M = 2 exciton determinants: one step's gram, hamiltonian and
    kinetic are the complex128 numpy reduction of the per-state dh_local_energy outputs to 1e-12 of the mean
    |term| of each entry (what a double sum in another order can differ by): the state order, the obs
    columns, the shift and the division by nvalid."""
    est, params, x = setup(cuda, {"type": "jain", "jain": {"occupation": GROUND}}, {"states": EXCITONS})
    assert est.K == 4
    L, E, T, _, _ = inputs(est, params, x)
    assert np.isfinite(L).all() and np.isfinite(E).all() and np.isfinite(T).all()
    shift = (L - L[:1]).real.mean(axis=1)
    r = np.exp(L - L[:1] - shift[:, None])
    w = r.conj()[:, None, :] * r[None, :, :]
    v, _, state = one_step(est, params, x)
    assert v["walkers"].tolist() == [float(B_WALK)] and state["shift"].shape == (4,)
    assert np.abs(state["shift"].numpy() - shift).max() < 1e-12 and state["shift"][0] == 0
    for name, terms in (("gram", w), ("hamiltonian", w * E[None]), ("kinetic", w * T[None])):
        got = v[name]
        assert got.shape == (1, 4, 4) and got.dtype == torch.complex128
        err = np.abs(got[0].numpy() - terms.mean(axis=-1)) / np.abs(terms).mean(axis=-1)
        print(f"{name}: {err.max():.2e} of the mean |term|")
        assert err.max() < 1e-12, name
    # the shift stays: a second step on other walkers is in the same units
    shift0 = state["shift"].clone()
    est.evaluate(1, params, None, x.flip(0).contiguous(), None, state, None)
    assert torch.equal(state["shift"], shift0)


def test_one_state_three_ways(cuda):
    """Laughlin, Jain with the four level-0 orbitals and Halperin (3, 3, 0) on nspins (4, 0) differ by a
    constant factor.  With delta_c = 2^-24 max |value| of state c's two log columns on these walkers (the
    float32 rounding of the inputs), every |overlap[c][c']| is within 2 (delta_c + delta_c') of 1, the rank is
    1 at rank_tol 1e-4, and the one energy is the walker mean of state 0's E_L within the largest of those
    bounds times max |E_L|."""
    est, params, x = setup(cuda, {"type": "laughlin"}, {"rank_tol": 1e-4, "states": [
        {"type": "jain", "jain": {"occupation": [list(o) for o in GROUND]}},
        {"type": "halperin", "halperin": {"exponents": [3, 3, 0]}}]})
    L, E, _, logs, _ = inputs(est, params, x)
    delta = 2.0 ** -24 * np.abs(logs).max(axis=(1, 2))
    bound = 2 * np.add.outer(delta, delta)
    _, values, state = one_step(est, params, x)
    out = est.digest(values, state)
    dev = np.abs(np.abs(out["overlap"].numpy()) - 1)
    print(f"delta {delta}, ||overlap| - 1| max {dev.max():.2e} (bound {bound.min():.2e}), rank {out['rank']}")
    assert (dev <= bound).all()
    assert out["rank"] == 1 and out["energies"].shape == (1,)
    e0 = E[0].mean().real
    print(f"energy {out['energies'][0].item():.9f}, <E_L> of state 0 {e0:.9f}, max |E_L| {np.abs(E).max():.3f}")
    assert abs(out["energies"][0].item() - e0) <= bound.max() * np.abs(E).max()
    assert math.isnan(out["energies_err"][0].item())  # one step


def test_zero_variance_without_interaction(cuda):
    """interaction_strength = 0 and the four Jain states of test_plumbing: every state lies in the lowest
    Landau level, so E_L is one constant c on every walker.  With eps = max |E_L - c| over states and walkers,
    read from the inputs, |H[c][c'] - c S[c][c']| <= eps sqrt(S[c][c] S[c'][c']) (Cauchy-Schwarz), and every
    energy is within eps / (the smallest kept eigenvalue of the scaled S) of c."""
    est, params, x = setup(cuda, {"type": "jain", "jain": {"occupation": GROUND}}, {"states": EXCITONS}, strength=0.0)
    _, E, T, _, _ = inputs(est, params, x)
    c = float(T[0].real.mean())  # state 0's kinetic energy, obs column 0
    assert abs(c - sum(NSPINS) / 2) < 1e-3  # N / 2 in units of the cyclotron energy
    eps = np.abs(E - c).max()
    print(f"c = {c:.9f}, eps = {eps:.2e}")
    assert eps < 1e-3
    _, values, state = one_step(est, params, x)
    out = est.digest(values, state)
    S, H = out["gram"].numpy(), out["hamiltonian"].numpy()
    d = np.sqrt(np.diag(S).real)
    lhs, rhs = np.abs(H - c * S), eps * np.outer(d, d)
    print(f"|H - c S| / (eps sqrt(S S)) max {(lhs / rhs).max():.3f}")
    assert (lhs <= rhs).all()
    Sh = (S + S.conj().T) / 2 / np.outer(d, d)
    w = np.linalg.eigvalsh(Sh)
    kept = w[w > est.rank_tol * w[-1]]
    assert out["rank"] == len(kept) == 4
    off = np.abs(out["energies"].numpy() - c)
    print(f"eigenvalues of the scaled S {w}, |E - c| max {off.max():.2e} (bound {eps / kept.min():.2e})")
    assert (off <= eps / kept.min()).all()
    # V = H - T: H is c S within eps and T within eps_t, the same inequality with KE for E_L
    eps_t = np.abs(T - c).max()
    assert (np.abs(out["potential"].numpy()) <= (eps + eps_t) * np.outer(d, d)).all()


def test_psiformer_as_state_0(cuda):
    """A freshly initialised one-layer Psiformer with states = [laughlin]: the step runs, the rank is 2, and
    hamiltonian[0][0] / gram[0][0] is the walker mean of the network's own E_L, called directly, to 1e-12."""
    network = {"type": "psiformer", "psiformer": {"num_layers": 1, "num_heads": 2, "heads_dim": 8, "determinants": 1}}
    est, params, x = setup(cuda, network, {"states": [{"type": "laughlin"}]})
    e_l, _ = _run_local_energy(est.networks[0], params, x)
    e = e_l.cpu().numpy().astype(np.float64)
    assert np.isfinite(e).all()
    want = complex(e[:, 0].mean(), e[:, 1].mean())
    v, values, state = one_step(est, params, x)
    assert v["walkers"].tolist() == [float(B_WALK)]
    S, H = v["gram"][0].numpy(), v["hamiltonian"][0].numpy()
    got = H[0, 0] / S[0, 0]
    print(f"H00 / S00 = {got}, <E_L> = {want}, off by {abs(got - want) / abs(want):.2e}")
    assert S[0, 0] == 1.0 and abs(got - want) <= 1e-12 * abs(want)
    out = est.digest(values, state)
    assert out["rank"] == 2 and out["energies"].shape == (2,) and torch.isfinite(out["energies"]).all()
    assert out["energies"][0].item() <= want.real + 1e-9 * abs(want)  # the span holds state 0
    sol = SS.solve(S, H)
    assert np.array_equal(sol.energies, out["energies"].numpy())
