"""Total-spin estimator on MI355X (csrc/spin.hip, netobs/observables/spin_square.py).

* the exchanged rows against the numpy restatement (tests/spin_ref.py), exactly: copied floats;
* the ratios and the reduction on synthetic float32 logs against the restatement in float64,
  bitwise against themselves, and bitwise between one window of all pairs and one per pair;
* zero variance: S^2_loc = S (S + 1) on every walker of the Halperin kernel's eigenstates and of
  the Laughlin kernel, within what storing the logs in float32 allows;
* a random Psiformer against the restatement fed by the float64 oracle;
* the driver on a checkpoint.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import spin_ref as SR
from deephall_amd import Config, config, make_network, train
from deephall_amd.netobs import ESTIMATORS, DeepHallAdaptor, evaluate
from deephall_amd.netobs._native import spin_exchange, spin_ratios, spin_reduce, spin_square_sums, spin_workspace
from deephall_amd.networks import HalperinCallable
from helpers import make_params, make_walkers, oracle_config, to_device_params
from oracle import reference as R
from test_gpu_parity import build

pytestmark = pytest.mark.gpu


def uniform(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.arccos(rng.uniform(-1, 1, (B, N))), rng.uniform(-np.pi, np.pi, (B, N))], -1).astype(np.float32)


def bits(t):
    return torch.view_as_real(t).cpu().contiguous().view(torch.int64)


# B = 257 crosses a 256-thread block; (10, 10) has the most pairs; (1, 1) has one
@pytest.mark.parametrize("nspins,B", [((3, 2), 257), ((10, 10), 5), ((1, 1), 3)])
def test_exchange_rows_match_restatement(cuda, nspins, B):
    N, P = sum(nspins), nspins[0] * nspins[1]
    x = uniform(B, N, seed=B)
    want = SR.exchange_rows(x, nspins)
    xd = torch.tensor(x, device=cuda)
    got = spin_exchange(xd, nspins)
    assert got.shape == (P, B, N, 2)
    assert torch.equal(got.cpu(), torch.tensor(want))
    # windows of pairs are slices of the full call
    for p0, p1 in ((0, 1), (P - 1, P), (P // 3, max(P // 3 + 1, 2 * P // 3))):
        assert torch.equal(spin_exchange(xd, nspins, p0, p1).cpu(), torch.tensor(want[p0:p1])), (p0, p1)


def _reduce(lp, lps, nspins, windows):
    """ratios by the given pair windows, then the reduction: (s2, pairs, total, nvalid)."""
    B = lp.shape[0]
    ws = spin_workspace(B, nspins, lp.device)
    ws.fill_(float("nan"))  # whatever a window leaves unwritten would show
    for p0, p1 in windows:
        spin_ratios(lp, lps[p0 * B:p1 * B], nspins, p0, p1, ws)
    return spin_reduce(lp, nspins, ws)


@pytest.mark.parametrize("B", [5, 257, 1024])
def test_reduce_matches_restatement_and_is_deterministic(cuda, B):
    """Synthetic float32 logs, real parts in +-10: the device sums differ from numpy's float64 sums
    in the order of summation (and the last bits of exp / sincos) only.  One NaN walker and one
    +inf row are dropped."""
    nspins = (3, 2)
    P = 6
    rng = np.random.default_rng(B)
    lp = np.stack([rng.uniform(-10, 10, B), rng.uniform(-np.pi, np.pi, B)], -1).astype(np.float32)
    lps = np.stack([rng.uniform(-10, 10, (P, B)), rng.uniform(-np.pi, np.pi, (P, B))], -1).astype(np.float32)
    lp[1, 0] = np.nan
    lps[4, 3, 0] = np.inf
    lpd, lpsd = torch.tensor(lp, device=cuda), torch.tensor(lps.reshape(P * B, 2), device=cuda)
    one = [(0, P)]
    s2, pairs, total, nvalid = _reduce(lpd, lpsd, nspins, one)
    s2_ref, pairs_ref, total_ref, nvalid_ref = SR.spin_square(lp, lps, nspins)
    assert nvalid == nvalid_ref == B - 2
    got = s2.cpu().numpy()
    assert np.isnan(got[[1, 3]].real).all() and np.isnan(got[[1, 3]].imag).all()
    keep = np.isfinite(s2_ref.real)
    assert keep.sum() == B - 2
    mags = np.abs(SR.ratios(lp, lps))  # [P, B]
    per_walker = np.nansum(mags, 0) + 2.75
    err_w = np.max(np.abs(got[keep] - s2_ref[keep]) / per_walker[keep])
    mag_p = np.where(keep[None, :], mags, 0).sum(1).reshape(3, 2)
    err_p = np.max(np.abs(pairs.cpu().numpy() - pairs_ref) / mag_p)
    err_t = abs(total.item() - total_ref) / per_walker[keep].sum()
    print(f"spin reduce B={B}: max err / sum|terms|: walkers {err_w:.1e} pairs {err_p:.1e} total {err_t:.1e}")
    assert err_w <= 1e-12 and err_p <= 1e-12 and err_t <= 1e-12
    # two calls, and one pair per window (in any order), give the same bits
    again = _reduce(lpd, lpsd, nspins, one)
    each = _reduce(lpd, lpsd, nspins, [(p, p + 1) for p in (3, 0, 5, 1, 4, 2)])
    for other in (again, each):
        assert torch.equal(bits(other[0]), bits(s2)) and torch.equal(bits(other[1]), bits(pairs))
        assert torch.equal(bits(other[2]), bits(total)) and other[3] == nvalid


def test_one_species_empty(cuda):
    """n_dn = 0: no pair, no exchange, S^2 = (N / 2)(N / 2 + 1) exactly on every valid walker."""
    nspins, B = (3, 0), 70
    lp = torch.zeros(B, 2, device=cuda)
    lp[7, 1] = float("nan")
    s2, pairs, total, nvalid = _reduce(lp, None, nspins, [])
    assert nvalid == B - 1 and pairs.shape == (3, 0)
    want = torch.full((B,), 3.75, dtype=torch.complex128)
    keep = torch.arange(B) != 7
    assert torch.equal(s2.cpu()[keep], want[keep]) and torch.isnan(s2.cpu()[7].real)
    assert total.item() == 3.75 * (B - 1)
    calls = []

    def apply(rows):
        calls.append(rows.shape)
        return torch.zeros(rows.shape[0], dtype=torch.complex64, device=rows.device)

    s2, _, total, nvalid = spin_square_sums(apply, torch.tensor(uniform(B, 3, 1), device=cuda), nspins)
    assert len(calls) == 1 and nvalid == B and total.item() == 3.75 * B  # no second wavefunction call


def _halperin(nspins, expo, flux):
    net = config.Network()
    net.type = config.NetworkType.halperin
    net.halperin.exponents = expo
    return make_network(config.System(nspins=nspins, flux=flux), net)


def _laughlin(nspins, flux):
    net = config.Network()
    net.type = config.NetworkType.laughlin
    return make_network(config.System(nspins=nspins, flux=flux), net)


def _zero_variance(cuda, model, ref, nspins, want, label):
    """Every walker of 512: |S^2_loc - S (S + 1)| within what float32 logs allow (spin_ref.float32_log_bound),
    the ratios and logs of the bound from ``ref`` (HalperinCallable, float64), not from the kernel."""
    x = make_walkers(512, sum(nspins), seed=31, margin=0.05)
    fn = lambda rows: ref(None, torch.as_tensor(rows, dtype=torch.float64)).numpy()  # noqa: E731
    s2_ref, _, _, nvalid_ref, lp64, lps64 = SR.spin_square_of(fn, x, nspins)
    bound = SR.float32_log_bound(lp64, lps64)
    # the reference itself: its float64 rounding is 2^-29 of what float32 logs do, times the conditioning of w
    assert nvalid_ref == 512 and (np.abs(s2_ref - want) <= 1e-3 * bound).all()
    params = model.init(0, device=cuda)
    s2, pairs, total, nvalid = spin_square_sums(lambda rows: model.apply(params, rows), torch.tensor(x, device=cuda),
                                                nspins)
    assert nvalid == 512
    err = np.abs(s2.cpu().numpy() - want)
    print(f"{label}: max |S^2_loc - {want}| = {err.max():.2e}, max err / bound = {np.max(err / bound):.3f}, "
          f"bound min {bound.min():.1e} median {np.median(bound):.1e} max {bound.max():.1e}")
    assert (err <= bound).all()
    assert abs(total.item() / nvalid - want) <= bound.mean()
    c0 = ((nspins[0] - nspins[1]) / 2) ** 2 + sum(nspins) / 2
    assert abs(pairs.sum().item() / nvalid - (c0 - want)) <= bound.mean()


@pytest.mark.parametrize("nspins,expo,flux,want", [((2, 2), (3, 3, 2), 7, 0.0), ((3, 3), (3, 3, 2), 12, 0.0),
                                                  ((2, 2), (1, 1, 1), 3, 6.0), ((4, 2), (1, 3, 0), 3, 2.0)])
def test_zero_variance_on_the_halperin_kernel(cuda, nspins, expo, flux, want):
    _zero_variance(cuda, _halperin(nspins, expo, flux), HalperinCallable(nspins, flux, expo), nspins, want,
                   f"halperin {nspins} {expo}")


def test_zero_variance_on_the_laughlin_kernel(cuda):
    """A kernel that predates the estimator: Laughlin at nspins (2,1), flux 6 is fully polarised in
    every component, S = 3/2."""
    _zero_variance(cuda, _laughlin((2, 1), 6), HalperinCallable((2, 1), 6, (3, 3, 3)), (2, 1), 3.75, "laughlin (2,1)")


def test_psiformer_matches_oracle(cuda):
    """(2,2), flux 7, random parameters, 64 walkers: S^2_loc against the restatement fed the oracle's
    float64 logs."""
    ocfg = oracle_config("MIX", flux=7)
    _, model = build(ocfg)
    p64 = make_params(ocfg, seed=11)
    params = to_device_params(p64)
    x = make_walkers(64, 4, seed=6)
    logpsi64 = lambda rows: R.batch_logpsi(p64, ocfg, torch.tensor(rows, dtype=torch.float64)).numpy()  # noqa: E731
    s2_ref, pairs_ref, total_ref, nvalid_ref, _, _ = SR.spin_square_of(logpsi64, x, (2, 2))
    s2, pairs, total, nvalid = spin_square_sums(lambda r: model.apply(params, r), torch.tensor(x, device=cuda), (2, 2))
    assert nvalid == nvalid_ref == 64
    err = np.max(np.abs(s2.cpu().numpy() - s2_ref))
    print("psiformer S^2_loc: max err", err, " max |ref|", np.max(np.abs(s2_ref)), " rel", err / np.max(np.abs(s2_ref)))
    assert err < 2e-4 * np.max(np.abs(s2_ref))
    assert np.max(np.abs(pairs.cpu().numpy() - pairs_ref)) < 2e-4 * np.max(np.abs(pairs_ref))
    # windows of one pair: the same rows at other batch sizes, where the network's GEMMs may tile otherwise
    s2w, _, _, _ = spin_square_sums(lambda r: model.apply(params, r), torch.tensor(x, device=cuda), (2, 2), max_rows=64)
    assert np.max(np.abs(s2w.cpu().numpy() - s2_ref)) < 2e-4 * np.max(np.abs(s2_ref))


class _Recording(ESTIMATORS["spin_square"]):
    """The estimator, keeping the walkers of every step for the test's bound."""

    seen: list = []

    def evaluate(self, i, params, key, data, system, state, aux_data):
        type(self).seen.append(data.reshape(-1, *data.shape[-2:]).cpu().numpy().copy())
        return super().evaluate(i, params, key, data, system, state, aux_data)


def test_driver_on_a_checkpoint(cuda, tmp_path):
    """evaluate on a (2,2)(3,3,2) checkpoint with 512 walkers: <S^2> = 0 within the float32 bound of
    the steps' own walkers, total spin 0, the exchange ratios sum to n_up; max_rows of one pair gives
    the same digest bits."""
    cfg = Config.from_dict({
        "batch_size": 512, "seed": 3,
        "system": {"nspins": (2, 2), "flux": 7},
        "network": {"type": "halperin", "halperin": {"exponents": [3, 3, 2]}},
        "mcmc": {"burn_in": 5},
        "optim": {"iterations": 2, "optimizer": "none"},
        "log": {"save_path": str(tmp_path)},
    })
    train(cfg)
    ckpt = sorted(tmp_path.glob("ckpt_*.npz"))[-1]
    steps = 5
    _Recording.seen = []
    out, vals = evaluate(DeepHallAdaptor(), _Recording, ckpt, steps, burn_in=3)
    assert vals["spin_square"].shape == (steps,) and vals["exchange"].shape == (steps, 2, 2)
    assert len(_Recording.seen) == steps and _Recording.seen[0].shape == (512, 4, 2)
    ref = HalperinCallable((2, 2), 7, (3, 3, 2))
    fn = lambda rows: ref(None, torch.as_tensor(rows, dtype=torch.float64)).numpy()  # noqa: E731
    bound = np.mean([SR.float32_log_bound(*SR.spin_square_of(fn, x, (2, 2))[4:]).mean() for x in _Recording.seen])
    print("driver: <S^2> =", out["spin_square"].item(), "+-", out["spin_square_err"].item(), " imag",
          out["spin_square_imag"].item(), " bound", bound, " S =", out["total_spin"].item())
    assert abs(out["spin_square"].item()) <= bound and abs(out["spin_square_imag"].item()) <= bound
    assert abs(out["total_spin"].item()) < 1e-3
    assert abs(out["exchange"].sum().item() - 2.0) <= bound  # S^2 = 0 = N / 2 - sum: the ratios sum to n_up
    assert out["sz"].item() == 0.0 and out["walkers"] == steps * 512
    assert torch.isfinite(out["spin_square_err"])
    plain, _ = evaluate(DeepHallAdaptor(), ESTIMATORS["spin_square"], ckpt, steps, burn_in=3)
    chunked, _ = evaluate(DeepHallAdaptor(), ESTIMATORS["spin_square"], ckpt, steps, burn_in=3,
                          estimator_options={"max_rows": 512})
    for k in ("spin_square", "spin_square_err", "spin_square_imag", "total_spin", "exchange", "sz"):
        a, b, c = (torch.as_tensor(o[k]) for o in (out, plain, chunked))
        same = lambda u, v: torch.equal(torch.view_as_real(u.to(torch.complex128)).view(torch.int64),  # noqa: E731
                                        torch.view_as_real(v.to(torch.complex128)).view(torch.int64))
        assert same(a, b) and same(b, c), k
