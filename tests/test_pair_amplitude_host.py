"""Pair amplitudes without a GPU: the closed form of the pair projector against the orbital route
(float64 numpy, pairamp_ref.py), its symmetries, the Haldane pseudopotentials, the argument checks
of the dh_pair_* calls (validation comes before any device call), the estimator's registration and
options, and its digest on hand-made step values."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

import pairamp_ref as PR
from deephall_amd import _lib
from deephall_amd.netobs import pseudopotential as V

DH_EINVAL = -1


def quadruples(flux, n=16):
    """n random quadruples (r1, r2, r1', r2') [n, 4, 2]; quadruple 0 has its primed pair 0.05 rad
    from the unprimed pair."""
    pts = PR.uniform(n, 4, seed=100 + flux).astype(np.float64)
    pts[0, 0, 0], pts[0, 1, 0] = 1.0, 2.0
    pts[0, 2:] = pts[0, :2] + [0.05, 0.0]
    return pts


# ---- 1 - 3: the closed form ---------------------------------------------------------------------------

@pytest.mark.parametrize("flux", [1, 2, 9, 15])
def test_closed_form_equals_the_orbital_route(flux):
    """The orbital route loses accuracy with 2Q (its eigenvectors); measured 2e-14 at 2Q = 15 here."""
    pts = quadruples(flux)
    K = PR.pair_kernel(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux)
    Ko = PR.pair_kernel_orbitals(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux)
    Ks = PR.pair_kernel_sum(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux)
    scale = np.max(np.abs(K), axis=-1, keepdims=True)
    print("flux", flux, " closed form vs orbitals", np.max(np.abs(K - Ko) / scale), " recurrence vs sum",
          np.max(np.abs(K - Ks) / scale))
    assert np.max(np.abs(K - Ko) / scale) <= 1e-8
    assert np.max(np.abs(K - Ks) / scale) <= 1e-12


@pytest.mark.parametrize("flux", [1, 2, 9, 15, 57])
def test_diagonal_is_real_and_not_negative(flux):
    pts = quadruples(flux)
    K = PR.pair_kernel(pts[:, 0], pts[:, 1], pts[:, 0], pts[:, 1], flux)
    scale = np.max(np.abs(K))
    assert np.max(np.abs(K.imag)) <= 1e-13 * scale and np.min(K.real) >= -1e-13 * scale
    # its integral over both points is (4 pi)^2 (2L + 1); at r1 = r2 only L = 2Q is left
    same = PR.pair_kernel(pts[:, 0], pts[:, 0], pts[:, 2], pts[:, 3], flux)
    assert (same[:, :flux] == 0).all() and np.isfinite(same).all()


@pytest.mark.parametrize("flux", [1, 2, 9, 15])
def test_exchange_symmetry(flux):
    pts = quadruples(flux)
    K = PR.pair_kernel(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux)
    Kx = PR.pair_kernel(pts[:, 1], pts[:, 0], pts[:, 2], pts[:, 3], flux)
    sign = (-1.0) ** (flux - np.arange(flux + 1))
    assert np.max(np.abs(Kx - sign * K)) <= 1e-12 * np.max(np.abs(K))


def test_projectors_resolve_the_pair_space():
    """sum_L K_L is the identity of two lowest-level electrons: K^(1)(r1, r1') K^(1)(r2, r2') with
    4 pi K^(1)(r, r') = (2Q + 1) <r|r'>^2Q."""
    for flux in (1, 2, 9):
        pts = quadruples(flux)
        K = PR.pair_kernel(pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], flux).sum(-1)
        s = [PR.spinor(pts[:, k]) for k in range(4)]
        want = (flux + 1) ** 2 * (PR.bracket(s[0], s[2]) * PR.bracket(s[1], s[3])) ** flux
        assert np.max(np.abs(K - want)) <= 1e-12 * np.max(np.abs(want))


# ---- 4, 5: pseudopotentials -----------------------------------------------------------------------------

@pytest.mark.parametrize("flux", [2, 9, 15])
def test_harmonic_pseudopotentials(flux):
    Q, L = flux / 2, np.arange(flux + 1)
    got = V.harmonic_pseudopotentials(flux)
    assert got.shape == (flux + 1,) and np.max(np.abs(got - L * (L + 1) / (2 * Q * (Q + 1)))) <= 1e-12


def test_coulomb_pseudopotentials():
    want = [0.2481, 0.2508, 0.2563, 0.2654, 0.2792, 0.2999, 0.3320, 0.3867, 0.5013, 0.9762]
    got = V.coulomb_pseudopotentials(9, math.sqrt(4.5))
    print("coulomb V_L at 2Q = 9:", np.round(got, 5))
    assert np.max(np.abs(got - want)) <= 1e-4


@pytest.mark.parametrize("flux", [1, 2, 9])
def test_moments_equal_the_quadrature_over_both_electrons(flux):
    """pair_legendre_moments integrates the rotation-invariant pair density in cos gamma; the
    restatement integrates the highest-weight state over both electrons."""
    M = V.pair_legendre_moments(flux)
    assert M.shape == (flux + 1, flux + 1) and np.max(np.abs(M[0] - 1.0)) <= 1e-13
    assert np.max(np.abs(M - PR.legendre_moments(flux))) <= 1e-12


def test_pseudopotential_arguments():
    assert np.array_equal(V.pseudopotentials(2, [1.0, 2.0, 3.0, 99.0]), V.pseudopotentials(2, [1.0, 2.0, 3.0]))
    assert np.allclose(V.pseudopotentials(3, [2.0]), 2.0)  # a constant
    A = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(V.interaction_energy(A, [1.0, 0.0, 2.0]), [4.0, 13.0])
    for bad in (lambda: V.pair_legendre_moments(-1), lambda: V.pair_legendre_moments(127),
                lambda: V.harmonic_pseudopotentials(0), lambda: V.coulomb_pseudopotentials(3, 0.0),
                lambda: V.interaction_energy(A, [1.0, 2.0])):
        with pytest.raises(ValueError):
            bad()


# ---- 6: argument checks of the C calls: DH_EINVAL before any device call -------------------------------

def _buf(n=64):
    """A host buffer standing in for a device pointer: a rejected call never touches it."""
    b = (C.c_float * n)()
    return b, C.cast(b, C.c_void_p)


GOOD = dict(B=8, nelec=4, n_up=2, flux=6, P=2, pair0=0, pair1=6, n=5)
BAD_FLUX = {"flux = -1": dict(flux=-1), "flux = 127": dict(flux=127)}
BAD_SIZE = {"nelec = 0": dict(nelec=0, n_up=0), "nelec = 33": dict(nelec=33), "B = 0": dict(B=0), "P = 0": dict(P=0),
            "rows = 2^31": dict(B=2**24, nelec=17, P=1),  # 136 pairs x 2^24 rows
            "P B = 2^30 + 2": dict(B=2**29 + 1, nelec=2, P=2)}  # one pair: rows below 2^31, samples past 2^30
BAD_SPIN = {"n_up = -1": dict(n_up=-1), "n_up = nelec + 1": dict(n_up=5)}
BAD_WINDOW = {"pair0 = -1": dict(pair0=-1), "pair1 = pair0": dict(pair0=2, pair1=2), "pair1 = pairs + 1": dict(pair1=7)}


def _rejected(lib, rc):
    assert rc == DH_EINVAL
    assert len(lib.dh_last_error()) > 0


def _displace(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("x", "r1", "r2", "xp")}
    return lib.dh_pair_displace(ptr["x"], ptr["r1"], ptr["r2"], a["B"], a["nelec"], a["P"], a["pair0"], a["pair1"],
                                ptr["xp"], None)


def _kernel(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("points", "out")}
    return lib.dh_pair_kernel(ptr["points"], a["n"], a["flux"], ptr["out"], None)


ACC_PTRS = ("x", "r1", "r2", "logpsi", "logpsi_p", "A", "nvalid", "ws")


def _accumulate(lib, p, null=None, ws_bytes=1 << 40, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ACC_PTRS}
    return lib.dh_pair_accumulate(ptr["x"], ptr["r1"], ptr["r2"], ptr["logpsi"], ptr["logpsi_p"], a["B"], a["nelec"],
                                  a["n_up"], a["flux"], a["P"], ptr["A"], ptr["nvalid"], ptr["ws"], ws_bytes, None)


@pytest.mark.parametrize("name", sorted({**BAD_FLUX, **BAD_SIZE, **BAD_SPIN, **BAD_WINDOW}))
def test_pair_calls_reject_bad_sizes(name):
    lib = _lib.load()
    keep, p = _buf()
    bad = {**BAD_FLUX, **BAD_SIZE, **BAD_SPIN, **BAD_WINDOW}[name]
    a = {**GOOD, **bad}
    if name in BAD_WINDOW:
        _rejected(lib, _displace(lib, p, **bad))
        return
    _rejected(lib, _accumulate(lib, p, **bad))
    if name in BAD_FLUX:
        _rejected(lib, _kernel(lib, p, **bad))
    if name in BAD_SIZE:
        _rejected(lib, _displace(lib, p, **{"pair1": 1, **bad}))
    if name not in BAD_SPIN:
        assert lib.dh_pair_workspace_bytes(a["B"], a["nelec"], a["flux"], a["P"]) == 0
    del keep


def test_pair_calls_reject_null_pointers_and_no_points():
    lib = _lib.load()
    keep, p = _buf()
    for which in ("x", "r1", "r2", "xp"):
        _rejected(lib, _displace(lib, p, null=which))
    for which in ("points", "out"):
        _rejected(lib, _kernel(lib, p, null=which))
    _rejected(lib, _kernel(lib, p, n=0))
    _rejected(lib, _kernel(lib, p, n=2**31 // 127 + 1, flux=126))
    for which in ACC_PTRS:
        _rejected(lib, _accumulate(lib, p, null=which))
    _rejected(lib, _displace(lib, p, nelec=1, pair1=1))  # one electron has no pair
    del keep


def test_pair_workspace_bytes_and_a_short_workspace():
    lib = _lib.load()
    keep, p = _buf()
    need = lib.dh_pair_workspace_bytes(GOOD["B"], GOOD["nelec"], GOOD["flux"], GOOD["P"])
    samples, pairs = GOOD["B"] * GOOD["P"], 6
    # a flag per sample and, per pair and chunk of samples, flux + 1 double complex partial sums
    assert need >= 4 * samples + pairs * (GOOD["flux"] + 1) * 16
    _rejected(lib, _accumulate(lib, p, ws_bytes=need - 1))
    assert lib.dh_pair_workspace_bytes(8, 1, 6, 1) > 0  # one electron: no pair, but a valid call
    del keep


# ---- 7, 8: the estimator's registration, options and digest -----------------------------------------------

def test_pair_amplitude_is_registered_apart_from_the_reference_names():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS
    from deephall_amd.netobs.observables import pair_amplitude

    est = pair_amplitude.PairAmplitudeEstimator
    assert ESTIMATORS["pair_amplitude"] is EXTRA_ESTIMATORS["pair_amplitude"] is pair_amplitude.DEFAULT is est
    assert ESTIMATORS.get("pair_amplitude") is est and EXTRA_ESTIMATORS.get("pair_amplitude") is est
    assert "pair_amplitude" not in list(ESTIMATORS) and len(ESTIMATORS) == 4
    assert list(EXTRA_ESTIMATORS) == ["renyi2"]


def test_pair_amplitude_reads_its_options():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import pair_amplitude

    sys_ = HallSystem(spins=[2, 2], flux=5)
    est = pair_amplitude.PairAmplitudeEstimator(None, sys_, {}, {})
    assert (est.points, est.max_rows, est.legendre) == (1, None, None) and est.observable.shape == (3, 6)
    assert est.radius == math.sqrt(2.5) and est.strength == 1.0 and sorted(est.potentials) == ["coulomb", "harmonic"]
    est = pair_amplitude.PairAmplitudeEstimator(None, sys_, {"points": 3, "max_rows": 1000, "legendre": [0, 0, 1],
                                                             "radius": 2.0, "interaction_strength": 0.5}, {})
    assert (est.points, est.max_rows, est.legendre) == (3, 1000, [0.0, 0.0, 1.0])
    assert np.allclose(est.potentials["coulomb"].numpy(), 0.5 * V.coulomb_pseudopotentials(5, 2.0), rtol=0, atol=1e-15)
    assert np.allclose(est.potentials["legendre"].numpy(), 0.5 * V.pair_legendre_moments(5)[2], rtol=0, atol=1e-15)
    values, state = est.empty_val_state(7)
    assert values["pair_amplitude"].shape == (7, 3, 6) and values["pair_amplitude"].dtype == torch.complex128
    assert state == {"samples": 0}

    class WithSystem:  # the adaptor's system supplies the radius and the strength
        class cfg:
            class system:
                radius, interaction_strength = 3.0, 2.0

    est = pair_amplitude.PairAmplitudeEstimator(WithSystem(), sys_, {}, {})
    assert (est.radius, est.strength) == (3.0, 2.0)
    for bad in ({"points": 0}, {"points": 1.5}, {"max_rows": 0}, {"legendre": []}, {"legendre": [math.nan]}):
        with pytest.raises(ValueError):
            pair_amplitude.PairAmplitudeEstimator(None, sys_, bad, {})
    with pytest.raises(ValueError):
        pair_amplitude.PairAmplitudeEstimator(None, HallSystem(spins=[2, 0], flux=0), {}, {})


def test_pair_amplitude_digest():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import pair_amplitude

    # the filled level, N = 3 at 2Q = 2: all three pairs at L = 1, the same at every step
    est = pair_amplitude.PairAmplitudeEstimator(None, HallSystem(spins=[3, 0], flux=2), {}, {})
    steps = torch.zeros(2, 3, 3, dtype=torch.complex128)
    steps[:, 0, 1] = 3.0
    out = est.digest({"pair_amplitude": steps}, {"samples": 8})
    assert out["amplitudes"].tolist() == [[0.0, 3.0, 0.0], [0.0] * 3, [0.0] * 3]
    assert out["by_relative"].tolist() == out["amplitudes"].tolist()  # m = 1 is L = 1 at 2Q = 2
    assert out["amplitudes_err"].abs().max().item() == 0.0 and out["total"].tolist() == [0.0, 3.0, 0.0]
    assert out["pairs_in_lll"].item() == 1.0 and out["forbidden"].item() == 0.0 and out["imag"].item() == 0.0
    assert abs(out["harmonic_energy"].item() - 3 * 2 / (2 * 1 * 2)) < 1e-12 and out["harmonic_energy_err"].item() == 0.0
    assert abs(out["coulomb_energy"].item() - 3 * V.coulomb_pseudopotentials(2, 1.0)[1]) < 1e-12
    assert "legendre_energy" not in out
    # a step that kept no sample is NaN and is left out: the same digest from the other steps
    holed = torch.cat([steps[:1], torch.full_like(steps[:1], math.nan), steps[1:]])
    again = est.digest({"pair_amplitude": holed}, {})
    assert all(torch.equal(again[k], out[k]) for k in out)
    none = est.digest({"pair_amplitude": holed[1:2]}, {})
    assert torch.isnan(none["amplitudes"]).all() and torch.isnan(none["coulomb_energy"])
    one = est.digest({"pair_amplitude": steps[:1]}, {})
    assert torch.isnan(one["amplitudes_err"]).all() and torch.isnan(one["coulomb_energy_err"])
    # two species at 2Q = 3, steps that differ: L = 3, 2, 1, 0 is m = 0, 1, 2, 3
    est = pair_amplitude.PairAmplitudeEstimator(None, HallSystem(spins=[2, 2], flux=3), {"legendre": [0.0, 1.0]}, {})
    steps = torch.zeros(2, 3, 4, dtype=torch.complex128)
    steps[0, 0] = torch.tensor([0.0, 0.25, 0.5, 0.0])   # up-up: 0.25 at L = 1 (m = 2, forbidden), 0.5 at L = 2
    steps[1, 0] = torch.tensor([0.0, -0.25, 1.5, 0.0])
    steps[:, 1, 3] = 4.0 + 0.5j                         # up-down at L = 3 (m = 0)
    steps[:, 2, 0] = torch.tensor([1.0, 0.5])           # down-down at L = 0 (m = 3)
    steps[:, 2, 3] = -0.125                             # down-down at m = 0: forbidden
    out = est.digest({"pair_amplitude": steps}, {})
    assert out["amplitudes"][0].tolist() == [0.0, 0.0, 1.0, 0.0]
    assert out["by_relative"][0].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert out["total"].tolist() == [0.75, 0.0, 1.0, 3.875]
    assert out["forbidden"].item() == 0.125 and out["imag"].item() == 0.5
    assert abs(out["pairs_in_lll"].item() - 5.625 / 6) < 1e-15
    assert abs(out["amplitudes_err"][0, 2].item() - 0.5) < 1e-15  # 0.5 and 1.5: std 1 / sqrt 2, / sqrt 2
    assert abs(out["amplitudes_err"][2, 0].item() - 0.25) < 1e-15
    M1 = V.pair_legendre_moments(3)[1]
    e = [float(steps[k].real.sum(0).numpy() @ M1) for k in range(2)]
    assert abs(out["legendre_energy"].item() - (e[0] + e[1]) / 2) < 1e-14
    assert abs(out["legendre_energy_err"].item() - abs(e[0] - e[1]) / 2) < 1e-14
