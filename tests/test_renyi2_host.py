"""Renyi-2 swap estimator without a GPU: the exact filled-Landau-level answer
(netobs/entanglement.py), the argument checks of the dh_swap_* calls (validation comes before
any device call), the estimator's registration and options."""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from deephall_amd import _lib
from deephall_amd.netobs.entanglement import cap_occupations, filled_lll_cap

ANGLES = [0.4, 1.0, math.pi / 2, 2.2, 2.9]
DH_EINVAL = -1


def test_half_sphere_purity_of_three_electrons():
    purity, sector, number = filled_lll_cap(2, [math.pi / 2])
    assert abs(purity[0] - 625 / 2048) < 1e-14
    assert sector.shape == (1, 4) and number.shape == (1, 4)


@pytest.mark.parametrize("flux", [2, 3, 6])
def test_cap_occupations_match_quadrature(flux):
    """lambda_m from the binomial sum against a 20001-point trapezoid integral of |Y_{Q,Q,m}|^2
    over the cap, |Y|^2 = (2Q + 1) / (4 pi) C(2Q, Q - m) ((1 - x) / 2)^(Q - m) ((1 + x) / 2)^(Q + m),
    x = cos theta (orbitals_kernel's convention, without its clip at the poles).  1e-6 is the
    quadrature's error: h^2 / 12 x the cap's length x max |f''| with h = 1.5e-4 and
    |f''| of order (2Q + 1) Q^2 / 2 < 130 gives 2.5e-7 at the largest flux here."""
    for theta in ANGLES:
        t = np.linspace(0.0, theta, 20001)
        x = np.cos(t)
        lam = cap_occupations(flux, theta)
        assert len(lam) == flux + 1
        for k in range(flux + 1):  # k = Q + m
            f = ((flux + 1) / (4 * np.pi) * math.comb(flux, flux - k) * ((1 - x) / 2) ** (flux - k)
                 * ((1 + x) / 2) ** k * 2 * np.pi * np.sin(t))
            quad = np.sum((f[1:] + f[:-1]) * np.diff(t)) / 2
            assert abs(lam[k] - quad) < 1e-6, (flux, theta, k)


@pytest.mark.parametrize("flux", [2, 3, 6])
def test_filled_lll_cap_identities(flux):
    purity, sector, number = filled_lll_cap(flux, ANGLES)
    mirror, _, _ = filled_lll_cap(flux, [math.pi - t for t in ANGLES])
    assert sector.shape == number.shape == (len(ANGLES), flux + 2)
    assert np.max(np.abs(sector.sum(-1) - purity)) < 1e-14
    assert np.max(np.abs(number.sum(-1) - 1.0)) < 1e-14
    assert np.max(np.abs(purity - mirror)) < 1e-13  # a pure state: Tr rho_A^2 = Tr rho_complement^2
    assert (purity > 0).all() and (purity <= 1).all() and (sector >= 0).all()


# ---- argument checks of the C calls: DH_EINVAL before any device call ------------------------------

def _buf(n=64):
    """A host buffer standing in for a device pointer: a rejected call never touches it."""
    b = (C.c_float * n)()
    return b, C.cast(b, C.c_void_p)


def _thetas(*v):
    return (C.c_float * len(v))(*v)


GOOD = dict(B=8, nelec=3, n_up=2, n_dn=1, A=2)
BAD = {
    "B < 2": dict(B=1),
    "nelec < 1": dict(nelec=0, n_up=0, n_dn=0),
    "n_up + n_dn != nelec": dict(n_up=2, n_dn=2),
    "A < 1": dict(A=0),
    "A above the cap": dict(A=_lib.DH_SWAP_MAX_ANGLES + 1),
}


def _rejected(lib, rc):
    assert rc == DH_EINVAL
    assert len(lib.dh_last_error()) > 0


def _classify(lib, p, th, x=True, sector=True, counts=True, **kw):
    a = {**GOOD, **kw}
    return lib.dh_swap_classify(p if x else None, a["B"], a["nelec"], a["n_up"], a["n_dn"], th, a["A"],
                                p if sector else None, p if counts else None, None)


def _compact(lib, p, th, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("x", "sector", "start", "pair", "xs", "ws")}
    return lib.dh_swap_compact(ptr["x"], a["B"], a["nelec"], a["n_up"], a["n_dn"], th, a["A"], ptr["sector"],
                               ptr["start"], ptr["pair"], ptr["xs"], ptr["ws"], 1 << 20, None)


def _reduce(lib, p, null=None, M=1, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("logpsi", "logpsi_s", "pair", "sector", "start", "sums")}
    return lib.dh_swap_reduce(ptr["logpsi"], ptr["logpsi_s"], a["B"], a["nelec"], a["n_up"], a["n_dn"], a["A"], M,
                              ptr["pair"], ptr["sector"], ptr["start"], ptr["sums"], None)


@pytest.mark.parametrize("name", sorted(BAD))
def test_swap_calls_reject_bad_sizes(name):
    lib = _lib.load()
    keep, p = _buf()
    th = _thetas(*([0.5] * (_lib.DH_SWAP_MAX_ANGLES + 1)))
    _rejected(lib, _classify(lib, p, th, **BAD[name]))
    _rejected(lib, _compact(lib, p, th, **BAD[name]))
    _rejected(lib, _reduce(lib, p, **BAD[name]))
    del keep


def test_swap_calls_reject_null_pointers():
    lib = _lib.load()
    keep, p = _buf()
    th = _thetas(0.5, 1.0)
    for which in ("x", "sector", "counts"):
        _rejected(lib, _classify(lib, p, th, **{which: False}))
    _rejected(lib, _classify(lib, p, None))
    for which in ("x", "sector", "start", "pair", "xs", "ws"):
        _rejected(lib, _compact(lib, p, th, null=which))
    _rejected(lib, _compact(lib, p, None))
    for which in ("logpsi", "logpsi_s", "pair", "sector", "start", "sums"):
        _rejected(lib, _reduce(lib, p, null=which))
    del keep


def test_swap_calls_reject_nan_theta_and_bad_m():
    lib = _lib.load()
    keep, p = _buf()
    th = _thetas(0.5, float("nan"))
    _rejected(lib, _classify(lib, p, th))
    _rejected(lib, _compact(lib, p, th))
    _rejected(lib, _reduce(lib, p, M=-1))
    _rejected(lib, _reduce(lib, p, M=GOOD["A"] * (GOOD["B"] // 2) + 1))
    del keep


def test_swap_workspace_bytes():
    lib = _lib.load()
    assert lib.dh_swap_workspace_bytes(1, 2) == 0
    assert lib.dh_swap_workspace_bytes(8, 0) == 0
    assert lib.dh_swap_workspace_bytes(8, _lib.DH_SWAP_MAX_ANGLES + 1) == 0
    assert lib.dh_swap_workspace_bytes(2**31 - 1, 64) == 0  # 2 A P would not fit an int
    n = lib.dh_swap_workspace_bytes(515, 5)
    assert n >= 5 * 257 * 4 and n % 64 == 0


# ---- the estimator's registration and options ---------------------------------------------------------

def test_renyi2_is_registered_and_reads_its_options():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS, HallSystem
    from deephall_amd.netobs.observables import renyi2

    assert ESTIMATORS["renyi2"] is renyi2.DEFAULT is renyi2.Renyi2Estimator
    assert ESTIMATORS.get("renyi2") is renyi2.DEFAULT and ESTIMATORS.get("nope") is None
    assert set(EXTRA_ESTIMATORS) == {"renyi2"}  # not a reference name: listed apart from the four
    with pytest.raises(KeyError):
        ESTIMATORS["nope"]
    sys_ = HallSystem(spins=[2, 1], flux=3)
    est = renyi2.Renyi2Estimator(None, sys_, {}, {})
    assert est.observable.shape == (16,)
    assert np.allclose(est.thetas, np.linspace(0, np.pi, 18)[1:-1], rtol=0, atol=1e-15)
    est = renyi2.Renyi2Estimator(None, sys_, {"thetas": 5}, {})
    assert est.observable.shape == (5,) and np.allclose(est.thetas, np.linspace(0, np.pi, 7)[1:-1], atol=1e-15)
    est = renyi2.Renyi2Estimator(None, sys_, {"thetas": [0.3, 1.2, 2.0]}, {})
    assert est.observable.shape == (3,) and est.thetas == [0.3, 1.2, 2.0]
    values, state = est.empty_val_state(7)
    assert values["purity"].shape == (7, 3, 6) and str(values["purity"].dtype) == "torch.complex128"
    assert state["counts"].shape == (3, 6) and state["pairs"] == 0
    for bad in (0, [], [0.3, float("nan")]):
        with pytest.raises(ValueError):
            renyi2.Renyi2Estimator(None, sys_, {"thetas": bad}, {})


def test_renyi2_digest_on_known_step_values():
    """digest from hand-made step values: two steps, one angle, (1, 0) electrons -> K = 2."""
    import torch

    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import renyi2

    est = renyi2.Renyi2Estimator(None, HallSystem(spins=[1, 0], flux=0), {"thetas": [1.0]}, {})
    values = {"purity": torch.tensor([[[0.30, 0.20]], [[0.34, 0.24]]], dtype=torch.complex128)}
    state = {"counts": torch.tensor([[30, 10]]), "pairs": 20}
    out = est.digest(values, state)
    assert out["purity"].shape == (1,) and abs(out["purity"][0].item() - 0.54) < 1e-15
    assert abs(out["renyi2"][0].item() + math.log(0.54)) < 1e-15
    # step sums 0.50 and 0.58: std 0.04 sqrt(2), standard error 0.04, over the purity
    assert abs(out["renyi2_err"][0].item() - 0.04 / 0.54) < 1e-12
    assert torch.allclose(out["number_distribution"], torch.tensor([[0.75, 0.25]], dtype=torch.float64))
    assert torch.allclose(out["sector_renyi2"], -torch.log(torch.tensor([[0.32 / 0.75**2, 0.22 / 0.25**2]],
                                                                        dtype=torch.float64)))
    empty = est.digest(values, {"counts": torch.tensor([[40, 0]]), "pairs": 20})
    assert math.isnan(empty["sector_renyi2"][0, 1].item())
