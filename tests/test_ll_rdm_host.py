"""Landau-level-resolved one-body density matrix without a GPU: the basis size, the argument
checks of the dh_rdm_* calls (validation comes before any device call), the estimator's
registration and options, and its digest on hand-made matrices."""

from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from deephall_amd import _lib

DH_EINVAL = -1


@pytest.mark.parametrize("flux,levels,norb", [(6, 1, 7), (2, 3, 15), (15, 3, 54), (57, 3, 180)])
def test_norb(flux, levels, norb):
    assert _lib.load().dh_rdm_norb(flux, levels) == norb


# ---- argument checks of the C calls: DH_EINVAL before any device call ------------------------------

def _buf(n=64):
    """A host buffer standing in for a device pointer: a rejected call never touches it."""
    b = (C.c_float * n)()
    return b, C.cast(b, C.c_void_p)


GOOD = dict(B=8, nelec=3, n_up=2, flux=6, levels=2, P=2, n=5)
BAD_BASIS = {"levels = 0": dict(levels=0), "levels = 5": dict(levels=5), "flux = -1": dict(flux=-1),
             "flux = 127": dict(flux=127)}
BAD_SIZE = {"nelec = 0": dict(nelec=0, n_up=0), "nelec = 33": dict(nelec=33), "B = 0": dict(B=0), "P = 0": dict(P=0)}
BAD_SPIN = {"n_up = -1": dict(n_up=-1), "n_up = nelec + 1": dict(n_up=4)}


def _rejected(lib, rc):
    assert rc == DH_EINVAL
    assert len(lib.dh_last_error()) > 0


def _harmonics(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("points", "out")}
    return lib.dh_monopole_harmonics(ptr["points"], a["n"], a["flux"], a["levels"], ptr["out"], None)


def _displace(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("x", "r_prime", "xp")}
    return lib.dh_rdm_displace(ptr["x"], ptr["r_prime"], a["B"], a["nelec"], a["P"], ptr["xp"], None)


ACC_PTRS = ("x", "r_prime", "logpsi", "logpsi_p", "rho", "nvalid", "ws")


def _accumulate(lib, p, null=None, ws_bytes=1 << 40, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ACC_PTRS}
    return lib.dh_rdm_accumulate(ptr["x"], ptr["r_prime"], ptr["logpsi"], ptr["logpsi_p"], a["B"], a["nelec"],
                                 a["n_up"], a["flux"], a["levels"], a["P"], 0, ptr["rho"], ptr["nvalid"], ptr["ws"],
                                 ws_bytes, None)


@pytest.mark.parametrize("name", sorted({**BAD_BASIS, **BAD_SIZE, **BAD_SPIN}))
def test_rdm_calls_reject_bad_sizes(name):
    lib = _lib.load()
    keep, p = _buf()
    bad = {**BAD_BASIS, **BAD_SIZE, **BAD_SPIN}[name]
    _rejected(lib, _accumulate(lib, p, **bad))
    if name in BAD_BASIS:
        _rejected(lib, _harmonics(lib, p, **bad))
        assert lib.dh_rdm_norb(bad.get("flux", 6), bad.get("levels", 2)) == 0
    if name in BAD_SIZE:
        _rejected(lib, _displace(lib, p, **bad))
    if name not in BAD_SPIN:
        a = {**GOOD, **bad}
        assert lib.dh_rdm_workspace_bytes(a["B"], a["nelec"], a["flux"], a["levels"], a["P"]) == 0
    del keep


def test_rdm_calls_reject_null_pointers_and_no_points():
    lib = _lib.load()
    keep, p = _buf()
    for which in ("points", "out"):
        _rejected(lib, _harmonics(lib, p, null=which))
    _rejected(lib, _harmonics(lib, p, n=0))
    for which in ("x", "r_prime", "xp"):
        _rejected(lib, _displace(lib, p, null=which))
    for which in ACC_PTRS:
        _rejected(lib, _accumulate(lib, p, null=which))
    del keep


def test_rdm_workspace_bytes_and_a_short_workspace():
    lib = _lib.load()
    keep, p = _buf()
    need = lib.dh_rdm_workspace_bytes(GOOD["B"], GOOD["nelec"], GOOD["flux"], GOOD["levels"], GOOD["P"])
    norb, samples = 16, GOOD["B"] * GOOD["P"]
    # U (up and down) and V as double complex [samples][norb], and at least one [2][norb][norb] of partial sums
    assert need >= (3 * samples * norb + 2 * norb * norb) * 16
    _rejected(lib, _accumulate(lib, p, ws_bytes=need - 1))
    assert lib.dh_rdm_workspace_bytes(2**30, 1, 6, 2, 2) == 0  # P B past 2^30
    assert lib.dh_rdm_workspace_bytes(2**22, 32, 6, 2, 1) == 0  # P B nelec^2 past 2^31
    del keep


# ---- the estimator's registration, options and digest ------------------------------------------------

def test_ll_rdm_is_registered_apart_from_the_reference_names():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS
    from deephall_amd.netobs.observables import ll_rdm

    assert ESTIMATORS["ll_rdm"] is EXTRA_ESTIMATORS["ll_rdm"] is ll_rdm.DEFAULT is ll_rdm.LLRDMEstimator
    assert ESTIMATORS.get("ll_rdm") is ll_rdm.DEFAULT
    assert "ll_rdm" not in list(ESTIMATORS) and len(ESTIMATORS) == 4


def test_ll_rdm_reads_its_options():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import ll_rdm

    sys_ = HallSystem(spins=[2, 1], flux=3)
    est = ll_rdm.LLRDMEstimator(None, sys_, {}, {})
    assert (est.levels, est.points, est.by_spin) == (2, 1, False) and est.observable.shape == (1, 10, 10)
    est = ll_rdm.LLRDMEstimator(None, sys_, {"levels": 3, "points": 4, "by_spin": True}, {})
    assert (est.levels, est.points, est.by_spin) == (3, 4, True) and est.observable.shape == (2, 18, 18)
    values, state = est.empty_val_state(7)
    assert values["ll_rdm"].shape == (7, 2, 18, 18) and values["ll_rdm"].dtype == torch.complex128
    assert state == {"samples": 0}
    for bad in ({"levels": 0}, {"levels": 5}, {"points": 0}):
        with pytest.raises(ValueError):
            ll_rdm.LLRDMEstimator(None, sys_, bad, {})


def _filled(steps=2):
    """Filled lowest level at flux 2, levels 2 (norb 8): diag(1, 1, 1, 0, ...), the same at every step."""
    rho = torch.zeros(steps, 1, 8, 8, dtype=torch.complex128)
    for k in range(3):
        rho[:, 0, k, k] = 1.0
    return rho


def test_ll_rdm_digest_of_the_filled_lowest_level():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import ll_rdm

    est = ll_rdm.LLRDMEstimator(None, HallSystem(spins=[3, 0], flux=2), {"levels": 2}, {})
    out = est.digest({"ll_rdm": _filled()}, {"samples": 10})
    assert out["occupations"].shape == (1, 2) and out["occupations"].tolist() == [[3.0, 0.0]]
    assert out["occupations_err"].tolist() == [[0.0, 0.0]]
    assert out["lll_weight"].item() == 1.0 and out["residual"].item() == 0.0
    assert out["hermiticity"].item() == 0.0 and out["lz_offdiag"].item() == 0.0
    assert out["ll_rdm"].shape == (1, 8, 8) and out["diagonal"].shape == (1, 8)
    assert out["trace"].shape == (1,) and out["trace"][0].item() == 3.0
    assert torch.allclose(out["natural_occupations"], torch.tensor([[0.0] * 5 + [1.0] * 3], dtype=torch.float64))
    one = est.digest({"ll_rdm": _filled(1)}, {"samples": 5})
    assert torch.isnan(one["occupations_err"]).all() and one["occupations"].tolist() == [[3.0, 0.0]]


def test_ll_rdm_digest_sees_coherences():
    """Orbitals at flux 2, levels 2: level 0 has t = Q + m = 0, 1, 2 at 0..2, level 1 has t = -1..3 at
    3..7.  (0, 1) couples m != m' inside level 0; (1, 5) couples the two levels at the same m."""
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables import ll_rdm

    est = ll_rdm.LLRDMEstimator(None, HallSystem(spins=[3, 0], flux=2), {"levels": 2}, {})
    rho = _filled()
    rho[:, 0, 1, 5] = 0.5
    rho[:, 0, 5, 1] = 0.5
    rho[:, 0, 5, 5] = 0.25
    out = est.digest({"ll_rdm": rho}, {})
    assert out["lz_offdiag"].item() == 0.0 and out["hermiticity"].item() == 0.0
    assert out["occupations"].tolist() == [[3.0, 0.25]] and out["residual"].item() == -0.25
    assert out["lll_weight"].item() == 1.0
    rho[:, 0, 0, 1] = 0.25j
    out = est.digest({"ll_rdm": rho}, {})
    assert out["lz_offdiag"].item() == 0.25
    norm = math.sqrt(3 + 0.25**2 + 2 * 0.5**2 + 0.25**2)
    assert abs(out["hermiticity"].item() - math.sqrt(2) * 0.25 / norm) < 1e-15
    # by_spin: one row of occupations per spin block, the lowest-level weight summed over both
    est2 = ll_rdm.LLRDMEstimator(None, HallSystem(spins=[2, 1], flux=2), {"levels": 2, "by_spin": True}, {})
    rho2 = torch.zeros(2, 2, 8, 8, dtype=torch.complex128)
    rho2[:, 0, 0, 0] = rho2[:, 0, 1, 1] = rho2[:, 1, 2, 2] = 1.0
    rho2[1, 1, 2, 2] = 0.5
    rho2[1, 1, 4, 4] = 0.5
    out = est2.digest({"ll_rdm": rho2}, {})
    assert out["occupations"].tolist() == [[2.0, 0.0], [0.75, 0.25]]
    assert abs(out["occupations_err"][1, 0].item() - 0.25) < 1e-15  # steps 1.0 and 0.5: std 0.5 / sqrt 2, / sqrt 2
    assert abs(out["lll_weight"].item() - 2.75 / 3) < 1e-15 and out["residual"].item() == 0.0
