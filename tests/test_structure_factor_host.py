"""Static structure factor without a GPU: the sizes, the argument checks of the dh_sf_* calls
(validation comes before any device call), the estimator's registration and options, the
single-particle form factor against a quadrature, and the digest on hand-made step arrays."""

from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

import sf_ref as SR
from deephall_amd import _lib

DH_EINVAL = -1


@pytest.mark.parametrize("lmax,nlm", [(0, 1), (1, 3), (7, 36), (12, 91), (64, 2145)])
def test_nlm(lmax, nlm):
    lib = _lib.load()
    assert lib.dh_sf_nlm(lmax) == nlm == SR.nlm(lmax)
    assert _lib.DH_SF_MAX_L == 64 and lib.dh_sf_nlm(-1) == -1 and lib.dh_sf_nlm(65) == -1


def test_workspace_bytes():
    lib = _lib.load()
    # one partial of pair sums [3][lmax+1], multipole sums [2][nlm] complex and a count, at the least
    for B, N, lmax in ((1, 1, 0), (67, 6, 7), (1030, 6, 64), (4096, 20, 64)):
        need = lib.dh_sf_workspace_bytes(B, N, lmax)
        assert need >= (3 * (lmax + 1) + 4 * SR.nlm(lmax)) * 8 + 4
        assert need == lib.dh_sf_workspace_bytes(B, 1, lmax)  # the partials do not depend on nelec
    assert lib.dh_sf_workspace_bytes(4096, 20, 64) <= 64 << 20
    for B, N, lmax in ((0, 3, 4), (-1, 3, 4), (8, 0, 4), (8, 33, 4), (8, 3, -1), (8, 3, 65), (2**27, 16, 4),
                       (2**31 - 1, 2, 4)):
        assert lib.dh_sf_workspace_bytes(B, N, lmax) == 0, (B, N, lmax)
    assert lib.dh_sf_workspace_bytes(2**27 - 1, 16, 0) > 0  # B nelec = 2^31 - 16


# ---- argument checks of the C calls: DH_EINVAL before any device call ------------------------------

def _buf(n=64):
    """A host buffer standing in for a device pointer: a rejected call never touches it."""
    b = (C.c_float * n)()
    return b, C.cast(b, C.c_void_p)


GOOD = dict(B=8, nelec=3, n_up=2, lmax=5)
BAD = {"B = 0": dict(B=0), "B = -3": dict(B=-3), "nelec = 0": dict(nelec=0, n_up=0), "nelec = 33": dict(nelec=33),
       "B nelec = 2^31": dict(B=2**27, nelec=16), "n_up = -1": dict(n_up=-1), "n_up = nelec + 1": dict(n_up=4),
       "lmax = -1": dict(lmax=-1), "lmax = 65": dict(lmax=65)}


def _rejected(lib, rc):
    assert rc == DH_EINVAL
    assert len(lib.dh_last_error()) > 0 and lib.dh_last_error().startswith(b"sf:")


def _pairs(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("x", "T")}
    return lib.dh_sf_pairs(ptr["x"], a["B"], a["nelec"], a["n_up"], a["lmax"], ptr["T"], None)


def _multipoles(lib, p, null=None, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ("x", "rho")}
    return lib.dh_sf_multipoles(ptr["x"], a["B"], a["nelec"], a["n_up"], a["lmax"], ptr["rho"], None)


ACC_PTRS = ("x", "pair_sums", "rho_sums", "nvalid", "ws")


def _accumulate(lib, p, null=None, want=1, ws_bytes=1 << 40, **kw):
    a = {**GOOD, **kw}
    ptr = {n: (None if n == null else p) for n in ACC_PTRS}
    return lib.dh_sf_accumulate(ptr["x"], a["B"], a["nelec"], a["n_up"], a["lmax"], want, ptr["pair_sums"],
                                ptr["rho_sums"], ptr["nvalid"], ptr["ws"], ws_bytes, None)


@pytest.mark.parametrize("name", sorted(BAD))
def test_sf_calls_reject_bad_sizes(name):
    lib = _lib.load()
    keep, p = _buf()
    _rejected(lib, _pairs(lib, p, **BAD[name]))
    _rejected(lib, _multipoles(lib, p, **BAD[name]))
    _rejected(lib, _accumulate(lib, p, **BAD[name]))
    _rejected(lib, _accumulate(lib, p, want=0, null="rho_sums", **BAD[name]))
    del keep


def test_sf_calls_reject_null_pointers_and_a_short_workspace():
    lib = _lib.load()
    keep, p = _buf()
    for which in ("x", "T"):
        _rejected(lib, _pairs(lib, p, null=which))
    for which in ("x", "rho"):
        _rejected(lib, _multipoles(lib, p, null=which))
    for which in ACC_PTRS:
        _rejected(lib, _accumulate(lib, p, null=which))
    for which in ("x", "pair_sums", "nvalid", "ws"):  # rho_sums may be null only without the multipoles
        _rejected(lib, _accumulate(lib, p, null=which, want=0))
    need = lib.dh_sf_workspace_bytes(GOOD["B"], GOOD["nelec"], GOOD["lmax"])
    assert need > 0
    _rejected(lib, _accumulate(lib, p, ws_bytes=need - 1))
    _rejected(lib, _accumulate(lib, p, ws_bytes=need - 1, want=0, null="rho_sums"))
    _rejected(lib, _accumulate(lib, p, ws_bytes=0))
    del keep


def test_wrappers_refuse_cpu_tensors():
    from deephall_amd.netobs import _native

    x = torch.zeros(4, 3, 2)
    for call in (lambda: _native.sf_pairs(x, 2, 3), lambda: _native.sf_multipoles(x, 2, 3),
                 lambda: _native.sf_accumulate(x, 2, 3), lambda: _native.sf_accumulate_host(x, 2, 3, False)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


# ---- the estimator's registration and options ---------------------------------------------------------

def test_structure_factor_is_registered_apart_from_the_pinned_names():
    from deephall_amd.netobs import ESTIMATORS, EXTRA_ESTIMATORS
    from deephall_amd.netobs.observables import structure_factor

    cls = structure_factor.StructureFactorEstimator
    assert ESTIMATORS["structure_factor"] is EXTRA_ESTIMATORS["structure_factor"] is structure_factor.DEFAULT is cls
    assert EXTRA_ESTIMATORS.more["structure_factor"] is cls and ESTIMATORS.get("structure_factor") is cls
    assert list(ESTIMATORS) == ["density", "pair_corr", "overlap", "one_rdm"] and len(ESTIMATORS) == 4
    assert list(EXTRA_ESTIMATORS) == ["renyi2"] and "structure_factor" not in EXTRA_ESTIMATORS


def test_structure_factor_reads_its_options():
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables.structure_factor import StructureFactorEstimator as Est

    sys_ = HallSystem(spins=[2, 1], flux=3)
    est = Est(None, sys_, {}, {})
    assert (est.lmax, est.multipoles, est.nspins, est.flux) == (8, True, (2, 1), 3) and est.observable.shape == (9,)
    values, state = est.empty_val_state(7)
    assert values["pairs"].shape == (7, 3, 9) and values["pairs"].dtype == torch.float64
    assert values["rho"].shape == (7, 2, 45) and values["rho"].dtype == torch.complex128
    assert state == {"walkers": 0}
    est = Est(None, sys_, {"lmax": 0, "multipoles": False}, {})
    assert (est.lmax, est.multipoles) == (0, False) and sorted(est.empty_val_state(2)[0]) == ["pairs"]
    assert Est(None, HallSystem(spins=[20, 0], flux=57), None, None).lmax == 64  # min(2 flux + 2, 64)
    assert Est(None, sys_, {"lmax": 64}, {}).lmax == 64
    for bad in (-1, 65, 2.5, True):
        with pytest.raises(ValueError, match="lmax"):
            Est(None, sys_, {"lmax": bad}, {})


# ---- the form factor ------------------------------------------------------------------------------------

@pytest.mark.parametrize("flux", [2, 5, 8])
def test_form_factor_against_the_filled_level_quadrature(flux):
    """S(L) of the filled lowest level (N = 2Q + 1) from its pair density, 80-point Gauss-Legendre:
    1 - F_L for 1 <= L <= 2Q + 2 to 1e-11, S(0) = N, S(L > 2Q) = 1, and F_1 = Q / (Q + 1)."""
    from deephall_amd.netobs.observables.structure_factor import form_factor

    lmax = flux + 2
    ff = form_factor(flux, lmax)
    assert ff.dtype == torch.float64 and ff.shape == (lmax + 1,)
    s0, F = SR.form_factor_quadrature(flux, lmax)
    assert abs(s0 - (flux + 1)) < 1e-11
    worst = max(abs(ff[L].item() - (1.0 - F[L - 1])) for L in range(1, lmax + 1))
    print(f"form factor 2Q = {flux}: max |1 - F_L - quadrature| = {worst:.1e}")
    assert worst < 1e-11
    Q = flux / 2
    assert abs((1.0 - ff[1].item()) - Q / (Q + 1)) < 1e-15
    assert ff[0].item() == 0.0 and ff[flux + 1].item() == 1.0 and ff[flux + 2].item() == 1.0  # F_0 = 1, F_{L>2Q} = 0


def test_form_factor_at_the_largest_flux_and_lmax():
    from deephall_amd.netobs.observables.structure_factor import form_factor

    ff = form_factor(126, 64)  # exact integers: 253! and its kin never become floats
    assert torch.isfinite(ff).all() and (ff[1:] > 0).all() and (ff <= 1).all() and (ff[1:] > ff[:-1]).all()
    assert abs((1.0 - ff[1].item()) - 63 / 64) < 1e-15


# ---- the digest on hand-made step arrays ------------------------------------------------------------------

def _steps(nspins, lmax, steps=3, seed=0):
    """Step arrays a run could have produced: row L = 0 of the pair means is the pair counts, the
    rest random; rho random but for rho_00 = n_a / sqrt(4 pi)."""
    n_up, n_dn = nspins
    g = torch.Generator().manual_seed(seed)
    pairs = torch.rand(steps, 3, lmax + 1, generator=g, dtype=torch.float64) - 0.5
    pairs[:, 0, 0], pairs[:, 1, 0], pairs[:, 2, 0] = n_up * (n_up - 1) / 2, n_up * n_dn, n_dn * (n_dn - 1) / 2
    nlm = (lmax + 1) * (lmax + 2) // 2
    rho = torch.complex(torch.rand(steps, 2, nlm, generator=g, dtype=torch.float64) - 0.5,
                        torch.rand(steps, 2, nlm, generator=g, dtype=torch.float64) - 0.5)
    rho[:, 0, 0], rho[:, 1, 0] = n_up / math.sqrt(4 * math.pi), n_dn / math.sqrt(4 * math.pi)
    return pairs, rho


@pytest.mark.parametrize("nspins", [(3, 2), (4, 0), (0, 2), (1, 1)])
def test_digest_identities(nspins):
    from deephall_amd.netobs import HallSystem
    from deephall_amd.netobs.observables.structure_factor import StructureFactorEstimator as Est

    N, lmax, flux = sum(nspins), 6, 4
    est = Est(None, HallSystem(spins=list(nspins), flux=flux), {"lmax": lmax}, {})
    pairs, rho = _steps(nspins, lmax)
    out = est.digest({"pairs": pairs, "rho": rho}, {"walkers": 12})
    for k in ("structure_factor", "structure_factor_err", "spin_structure_factor", "connected", "guiding_center",
              "form_factor"):
        assert out[k].shape == (lmax + 1,) and out[k].dtype == torch.float64, k
    assert out["partial"].shape == (3, lmax + 1) and out["multipole_mean"].shape == (2, SR.nlm(lmax))
    s, (uu, ud, dd) = out["structure_factor"], out["partial"]
    assert (s - (uu + dd + 2 * ud)).abs().max() < 1e-12
    assert (out["spin_structure_factor"] - (uu + dd - 2 * ud)).abs().max() < 1e-12
    assert abs(s[0].item() - N) < 1e-12
    assert (s - (1 + 2 / N * pairs.sum(1).mean(0))).abs().max() < 1e-12
    assert (uu - (nspins[0] / N + 2 / N * pairs[:, 0].mean(0))).abs().max() < 1e-12
    assert (ud - pairs[:, 1].mean(0) / N).abs().max() < 1e-12
    # the error bar: the scatter of the steps' own S(L); zero where every step agrees (L = 0)
    s_steps = 1 + 2 / N * pairs.sum(1)
    assert torch.allclose(out["structure_factor_err"], s_steps.std(0, unbiased=True) / math.sqrt(3), rtol=1e-12, atol=0)
    assert out["structure_factor_err"][0].item() < 1e-15
    # connected: rho_00 = N / sqrt(4 pi) takes N off at L = 0; at L >= 1 the formula, M > 0 counted twice
    assert abs(out["connected"][0].item() - (s[0].item() - N)) < 1e-12
    mean = rho.mean(0).sum(0)
    for L in range(1, lmax + 1):
        k = L * (L + 1) // 2
        want = s[L] - 4 * math.pi / (N * (2 * L + 1)) * (mean[k].abs() ** 2 + 2 * (mean[k + 1:k + L + 1].abs() ** 2).sum())
        assert abs(out["connected"][L].item() - want.item()) < 1e-12
    assert torch.equal(out["multipole_mean"], rho.mean(0))
    assert (out["guiding_center"] - (s - out["form_factor"])).abs().max() < 1e-15


def test_digest_guiding_centre_of_the_filled_level_and_without_multipoles():
    """Fed S(L) = 1 - F_L (all of it in T_uu), the guiding-centre structure factor is 0 at every L."""
    from deephall_amd.netobs.observables.structure_factor import digest_steps, form_factor

    flux, lmax = 4, 6
    N = flux + 1
    ff = form_factor(flux, lmax)
    pairs = torch.zeros(2, 3, lmax + 1, dtype=torch.float64)
    pairs[:, 0] = (ff - 1.0) * N / 2
    out = digest_steps(pairs, None, (N, 0), flux)
    assert out["guiding_center"].abs().max() < 1e-15 and torch.equal(out["form_factor"], ff)
    assert (out["structure_factor"] - ff).abs().max() < 1e-15
    assert "connected" not in out and "multipole_mean" not in out
    one = digest_steps(pairs[:1], None, (N, 0), flux)
    assert torch.isnan(one["structure_factor_err"]).all() and torch.equal(one["structure_factor"], out["structure_factor"])
