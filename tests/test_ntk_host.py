"""MinSR without a GPU: the dh_ntk C ABI's host-side contract (exports, tile geometry,
workspace, argument checks that come before any device call), the config entry, the
single-rank guard, and the step's linear algebra against a parameter-space solve on a dense
stand-in Jacobian."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from deephall_amd import _lib, constants, optimizers
from deephall_amd.config import Config, OptimizerName
from deephall_amd.networks.psiformer import NetworkSpec
from helpers import CONFIGS

DH_EINVAL, DH_ENOMEM = -1, -3


def make_handle(name="C2", **kw):
    c = dict(CONFIGS[name])
    spec = NetworkSpec(**{**dict(nspins=c["nspins"], flux=c["flux"], ndets=c.get("determinants", 1),
                                 num_heads=c.get("num_heads", 4), heads_dim=c.get("heads_dim", 64), num_layers=2), **kw})
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dh_create(C.byref(spec.to_c()), C.byref(h)) == 0
    return lib, spec, h


def test_error_codes_match_header():
    from pathlib import Path
    import re

    txt = (Path(__file__).resolve().parents[1] / "include" / "deephall_amd.h").read_text()
    codes = dict(re.findall(r"#define (DH_E\w+) \(?(-?\d+)\)?", txt))
    assert int(codes["DH_EINVAL"]) == DH_EINVAL and int(codes["DH_ENOMEM"]) == DH_ENOMEM


def test_library_exports_ntk_symbols():
    lib = _lib.load()
    for s in ("dh_ntk_workspace_bytes", "dh_ntk_tile_walkers", "dh_ntk"):
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS


@pytest.mark.parametrize("name", ["C1", "C2", "C4", "MIX"])
def test_tile_walkers(name):
    lib, spec, h = make_handle(name)
    tw = lib.dh_ntk_tile_walkers(h)
    assert tw >= 1 and tw * spec.nelec <= 192
    lib.dh_destroy(h)


def test_workspace_monotone_and_covers_the_vjp():
    lib, spec, h = make_handle("C2")
    sizes = [lib.dh_ntk_workspace_bytes(h, b) for b in (1, 2, 45, 46, 512, 4096, 8192)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) > 3
    assert all(lib.dh_ntk_workspace_bytes(h, b) >= lib.dh_vjp_workspace_bytes(h, b) for b in (1, 45, 8192))
    lib.dh_destroy(h)


@pytest.mark.parametrize("kw", [dict(orbital_type="sparse"), dict(network_type="laughlin")])
def test_unsupported_handles_are_rejected(kw):
    if "network_type" in kw:
        lib, spec, h = make_handle("C1", nspins=(3, 0), flux=6, **kw)
    else:
        lib, spec, h = make_handle("C1", **kw)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dh_ntk(h, p, 1, p, p, None, p, 1 << 40, None) == DH_EINVAL
    assert len(lib.dh_last_error()) > 0
    assert lib.dh_ntk_tile_walkers(h) == 0
    lib.dh_destroy(h)


def test_argument_checks_precede_any_device_call():
    """A null T and a workspace one byte short are refused on a machine without a GPU (and
    with no parameters uploaded): the checks touch no device."""
    lib, spec, h = make_handle("C1")
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.dh_ntk_workspace_bytes(h, 5)
    assert lib.dh_ntk(h, p, 5, p, None, None, p, need, None) == DH_EINVAL
    assert lib.dh_ntk(h, p, 5, None, p, None, p, need, None) == DH_EINVAL
    assert lib.dh_ntk(h, p, 0, p, p, None, p, need, None) == DH_EINVAL
    assert lib.dh_ntk(None, p, 5, p, p, None, p, need, None) == DH_EINVAL
    assert lib.dh_ntk(h, p, 5, p, p, None, p, need - 1, None) == DH_ENOMEM
    assert b"one chunk" in lib.dh_last_error()
    assert lib.dh_ntk(h, p, 5, p, p, None, None, need, None) == DH_ENOMEM
    lib.dh_destroy(h)


def test_config_accepts_minsr():
    cfg = Config.from_dict({"optim": {"optimizer": "minsr"}})
    assert OptimizerName(cfg.optim.optimizer) == OptimizerName.minsr
    m = cfg.optim.minsr
    assert (m.lr.rate, m.damping, m.norm_constraint) == (0.05, 1e-3, 1e-3)
    cfg = Config.from_dict({"optim": {"optimizer": "minsr", "minsr": {"damping": 0.1, "lr": {"rate": 0.2}}}})
    assert cfg.optim.minsr.damping == 0.1 and cfg.optim.minsr.lr.rate == 0.2 and cfg.optim.minsr.lr.delay == 2000.0


def test_minsr_refuses_more_than_one_rank(monkeypatch):
    monkeypatch.setattr(constants, "world_size", lambda: 2)
    cfg = Config.from_dict({"optim": {"optimizer": "minsr"}})
    with pytest.raises(NotImplementedError, match="rank"):
        optimizers.make_optimizer_step(cfg, None)


def test_minsr_state_roundtrip():
    st = optimizers.MinsrState()
    st.step = 7
    d = {k: np.asarray(v) for k, v in st.state_dict().items()}
    assert set(d) == {"step"}
    st2 = optimizers.MinsrState()
    st2.load_state_dict(d)
    assert st2.step == 7


class _DenseNet:
    """A stand-in with an explicit Jacobian: ntk / vjp as the Psiformer serves them."""

    def __init__(self, Jre, Jim, bad):
        self.Jre, self.Jim, self.bad = Jre, Jim, bad

    def _rows(self, ct):
        B = self.Jre.shape[0]
        k = ct.shape[0] // B
        J = torch.cat([self.Jre] * k) * ct[:, :1].double() + torch.cat([self.Jim] * k) * ct[:, 1:].double()
        J[torch.cat([self.bad] * k)] = 0.0
        return J

    def ntk(self, params, data, ct, logpsi=None):
        J = self._rows(ct)
        if logpsi is not None:
            logpsi.zero_()
            logpsi[torch.cat([self.bad] * (ct.shape[0] // self.Jre.shape[0])), 0] = -float("inf")
        return (J @ J.t()).float()

    def vjp(self, params, data, ct):
        out = type("G", (), {})()
        out.flat = self._rows(ct).sum(0)
        return out


def test_minsr_direction_equals_parameter_space_solve():
    """(O~^T O~ + lambda)^-1 2 O~^T eps~ in parameter space == the sample-space form the step
    takes, with one NaN diff and one walker of non-finite log psi dropped from the centring."""
    g = torch.Generator().manual_seed(3)
    B, P, lam = 9, 40, 0.3
    Jre = torch.randn(B, P, generator=g, dtype=torch.float64)
    Jim = torch.randn(B, P, generator=g, dtype=torch.float64)
    diff = torch.randn(B, 2, generator=g, dtype=torch.float64)
    diff[4] = float("nan")
    bad = torch.zeros(B, dtype=torch.bool)
    bad[7] = True
    net = _DenseNet(Jre, Jim, bad)
    delta = optimizers.minsr_direction(net, None, torch.zeros(B, 3, 2), diff.float(), lam).flat
    v = torch.ones(B, dtype=torch.float64)
    v[4] = v[7] = 0.0
    n = v.sum()
    Cm = torch.diag(v) - torch.outer(v, v) / n
    Ot = torch.cat([Cm @ Jre, Cm @ Jim]) / n.sqrt()
    eps = torch.cat([torch.nan_to_num(diff.float().double()[:, 0]) * v, torch.nan_to_num(diff.float().double()[:, 1]) * v]) / n.sqrt()
    ref = torch.linalg.solve(Ot.t() @ Ot + lam * torch.eye(P, dtype=torch.float64), 2 * Ot.t() @ eps)
    # the stand-in's Gram matrix passes through float32, as dh_ntk's does
    assert (delta - ref).abs().max() <= 1e-5 * ref.abs().max()
