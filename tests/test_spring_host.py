"""SPRING without a GPU: dh_ntk_jvp's host-side contract (exports, header, workspace, argument
checks that come before any device call), the ``momentum`` config entry, the optimizer state's
round trip with and without a stored direction, and the step's linear algebra against a
parameter-space solve on a dense stand-in Jacobian."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from deephall_amd import _lib, optimizers
from deephall_amd.config import Config
from test_ntk_host import DH_EINVAL, DH_ENOMEM, _DenseNet, make_handle


def test_exports_and_header():
    lib = _lib.load()
    txt = (Path(__file__).resolve().parents[1] / "include" / "deephall_amd.h").read_text()
    for s in ("dh_ntk_jvp_workspace_bytes", "dh_ntk_jvp"):
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS
        assert re.search(rf"\b{s}\(", txt), s


def jvp(lib, h, p, B, ct, v, T, jv, ws, ws_bytes, part=0, nparts=1):
    return lib.dh_ntk_jvp(h, p, B, ct, v, T, jv, None, ws, ws_bytes, part, nparts, None)


def test_argument_checks_precede_any_device_call():
    """Refused on a machine without a GPU and with no parameters uploaded: the checks touch no
    device.  A null T is an argument error only with more than one part."""
    lib, spec, h = make_handle("C1")
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.dh_ntk_jvp_workspace_bytes(h, 5)
    assert jvp(lib, h, p, 5, p, None, p, p, p, need) == DH_EINVAL          # null v
    assert jvp(lib, h, p, 5, p, p, p, None, p, need) == DH_EINVAL          # null jv
    assert jvp(lib, h, p, 5, None, p, p, p, p, need) == DH_EINVAL          # null ct
    assert jvp(lib, h, p, 0, p, p, p, p, p, need) == DH_EINVAL
    assert jvp(lib, None, p, 5, p, p, p, p, p, need) == DH_EINVAL
    assert jvp(lib, h, p, 5, p, p, p, p, p, need, part=2, nparts=2) == DH_EINVAL
    assert jvp(lib, h, p, 5, p, p, None, p, p, need, part=0, nparts=2) == DH_EINVAL
    assert b"part 0 of 1" in lib.dh_last_error()
    # null T, one part: past the argument checks, stopped by the workspace and then by the state
    assert jvp(lib, h, p, 5, p, p, None, p, p, need - 1) == DH_ENOMEM
    assert b"one chunk" in lib.dh_last_error()
    rc = jvp(lib, h, p, 5, p, p, None, p, p, need)
    assert rc not in (0, DH_EINVAL, DH_ENOMEM)
    assert b"parameters" in lib.dh_last_error()
    assert jvp(lib, h, p, 5, p, p, p, p, p, need - 1) == DH_ENOMEM
    assert jvp(lib, h, p, 5, p, p, p, p, None, need) == DH_ENOMEM
    lib.dh_destroy(h)


@pytest.mark.parametrize("kw", [dict(orbital_type="sparse"), dict(network_type="laughlin")])
def test_unsupported_handles_are_rejected(kw):
    if "network_type" in kw:
        lib, spec, h = make_handle("C1", nspins=(3, 0), flux=6, **kw)
    else:
        lib, spec, h = make_handle("C1", **kw)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert jvp(lib, h, p, 1, p, p, p, p, p, 1 << 40) == DH_EINVAL
    assert len(lib.dh_last_error()) > 0
    assert lib.dh_ntk_jvp_workspace_bytes(h, 4) == 0
    lib.dh_destroy(h)


@pytest.mark.parametrize("name", ["C1", "C2", "MIX"])
def test_workspace_covers_dh_ntk(name):
    lib, spec, h = make_handle(name)
    for b in (1, 45, 46, 8192):
        assert lib.dh_ntk_jvp_workspace_bytes(h, b) >= lib.dh_ntk_workspace_bytes(h, b) > 0
    lib.dh_destroy(h)


def test_config_momentum():
    assert Config.from_dict({"optim": {"optimizer": "minsr"}}).optim.minsr.momentum == 0.0
    cfg = Config.from_dict({"optim": {"optimizer": "minsr", "minsr": {"momentum": 0.9}}})
    assert cfg.optim.minsr.momentum == 0.9 and cfg.optim.minsr.damping == 1e-3
    for bad in (1.0, -0.1):
        cfg = Config.from_dict({"optim": {"optimizer": "minsr", "minsr": {"momentum": bad}}})
        with pytest.raises(ValueError, match="momentum"):
            optimizers.make_optimizer_step(cfg, None)


def test_state_roundtrip():
    st = optimizers.MinsrState()
    st.step = 7
    assert set(st.state_dict()) == {"step"}
    prev = torch.arange(6, dtype=torch.float32)
    st = optimizers.MinsrState(prev.clone())
    st.step = 3
    d = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in st.state_dict().items()}
    assert set(d) == {"step", "prev"}
    st2 = optimizers.MinsrState(torch.zeros(6))
    st2.load_state_dict(d)
    assert st2.step == 3 and torch.equal(st2.prev, prev)


class _DenseNetJvp(_DenseNet):
    """test_ntk_host's stand-in, extended by the Jacobian-vector product as the Psiformer serves it."""

    def jvp(self, params, data, ct, v, logpsi=None):
        return (self._rows(ct) @ v.double()).float()

    def ntk_jvp(self, params, data, ct, v, logpsi=None, part=0, nparts=1, mirror=True):
        return self.ntk(params, data, ct, logpsi=logpsi), self.jvp(params, data, ct, v)


def _problem():
    g = torch.Generator().manual_seed(3)
    B, P, lam = 9, 40, 0.3
    Jre = torch.randn(B, P, generator=g, dtype=torch.float64)
    Jim = torch.randn(B, P, generator=g, dtype=torch.float64)
    diff = torch.randn(B, 2, generator=g, dtype=torch.float64)
    diff[4] = float("nan")
    bad = torch.zeros(B, dtype=torch.bool)
    bad[7] = True
    prev = torch.randn(P, generator=g, dtype=torch.float64)
    return B, P, lam, Jre, Jim, diff, bad, prev


def test_spring_direction_equals_parameter_space_solve():
    """(O~^T O~ + lambda) phi = 2 O~^T eps~ + lambda mu phi_prev in parameter space == the
    sample-space form the step takes (one NaN diff, one walker of non-finite log psi, mu = 0.9),
    within test_minsr_direction_equals_parameter_space_solve's 1e-5 of max |phi|: the stand-in's
    Gram matrix and Jacobian-vector products pass through float32, as the library's do."""
    B, P, lam, Jre, Jim, diff, bad, prev = _problem()
    mu = 0.9
    net = _DenseNetJvp(Jre, Jim, bad)
    phi = optimizers.minsr_direction(net, None, torch.zeros(B, 3, 2), diff.float(), lam, prev=prev, momentum=mu).flat
    v = torch.ones(B, dtype=torch.float64)
    v[4] = v[7] = 0.0
    n = v.sum()
    Cm = torch.diag(v) - torch.outer(v, v) / n
    Ot = torch.cat([Cm @ Jre, Cm @ Jim]) / n.sqrt()
    d64 = torch.nan_to_num(diff.float().double())
    eps = torch.cat([d64[:, 0] * v, d64[:, 1] * v]) / n.sqrt()
    ref = torch.linalg.solve(Ot.t() @ Ot + lam * torch.eye(P, dtype=torch.float64), 2 * Ot.t() @ eps + lam * mu * prev)
    minsr = torch.linalg.solve(Ot.t() @ Ot + lam * torch.eye(P, dtype=torch.float64), 2 * Ot.t() @ eps)
    assert (ref - minsr).abs().max() > 1e-2 * ref.abs().max()  # the momentum term matters here
    assert (phi - ref).abs().max() <= 1e-5 * ref.abs().max()


def test_without_prev_or_momentum_it_is_minsr():
    B, P, lam, Jre, Jim, diff, bad, prev = _problem()
    x = torch.zeros(B, 3, 2)
    ref = optimizers.minsr_direction(_DenseNet(Jre, Jim, bad), None, x, diff.float(), lam).flat
    net = _DenseNetJvp(Jre, Jim, bad)
    assert torch.equal(optimizers.minsr_direction(net, None, x, diff.float(), lam, prev=None, momentum=0.9).flat, ref)
    assert torch.equal(optimizers.minsr_direction(net, None, x, diff.float(), lam, prev=prev, momentum=0.0).flat, ref)
