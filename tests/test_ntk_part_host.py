"""Sharded MinSR without a GPU: the host-side contract of dh_ntk_part, dh_ntk_mirror,
dh_ntk_owner and dh_minsr_matrix (exports, the ownership rule, argument checks that come before
any device call), the ``optim.minsr.sharded`` flag and the guard it lifts."""

from __future__ import annotations

import ctypes as C

import pytest

from deephall_amd import _lib, constants, optimizers
from deephall_amd.config import Config
from test_ntk_host import DH_EINVAL, DH_ENOMEM, make_handle

NEW = ("dh_ntk_part", "dh_ntk_mirror", "dh_ntk_owner", "dh_minsr_matrix_workspace_bytes", "dh_minsr_matrix")


def test_library_exports_the_new_symbols():
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS


@pytest.mark.parametrize("name", ["C1", "C2", "C4", "MIX"])
def test_owner_rule(name):
    """owner(w) = (w / tile walkers) % nparts: one owner in [0, nparts) for every walker."""
    lib, spec, h = make_handle(name)
    tw = lib.dh_ntk_tile_walkers(h)
    assert tw >= 1
    for nparts in (1, 2, 3, 8):
        for w in range(4 * tw + 1):
            o = lib.dh_ntk_owner(h, w, nparts)
            assert o == (w // tw) % nparts, (w, nparts)
            assert 0 <= o < nparts
    assert lib.dh_ntk_owner(h, -1, 2) == -1 and lib.dh_ntk_owner(h, 0, 0) == -1
    assert lib.dh_ntk_owner(None, 0, 2) == -1
    lib.dh_destroy(h)


@pytest.mark.parametrize("kw", [dict(orbital_type="sparse"), dict(network_type="laughlin")])
def test_owner_of_unsupported_handles(kw):
    if "network_type" in kw:
        lib, spec, h = make_handle("C1", nspins=(3, 0), flux=6, **kw)
    else:
        lib, spec, h = make_handle("C1", **kw)
    assert lib.dh_ntk_owner(h, 0, 2) == -1
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dh_ntk_part(h, p, 1, p, p, None, p, 1 << 40, 0, 1, None) == DH_EINVAL
    lib.dh_destroy(h)


def test_part_argument_checks_precede_any_device_call():
    """Refused on a machine without a GPU and with no parameters uploaded."""
    lib, spec, h = make_handle("C1")
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.dh_ntk_workspace_bytes(h, 5)
    assert lib.dh_ntk_part(h, p, 5, p, p, None, p, need, -1, 2, None) == DH_EINVAL
    assert b"part" in lib.dh_last_error()
    assert lib.dh_ntk_part(h, p, 5, p, p, None, p, need, 2, 2, None) == DH_EINVAL
    assert lib.dh_ntk_part(h, p, 5, p, p, None, p, need, 0, 0, None) == DH_EINVAL
    assert lib.dh_ntk_part(h, p, 5, p, p, None, p, need, 0, -3, None) == DH_EINVAL
    assert lib.dh_ntk_part(h, p, 5, p, None, None, p, need, 0, 2, None) == DH_EINVAL
    assert lib.dh_ntk_part(None, p, 5, p, p, None, p, need, 0, 2, None) == DH_EINVAL
    assert lib.dh_ntk_part(h, p, 5, p, p, None, p, need - 1, 0, 2, None) == DH_ENOMEM
    assert b"one chunk" in lib.dh_last_error()
    assert lib.dh_ntk_part(h, p, 5, p, p, None, None, need, 1, 2, None) == DH_ENOMEM
    assert lib.dh_ntk_mirror(None, 5, None) == DH_EINVAL
    assert lib.dh_ntk_mirror(p, 0, None) == DH_EINVAL
    lib.dh_destroy(h)


def test_minsr_matrix_argument_checks():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    need = lib.dh_minsr_matrix_workspace_bytes(6)
    assert need >= 8 * (2 * 12 + 5)  # row sums [2 Bg][2], g [4], n
    assert lib.dh_minsr_matrix_workspace_bytes(0) == 0
    assert lib.dh_minsr_matrix_workspace_bytes(4096) > lib.dh_minsr_matrix_workspace_bytes(70) > need
    assert lib.dh_minsr_matrix(None, p, 6, 1e-3, p, p, need, None) == DH_EINVAL
    assert lib.dh_minsr_matrix(p, None, 6, 1e-3, p, p, need, None) == DH_EINVAL
    assert lib.dh_minsr_matrix(p, p, 6, 1e-3, None, p, need, None) == DH_EINVAL
    assert lib.dh_minsr_matrix(p, p, 0, 1e-3, p, p, need, None) == DH_EINVAL
    assert lib.dh_minsr_matrix(p, p, 6, 1e-3, p, p, need - 1, None) == DH_ENOMEM
    assert b"workspace" in lib.dh_last_error()
    assert lib.dh_minsr_matrix(p, p, 6, 1e-3, p, None, need, None) == DH_ENOMEM


def test_config_reads_sharded():
    assert Config.from_dict({"optim": {"optimizer": "minsr"}}).optim.minsr.sharded is False
    cfg = Config.from_dict({"optim": {"optimizer": "minsr", "minsr": {"sharded": True, "damping": 0.1}}})
    assert cfg.optim.minsr.sharded is True and cfg.optim.minsr.damping == 0.1


def test_sharded_lifts_the_rank_guard(monkeypatch):
    monkeypatch.setattr(constants, "world_size", lambda: 2)
    cfg = Config.from_dict({"optim": {"optimizer": "minsr", "minsr": {"sharded": True}}})
    with pytest.raises(TypeError, match="Psiformer"):
        optimizers.make_optimizer_step(cfg, None)
    cfg = Config.from_dict({"optim": {"optimizer": "minsr"}})
    with pytest.raises(NotImplementedError, match="sharded"):
        optimizers.make_optimizer_step(cfg, None)
