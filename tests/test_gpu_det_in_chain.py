"""The determinant tail of the last chain launch against the separate value kernel.

Where a log-psi pass ends in a chain launch that maps the orbitals and the value kernel would
put two walkers on a wave, the chain launch runs the value kernel's body (csrc/det_value.h) as
its tail on F rows still in LDS (TrunkRoute::det_in_chain, DESIGN.md §1 "Routes").  The tail
moves code without changing an operation, so every case here holds the two forms to bitwise
equality on the same handle, switching with dh_debug_set_det_in_chain.  Shapes: a dead half-wave
(B = 1), one full 16-walker tile, a tile plus one walker, partial last tiles, 32 walkers per tile
with two walker pairs per wave (N = 3), and two spin blocks with two determinants (wider F
rows, N = 4)."""

from __future__ import annotations

import contextlib
import ctypes as C
import functools

import pytest
import torch

from deephall_amd import _lib, config, make_network
from deephall_amd.mcmc import make_mcmc_step
from deephall_amd.networks.psiformer import _ptr, _stream
from deephall_amd.random import Key, PRNGKey
from deephall_amd.train import init_guess
from test_abi_host import GEMM_MODES, make_handle

gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def network(nspins, flux, ndets=1):
    net = config.Network()
    net.psiformer.determinants = ndets
    system = config.System(nspins=nspins, flux=flux)
    model = make_network(system, net)
    return model, model.init(PRNGKey(42), device="cuda")


@contextlib.contextmanager
def separate_form():
    """Every pass inside launches the value kernel on its own."""
    lib = _lib.load()
    old = lib.dh_debug_set_det_in_chain(0)
    try:
        yield
    finally:
        assert lib.dh_debug_set_det_in_chain(old) == 0


def bits(t):
    """The bit patterns (equal NaNs and signed zeros compare as what they are)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32)


def det_value_launches(h, fn):
    """Launches of the value-kernel class during fn (dh_profile_read), and fn's result.  The
    profiler times classes by events around launches, so a pass it records launches the value
    kernel on its own whatever the route says."""
    lib = h.lib
    lib.dh_profile_enable(h.h, 1)
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = (C.c_double * (4 * len(_lib.PROF_KINDS)))()
        assert lib.dh_profile_read(h.h, buf, 1) == len(_lib.PROF_KINDS)
    finally:
        lib.dh_profile_enable(h.h, 0)
    return int(buf[4 * _lib.PROF_KINDS.index("det_value")]), out


# (nspins, flux, ndets, B, the route carries the tail)
LOGPSI = [((6, 0), 15, 1, 1, True), ((6, 0), 15, 1, 16, True), ((6, 0), 15, 1, 17, True), ((6, 0), 15, 1, 40, True),
          ((3, 0), 2, 1, 33, True), ((2, 2), 3, 2, 25, True)]


@gpu
@pytest.mark.parametrize("nspins,flux,ndets,B,on", LOGPSI)
def test_logpsi_tail_equals_value_kernel(cuda, nspins, flux, ndets, B, on):
    model, params = network(nspins, flux, ndets)
    N = sum(nspins)
    x = init_guess(Key(4242), B, N, cuda, network=model)
    h = model.prepare(params, x.device)
    assert h.lib.dh_debug_det_in_chain(h.h, B, 0) == int(on)
    fused = model.apply(params, x).clone()
    n_prof, profiled = det_value_launches(h, lambda: model.apply(params, x).clone())
    with separate_form():
        assert h.lib.dh_debug_det_in_chain(h.h, B, 0) == 0
        sep = model.apply(params, x).clone()
    assert n_prof == 1  # recorded passes keep the value kernel's own launch
    assert torch.isfinite(sep).all()
    assert torch.equal(bits(fused), bits(sep))
    assert torch.equal(bits(profiled), bits(sep))


@gpu
@pytest.mark.parametrize("steps", [3, 0, 1])
def test_mcmc_tail_equals_value_kernel(cuda, steps):
    """Injected noise; steps = 0: the initial pass alone (epilogue off); steps = 1: the only move
    runs its accept without a next proposal."""
    nspins, B = (6, 0), 40
    model, params = network(nspins, 15)
    N = sum(nspins)
    x0 = init_guess(Key(77), B, N, cuda, network=model)
    noise = None
    if steps:
        g = torch.Generator(device="cpu").manual_seed(5)
        noise = torch.cat([torch.randn(steps, B, N, generator=g), torch.rand(steps, B, N + 1, generator=g)], -1).to(cuda)
    step = make_mcmc_step(model, batch_per_device=B, steps=steps)

    def run():
        x, _ = step(params, x0.clone(), Key(3, 9), 0.3, noise=noise)
        torch.cuda.synchronize()
        return x, step.last_lp.clone(), step.last_n_accept.clone()

    xa, lpa, na = run()
    with separate_form():
        xb, lpb, nb = run()
    assert torch.equal(bits(xa), bits(xb))
    assert torch.equal(bits(lpa), bits(lpb))
    assert torch.equal(na, nb)
    if steps == 3:  # the comparison is not between two idle chains
        assert 0 < int(na.sum()) < steps * B
    if steps == 0:
        assert torch.equal(xa, x0) and int(na.sum()) == 0


@gpu
def test_singular_walker_same_zero_pivot(cuda):
    """Two electrons at the same angles (tests/test_gpu_grad.py): two equal orbital rows cancel
    exactly in the elimination, the pivot is an exact zero and psi = 0, in both forms alike."""
    model, params = network((6, 0), 15)
    x = init_guess(Key(8), 6, 6, cuda, network=model)
    x[2, 1] = x[2, 0]
    fused = model.apply(params, x).clone()
    with separate_form():
        sep = model.apply(params, x).clone()
    assert not torch.isfinite(sep[2].real)  # psi = 0 for the coincident walker
    assert torch.isfinite(sep[[0, 1, 3, 4, 5]]).all()
    assert torch.equal(bits(fused), bits(sep))


@gpu
def test_debug_trunk_keeps_f_with_the_tail(cuda):
    """dh_debug_trunk on a route that carries the tail runs the tail's launch and still leaves F
    (and the trunk's h) in the workspace, equal to the separate form's."""
    B, N, D = 17, 6, 256
    orb_cols, ld_orb = 2 * 16 * N, 256  # one spin block, M = 2Q + 1 = 16, one determinant; padded to 128
    model, params = network((6, 0), 15)
    x = init_guess(Key(4242), B, N, cuda, network=model)
    h = model.prepare(params, x.device)
    off = h.lib.dh_debug_f_offset(h.h, B, 0)

    def run():
        ws = h.workspace(h.lib.dh_workspace_bytes(h.h, B, 0))
        ws.zero_()
        rc = h.lib.dh_debug_trunk(h.h, _ptr(x), B, 0, _ptr(ws), ws.numel(), _stream(x.device))
        torch.cuda.synchronize()
        assert rc == 0, h.lib.dh_last_error()
        f = ws.view(torch.float32)
        return (f[off:off + B * N * ld_orb].view(B * N, ld_orb)[:, :orb_cols].clone(),
                f[:B * N * D].view(B * N, D).clone())

    assert h.lib.dh_debug_det_in_chain(h.h, B, 0) == 1
    Fa, ha = run()
    with separate_form():
        Fb, hb = run()
    assert Fb.abs().max().item() > 0 and torch.isfinite(Fb).all()
    assert torch.equal(bits(Fa), bits(Fb))
    assert torch.equal(bits(ha), bits(hb))


def test_route_member_host():
    """TrunkRoute::det_in_chain on the host (no device call): on for the flagship log-psi pass;
    off for the channel pass, in exact-f32 mode, at N = 10 and 20 (no two-walker value kernel, no
    whole walkers in 96 rows) and past the chain's 65,536-row threshold at N = 6."""

    def member(mode, op, B, **kw):
        lib, _, h, rc = make_handle(**kw)
        assert rc == 0
        assert lib.dh_set_gemm_mode(h, GEMM_MODES[mode]) == 0
        out = lib.dh_debug_det_in_chain(h, B, op)
        lib.dh_destroy(h)
        return out

    assert member("x6all", 0, 4096) == 1
    assert member("x6all", 1, 8) == 0
    assert member("f32", 0, 4096) == 0
    assert member("x6", 0, 4096) == 0  # log-psi rows take the split-bf16 chain in x6all only
    assert member("x6all", 0, 4096, nspins=(10, 0), flux=23) == 0
    assert member("x6all", 0, 4096, nspins=(20, 0), flux=57) == 0
    assert member("x6all", 0, 65535 // 6) == 1
    assert member("x6all", 0, -(-65536 // 6)) == 0
    lib = _lib.load()
    old = lib.dh_debug_set_det_in_chain(0)
    try:
        assert old == 1
        assert member("x6all", 0, 4096) == 0
    finally:
        assert lib.dh_debug_set_det_in_chain(old) == 0
    assert member("x6all", 0, 4096) == 1
