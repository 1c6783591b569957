"""The launches a pass makes are the ones its route names (csrc/trunk_route.cpp, DESIGN.md §1
"Routes"; the route values themselves are pinned on the host by test_abi_host.py).

One dh_logpsi or one single-chunk dh_local_energy per case under the profiler; the per-class launch
counts of dh_profile_read are compared with a literal table recorded on commit 8b3da0d, the last
one whose run_trunk chose its kernels through inline booleans — not produced by the code under
test.  The shapes are the smallest that reach every layer form, both sides of the 65,536-row chain
threshold, and the envelope-first and precontracted determinant stages."""

from __future__ import annotations

import ctypes as C
import functools

import pytest
import torch

from deephall_amd import _lib, config, hamiltonian, make_network
from deephall_amd.networks import psiformer as PS
from deephall_amd.networks.psiformer import _ptr, _stream
from deephall_amd.random import Key, PRNGKey
from deephall_amd.train import init_guess

pytestmark = pytest.mark.gpu

FLUX = {3: 2, 5: 12, 6: 15, 8: 21, 10: 23, 12: 33, 20: 57}
assert _lib.PROF_KINDS == ["gemm", "attention", "layernorm", "input", "det_value", "det_energy", "mcmc",
                           "gemm_ch", "attention_ch", "layernorm_ch", "input_ch", "layer1_ch"]

# log psi (classes 0 .. 6): chain = 2 launches + attention where it is not in the chain prologue
# (N = 5, 12); past the threshold 2 x 2 LayerNorm GEMMs, layer 2's q|k|v and the orbital map
LOGPSI = {
    (3, 8): [2, 1, 0, 1, 1, 0, 0], (5, 8): [2, 2, 0, 1, 1, 0, 0], (6, 8): [2, 1, 0, 1, 1, 0, 0],
    (10, 8): [2, 1, 0, 1, 1, 0, 0], (12, 8): [2, 2, 0, 1, 1, 0, 0], (20, 8): [2, 1, 0, 1, 1, 0, 0],
    (6, 10922): [2, 1, 0, 1, 1, 0, 0], (6, 10923): [6, 2, 0, 1, 1, 0, 0],
}
# local energy: (det_energy, gemm_ch, attention_ch, layernorm_ch, input_ch, layer1_ch)
FUSED = [1, 4, 2, 0, 1, 1]     # gemm_lnch: layer 1 whole, then q|k|v, the pair, the orbital map
SEPARATE = [1, 6, 2, 4, 1, 0]  # per layer two GEMMs and two LayerNorms, q|k|v, the orbital map / envelope first
L1CH = [1, 4, 2, 2, 1, 1]      # layer1_ch, then q|k|v, two GEMMs, two LayerNorms, envelope first / orbital map
ENERGY = {
    (3, "x6all"): FUSED, (3, "x6all_unfused"): SEPARATE, (3, "f32"): SEPARATE,
    (6, "x6all"): FUSED, (6, "x6all_unfused"): SEPARATE, (6, "f32"): SEPARATE,
    (8, "x6all"): SEPARATE, (8, "x6all_unfused"): SEPARATE, (8, "f32"): SEPARATE,
    (10, "x6all"): L1CH, (10, "x6all_unfused"): SEPARATE, (10, "f32"): L1CH,
    (20, "x6all"): L1CH, (20, "x6all_unfused"): SEPARATE, (20, "f32"): L1CH,
}


@functools.lru_cache(maxsize=None)
def network(N, ndets=1):
    net = config.Network()
    net.psiformer.determinants = ndets
    system = config.System(nspins=(N, 0), flux=FLUX[N])
    model = make_network(system, net)
    return model, system, model.init(PRNGKey(42), device="cuda")


@pytest.fixture
def gemm_mode():
    yield PS.set_gemm_mode
    PS.set_gemm_mode("x6all")


def launch_counts(h, fn):
    lib = h.lib
    lib.dh_profile_enable(h.h, 1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = (C.c_double * (4 * len(_lib.PROF_KINDS)))()
        assert lib.dh_profile_read(h.h, buf, 1) == len(_lib.PROF_KINDS)
    finally:
        lib.dh_profile_enable(h.h, 0)
    return [int(buf[4 * i]) for i in range(len(_lib.PROF_KINDS))]


@pytest.mark.parametrize("N,B", sorted(LOGPSI))
def test_logpsi_launches(cuda, N, B):
    model, _, params = network(N)
    x = init_guess(Key(4242), B, N, cuda, network=model)
    h = model.prepare(params, x.device)
    got = launch_counts(h, lambda: model.apply(params, x))
    assert got == LOGPSI[(N, B)] + [0] * 5


def energy_counts(N, B, ndets=1):
    model, system, params = network(N, ndets)
    x = init_guess(Key(4242), B, N, torch.device("cuda"), network=model)
    h = model.prepare(params, x.device)
    e_l = hamiltonian.local_energy(model.apply, system)  # workspace for the whole batch: one chunk
    got = launch_counts(h, lambda: e_l.raw(params, x))
    assert got[:5] == [0] * 5 and got[6] == 0
    return [got[5]] + got[7:]


@pytest.mark.parametrize("N,mode", sorted(ENERGY))
def test_local_energy_launches(cuda, gemm_mode, N, mode):
    gemm_mode(mode)
    assert energy_counts(N, 8) == ENERGY[(N, mode)]


def test_local_energy_launches_two_determinants(cuda):
    """N = 10 with two determinants: not envelope first, so the orbital map runs (the fourth GEMM)
    and the determinants take the precontracted PhiC."""
    assert energy_counts(10, 4, ndets=2) == L1CH


def test_debug_trunk_refused_without_f(cuda):
    """dh_debug_trunk / dh_debug_f_offset for the local energy: accepted at N = 6, refused at N = 10
    (envelope first: no F over the channel rows, the q|k|v buffer is sized for S, FS, E2, Weff)."""
    for N, ok in ((6, True), (10, False)):
        model, _, params = network(N)
        x = init_guess(Key(4242), 2, N, cuda, network=model)
        h = model.prepare(params, x.device)
        ws = h.workspace(h.lib.dh_workspace_bytes(h.h, 2, 1))
        rc = h.lib.dh_debug_trunk(h.h, _ptr(x), 2, 1, _ptr(ws), ws.numel(), _stream(x.device))
        off = h.lib.dh_debug_f_offset(h.h, 2, 1)
        torch.cuda.synchronize()
        if ok:
            assert rc == 0, h.lib.dh_last_error()
            assert 0 < off < ws.numel() // 4
        else:
            assert rc == -1 and b"envelope first" in h.lib.dh_last_error()
            assert off == C.c_size_t(-1).value
        # log psi maps F on every route
        assert h.lib.dh_debug_f_offset(h.h, 2, 0) < ws.numel() // 4
