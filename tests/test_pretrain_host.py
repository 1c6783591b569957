"""Host-side checks of the fidelity pretraining (deephall_amd/pretrain.py): the config field,
the combination of partial sums on CPU tensors against numpy float64, and the three refusals
that must come before any device call.  No GPU: nothing here launches a kernel.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from deephall_amd import Config, _lib
from deephall_amd.config import LearningRate, Pretrain
from deephall_amd.pretrain import combine_partials, make_reference


def test_config_reads_pretrain():
    cfg = Config.from_dict({"seed": 1})
    assert isinstance(cfg.optim.pretrain, Pretrain)
    assert cfg.optim.pretrain.iterations == 0
    assert cfg.optim.pretrain.reference == "laughlin" and cfg.optim.pretrain.lr is None
    cfg = Config.from_dict({"seed": 1, "optim": {"pretrain": {"iterations": 7, "reference": "jain",
                                                              "lr": {"rate": 0.01, "delay": 50.0}}}})
    pre = cfg.optim.pretrain
    assert pre.iterations == 7 and pre.reference == "jain"
    assert isinstance(pre.lr, LearningRate) and pre.lr.rate == 0.01 and pre.lr.delay == 50.0 and pre.lr.decay == 1.0


def test_exports():
    lib = _lib.load()
    for s in ("dh_fidelity_partial", "dh_fidelity_residual"):
        assert hasattr(lib, s) and s in _lib.EXPORTS
    assert _lib.DH_NFID == 5
    # argument checks come before any device call
    assert lib.dh_fidelity_partial(None, None, 4, None, None) != 0
    assert b"null" in lib.dh_last_error()
    buf = np.zeros(16)
    p = buf.ctypes.data
    assert lib.dh_fidelity_partial(p, p, 0, p, None) != 0 and b"B >= 1" in lib.dh_last_error()
    assert lib.dh_fidelity_residual(p, p, 0, p, p, None) != 0 and b"B >= 1" in lib.dh_last_error()
    assert lib.dh_fidelity_residual(p, p, 3, None, p, None) != 0 and b"null" in lib.dh_last_error()


def numpy_combine(parts):
    """M = max m_r, S = sum S_r e^{m_r - M}, S2 = sum S2_r e^{2 (m_r - M)}, n = sum n_r over the
    partials with n_r > 0; F = |S|^2 / (n S2)."""
    live = [p for p in parts if p[4] > 0]
    if not live:
        return None
    M = max(p[0] for p in live)
    S = sum(complex(p[1], p[2]) * np.exp(p[0] - M) for p in live)
    S2 = sum(p[3] * np.exp(2.0 * (p[0] - M)) for p in live)
    n = sum(p[4] for p in live)
    return np.array([M, S.real, S.imag, S2, n]), abs(S) ** 2 / (n * S2)


def random_partials(rng, count, empty=()):
    """Partials as a batch could produce them (|S| <= n, 1 <= S2 <= n) with m spread over +-700."""
    parts = []
    for r in range(count):
        n = float(rng.integers(1, 5000))
        s2 = 1.0 + (n - 1.0) * rng.random()
        mod, arg = np.sqrt(s2) * rng.random(), rng.uniform(-np.pi, np.pi)
        parts.append([rng.uniform(-700.0, 700.0), mod * np.cos(arg), mod * np.sin(arg), s2, n])
        if r in empty:
            parts[-1] = [-np.inf, 0.0, 0.0, 0.0, 0.0]
    return np.array(parts, dtype=np.float64)


@pytest.mark.parametrize("count,empty", [(1, ()), (2, ()), (2, (0,)), (5, ()), (5, (1, 3))])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_combine_partials_against_numpy(count, empty, seed):
    parts = random_partials(np.random.default_rng(100 * count + seed), count, empty)
    total, fid = combine_partials(torch.tensor(parts, dtype=torch.float64))
    assert total.dtype == torch.float64 and tuple(total.shape) == (5,) and fid.dim() == 0
    assert_combined(total, fid, parts)


def assert_combined(total, fid, parts):
    """1e-12 relative: m and n exactly, S as a complex number, S2 and F."""
    ref_total, ref_f = numpy_combine(parts)
    got = total.numpy()
    assert got[0] == ref_total[0] and got[4] == ref_total[4]
    s_ref = complex(ref_total[1], ref_total[2])
    assert abs(complex(got[1], got[2]) - s_ref) <= 1e-12 * abs(s_ref)
    assert abs(got[3] - ref_total[3]) <= 1e-12 * ref_total[3]
    assert abs(float(fid) - ref_f) <= 1e-12 * ref_f


def test_combine_partials_close_shifts():
    """Partials whose m differ by a few units all contribute (the +-700 spread above leaves one
    dominant partial): same gate."""
    rng = np.random.default_rng(9)
    parts = random_partials(rng, 5)
    parts[:, 0] = 300.0 + rng.uniform(-3.0, 3.0, 5)
    total, fid = combine_partials(torch.tensor(parts))
    assert_combined(total, fid, parts)


def test_combine_partials_single_is_identity():
    parts = random_partials(np.random.default_rng(3), 1)
    total, _ = combine_partials(torch.tensor(parts[0]))
    assert np.array_equal(total.numpy(), parts[0])


def test_combine_partials_all_empty():
    parts = torch.tensor([[-np.inf, 0.0, 0.0, 0.0, 0.0]] * 3, dtype=torch.float64)
    total, fid = combine_partials(parts)
    assert float(total[4]) == 0.0 and float(total[0]) == -np.inf
    assert float(total[1]) == 0.0 and float(total[2]) == 0.0 and float(total[3]) == 0.0
    assert np.isnan(float(fid))


def base_config(**optim):
    return Config.from_dict({
        "batch_size": 16, "seed": 3, "system": {"nspins": (3, 0), "flux": 6},
        "network": {"psiformer": {"num_layers": 1, "num_heads": 1, "heads_dim": 4}},
        "optim": {"optimizer": "adam", "pretrain": {"iterations": 2}, **optim},
    })


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any attempt to obtain a device handle or to move a walker fails the test."""
    from deephall_amd.networks import psiformer

    def boom(*a, **k):
        raise AssertionError("a device call was made before the configuration was refused")

    monkeypatch.setattr(psiformer, "get_handle", boom)
    monkeypatch.setattr(psiformer.NativeHandle, "__init__", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)


def refused(cfg, match):
    from deephall_amd.pretrain import pretrain
    from deephall_amd.train import train

    with pytest.raises(ValueError, match=match):
        make_reference(cfg)
    with pytest.raises(ValueError, match=match):
        pretrain(cfg, None, None, None, None)
    with pytest.raises(ValueError, match=match):
        train(cfg)


def test_valid_config_builds_the_reference(no_gpu_calls):
    ref = make_reference(base_config())
    assert ref.spec.network_type == "laughlin" and ref.spec.flux == 6


def test_refuses_missing_trial_state(no_gpu_calls):
    """(3, 0) at flux 8: 2 Q1 = 4, and N = 3 is none of 2 Q1 + 1 (ground state), 2 Q1
    (quasihole), 2 Q1 + 2 (quasiparticle): dh_create itself refuses the Laughlin handle."""
    cfg = base_config()
    cfg.system.flux = 8
    refused(cfg, "no laughlin trial state at N = 3, flux = 8")
    jain = base_config()
    jain.optim.pretrain.reference = "jain"  # (3, 0) at flux 6: N != 4 Q1 + 4
    refused(jain, "no jain trial state")
    mr = base_config()
    mr.optim.pretrain.reference = "pfaffian"  # odd N
    refused(mr, "no pfaffian trial state")
    other = base_config()
    other.optim.pretrain.reference = "hartree-fock"
    refused(other, "reference must be one of")


def test_refuses_a_network_without_parameters(no_gpu_calls):
    cfg = base_config()
    cfg = dataclasses.replace(cfg, network=dataclasses.replace(cfg.network, type="laughlin"))
    refused(cfg, "trains a Psiformer")


def test_refuses_optimizer_none(no_gpu_calls):
    refused(base_config(optimizer="none"), "needs an optimizer")
    refused(base_config(optimizer=None), "needs an optimizer")
    from deephall_amd.optimizers import make_optimizer_step
    from deephall_amd import make_network

    cfg = base_config(optimizer="none")
    model = make_network(cfg.system, cfg.network)
    with pytest.raises(ValueError, match="needs an optimizer"):
        make_optimizer_step(cfg, model, residual=lambda params, data: None)
