"""Host-side checks of the overlap penalty (deephall_amd/orthogonal.py): the config field, the
exports, the combination of per-state partial sums on CPU tensors, checkpoint-entry resolution and
every refusal that must come before any device call.  No GPU: nothing here launches a kernel.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from deephall_amd import Config, _lib, make_network
from deephall_amd.config import Orthogonal
from deephall_amd.networks.psiformer import param_shapes
from deephall_amd.orthogonal import (FrozenPsiformer, combine_state_partials, load_checkpoint_params,
                                     make_orthogonal_residual, make_states, resolve_checkpoint)
from deephall_amd.pretrain import combine_partials
from test_pretrain_host import no_gpu_calls, random_partials  # noqa: F401  (a fixture)

NET = {"psiformer": {"num_layers": 1, "num_heads": 1, "heads_dim": 4}}


def base_config(states=({"type": "laughlin"},), **optim):
    return Config.from_dict({
        "batch_size": 16, "seed": 3, "system": {"nspins": (3, 0), "flux": 6}, "network": NET,
        "optim": {"optimizer": "adam", "orthogonal": {"states": list(states)}, **optim},
    })


def test_config_round_trip():
    cfg = Config.from_dict({"seed": 1})
    assert isinstance(cfg.optim.orthogonal, Orthogonal)
    assert cfg.optim.orthogonal.states == () and cfg.optim.orthogonal.penalty == 1.0
    entries = [{"type": "laughlin", "penalty": 2.0}, {"checkpoint": "runs/ground", "psiformer": {"num_layers": 2}}]
    cfg = Config.from_dict({"seed": 1, "optim": {"orthogonal": {"states": entries, "penalty": 0.5}}})
    orth = cfg.optim.orthogonal
    assert isinstance(orth.states, tuple) and list(orth.states) == entries and orth.penalty == 0.5
    assert orth.states[0] is not entries[0]  # the config owns its entries
    from deephall_amd.log import _plain

    again = Config.from_dict(_plain(cfg))  # what config.yml holds
    assert again.optim.orthogonal == orth


def test_defaults_leave_the_config_unchanged():
    """Every other field of Config() is what it is without the new key."""
    a, b = Config(seed=1), Config.from_dict({"seed": 1, "optim": {"orthogonal": {"states": [], "penalty": 1.0}}})
    assert a == b
    plain = dataclasses.asdict(a)
    assert plain["optim"].pop("orthogonal") == {"states": (), "penalty": 1.0}
    assert set(plain["optim"]) == {"iterations", "optimizer", "adam", "kfac", "minsr", "pretrain"}


def test_exports():
    lib = _lib.load()
    for s in ("dh_ortho_partial", "dh_ortho_residual"):
        assert hasattr(lib, s) and s in _lib.EXPORTS
    assert _lib.DH_ORTHO_MAX_STATES == 16
    buf = np.zeros(16)
    p = buf.ctypes.data
    # argument checks come before any device call
    assert lib.dh_ortho_partial(None, p, 4, 1, p, None) != 0 and b"null" in lib.dh_last_error()
    assert lib.dh_ortho_partial(p, p, 0, 1, p, None) != 0 and b"B >= 1" in lib.dh_last_error()
    for K in (0, 17, -1):
        assert lib.dh_ortho_partial(p, p, 4, K, p, None) != 0 and b"K" in lib.dh_last_error()
        assert lib.dh_ortho_residual(p, p, 4, K, p, p, None, p, None) != 0 and b"K" in lib.dh_last_error()
    assert lib.dh_ortho_residual(p, p, 0, 1, p, p, None, p, None) != 0 and b"B >= 1" in lib.dh_last_error()
    assert lib.dh_ortho_residual(p, p, 4, 1, p, None, None, p, None) != 0 and b"null" in lib.dh_last_error()
    assert lib.dh_ortho_residual(p, p, 4, 1, None, p, p, p, None) != 0 and b"null" in lib.dh_last_error()


@pytest.mark.parametrize("ranks,empty", [(1, ()), (2, ()), (2, (0,)), (4, (1, 3))])
def test_combine_state_partials_is_combine_partials_per_state(ranks, empty):
    K = 3
    rng = np.random.default_rng(17 + ranks)
    parts = np.stack([random_partials(rng, ranks, empty if k != 1 else ()) for k in range(K)], axis=1)  # [R, K, 5]
    parts[:, 2, 0] = 300.0 + rng.uniform(-3.0, 3.0, ranks)  # close shifts: every rank contributes
    if empty:
        parts[list(empty), 2] = [-np.inf, 0.0, 0.0, 0.0, 0.0]
    t = torch.tensor(parts, dtype=torch.float64)
    total, fid = combine_state_partials(t)
    assert total.dtype == torch.float64 and tuple(total.shape) == (K, 5) and tuple(fid.shape) == (K,)
    for k in range(K):
        tk, fk = combine_partials(t[:, k])
        assert torch.equal(total[k], tk) and torch.equal(fid[k], fk)
    if ranks == 1:
        assert torch.equal(total, t[0])  # one partial combines to itself


def test_combine_state_partials_empty_state():
    t = torch.tensor([[[0.5, 1.0, 0.0, 1.0, 1.0], [-np.inf, 0.0, 0.0, 0.0, 0.0]]] * 2, dtype=torch.float64)
    total, fid = combine_state_partials(t)
    assert float(fid[0]) == 1.0 and np.isnan(float(fid[1]))
    assert total[1].tolist() == [-np.inf, 0.0, 0.0, 0.0, 0.0]


# ---- states ------------------------------------------------------------------------------------

def write_checkpoint(path, cfg, seed, **replace):
    model = make_network(cfg.system, cfg.network)
    tree = model.init(seed, device="cpu")
    arrays = {"step": np.asarray(0), "mcmc_width": np.asarray(0.1), "data": np.zeros((4, 3, 2), np.float32)}
    arrays.update({f"params/{k}": v.numpy() for k, v in tree.items()})
    for k, v in replace.items():
        if v is None:
            arrays.pop(k)
        else:
            arrays[k] = v
    np.savez_compressed(path, **arrays)
    return tree


def test_checkpoint_resolution(tmp_path, no_gpu_calls):
    cfg = base_config()
    old = write_checkpoint(tmp_path / "ckpt_000002.npz", cfg, seed=1)
    new = write_checkpoint(tmp_path / "ckpt_000010.npz", cfg, seed=2)
    (tmp_path / "notes.npz").write_bytes(b"")
    assert resolve_checkpoint(tmp_path) == tmp_path / "ckpt_000010.npz"  # the newest of a directory
    assert resolve_checkpoint(tmp_path / "ckpt_000002.npz") == tmp_path / "ckpt_000002.npz"
    spec = make_network(cfg.system, cfg.network).spec
    assert torch.equal(load_checkpoint_params(tmp_path, spec).flat, new.flat)
    assert torch.equal(load_checkpoint_params(tmp_path / "ckpt_000002.npz", spec).flat, old.flat)
    assert not torch.equal(old.flat, new.flat)
    # the newest is the largest step number, not the last name: a step past the six-digit padding wins,
    # a hand-named file is passed over
    (tmp_path / "ckpt_best.npz").write_bytes(b"")
    assert resolve_checkpoint(tmp_path) == tmp_path / "ckpt_000010.npz"
    (tmp_path / "ckpt_1000000.npz").write_bytes(b"")
    assert resolve_checkpoint(tmp_path) == tmp_path / "ckpt_1000000.npz"
    (tmp_path / "ckpt_1000000.npz").unlink()

    cfg = base_config([{"type": "laughlin"}, {"checkpoint": str(tmp_path), "penalty": 0.25},
                       {"type": "psiformer", "checkpoint": str(tmp_path / "ckpt_000002.npz")}], )
    cfg.optim.orthogonal.penalty = 3.0
    states, penalties = make_states(cfg)
    assert penalties == [3.0, 0.25, 3.0]
    assert states[0].spec.network_type == "laughlin" and states[0].spec.flux == 6
    assert isinstance(states[1], FrozenPsiformer) and isinstance(states[2], FrozenPsiformer)
    assert torch.equal(states[1]._source.flat, new.flat) and torch.equal(states[2]._source.flat, old.flat)
    # the run's own architecture, a handle of its own each
    run = make_network(cfg.system, cfg.network).spec
    tags = set()
    for s in states[1:]:
        assert s.network.spec.handle_tag is not None and s.network.spec != run
        assert dataclasses.replace(s.network.spec, handle_tag=None) == run
        tags.add(s.network.spec.handle_tag)
    assert len(tags) == 2


def test_checkpoint_entry_overrides_the_architecture(tmp_path, no_gpu_calls):
    wide = base_config()
    wide.network.psiformer.heads_dim = 8
    write_checkpoint(tmp_path / "ckpt_000000.npz", wide, seed=1)
    cfg = base_config([{"checkpoint": str(tmp_path), "psiformer": {"heads_dim": 8}}])
    (state,), _ = make_states(cfg)
    assert state.network.spec.heads_dim == 8 and make_network(cfg.system, cfg.network).spec.heads_dim == 4
    with pytest.raises(ValueError, match=r"Dense_0/kernel has shape \(4, 8\) .*needs \(4, 4\)"):
        make_states(base_config([{"checkpoint": str(tmp_path)}]))


def refused(cfg, match):
    from deephall_amd.train import train

    with pytest.raises(ValueError, match=match):
        make_states(cfg)
    with pytest.raises(ValueError, match=match):
        train(cfg)


def test_refuses_too_many_states(no_gpu_calls):
    make_states(base_config([{"type": "laughlin"}] * 16))
    refused(base_config([{"type": "laughlin"}] * 17), "at most 16 states, got 17")


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), "much"])
def test_refuses_bad_penalties(no_gpu_calls, bad):
    refused(base_config([{"type": "laughlin", "penalty": bad}]), "state 0: penalty must be")
    cfg = base_config()
    cfg.optim.orthogonal.penalty = bad
    refused(cfg, "optim.orthogonal: penalty must be")
    model = make_network(cfg.system, cfg.network)
    with pytest.raises(ValueError, match="penalty must be"):
        make_orthogonal_residual(model, [model], [bad])


def test_refuses_unknown_types_and_malformed_entries(no_gpu_calls):
    refused(base_config([{"type": "hartree-fock"}]), "optim.orthogonal: state 0 has the unknown type 'hartree-fock'")
    refused(base_config([{"type": "laughlin"}, {"type": "psiformer"}]), "state 1: type psiformer needs a checkpoint")
    refused(base_config(["laughlin"]), "state 0 must be a dict")
    refused(base_config([{"type": "laughlin", "iterations": 3}]), "optim.orthogonal: state 0 must be a dict of type")
    refused(base_config([{"type": "jain", "checkpoint": "x"}]), "a checkpoint entry is a psiformer")


def test_refuses_unreadable_checkpoints(tmp_path, no_gpu_calls):
    refused(base_config([{"checkpoint": str(tmp_path / "absent.npz")}]), "state 0: checkpoint .*absent.npz does not exist")
    refused(base_config([{"checkpoint": str(tmp_path)}]), "state 0: no ckpt_\\*.npz in")
    (tmp_path / "ckpt_000001.npz").write_bytes(b"not an archive")
    refused(base_config([{"checkpoint": str(tmp_path)}]), "ckpt_000001.npz cannot be read")
    cfg = base_config()
    name = next(iter(param_shapes(make_network(cfg.system, cfg.network).spec)))
    write_checkpoint(tmp_path / "ckpt_000002.npz", cfg, seed=1, **{f"params/{name}": None})
    refused(base_config([{"checkpoint": str(tmp_path)}]), f"tensor params/{name} is missing")
    write_checkpoint(tmp_path / "ckpt_000003.npz", cfg, seed=1, **{"params/Jastrow_0/ee_par": np.zeros(2, np.float32)})
    refused(base_config([{"checkpoint": str(tmp_path)}]), r"tensor params/Jastrow_0/ee_par has shape \(2,\)")


def test_refuses_missing_trial_state(no_gpu_calls):
    """(3, 0) at flux 8 has no Laughlin state, (3, 0) at flux 6 no Jain or Moore-Read state: the
    library's own dh_create (host code) or the network's constructor refuses."""
    cfg = base_config()
    cfg.system.flux = 8
    refused(cfg, "state 0: no laughlin trial state at N = 3, flux = 8: ")
    refused(base_config([{"type": "laughlin"}, {"type": "jain"}]), "optim.orthogonal: state 1")
    refused(base_config([{"type": "pfaffian"}]), "optim.orthogonal: state 0")


def test_refuses_a_network_without_parameters(no_gpu_calls):
    cfg = base_config()
    cfg = dataclasses.replace(cfg, network=dataclasses.replace(cfg.network, type="laughlin"))
    refused(cfg, "trains a Psiformer")


def test_refuses_optimizer_none(no_gpu_calls):
    refused(base_config(optimizer="none"), "needs an optimizer")
    refused(base_config(optimizer=None), "needs an optimizer")


def test_residual_argument_checks(no_gpu_calls):
    cfg = base_config()
    model = make_network(cfg.system, cfg.network)
    with pytest.raises(ValueError, match="1 to 16 states"):
        make_orthogonal_residual(model, [], [])
    with pytest.raises(ValueError, match="2 states but 1 penalties"):
        make_orthogonal_residual(model, [model, model], [1.0])
    hook = make_orthogonal_residual(model, [model], [1.5])
    assert hook.keeps_energy and hook.penalties == (1.5,)
    assert not make_orthogonal_residual(model, [model], [1.5], energy=False).keeps_energy
