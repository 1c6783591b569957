"""The sharded Gram matrix (dh_ntk_part, dh_ntk_mirror, dh_ntk_owner) and the fused solve matrix
(dh_minsr_matrix) on the MI355X, in one process: the parts of T have disjoint support that obeys
the ownership rule and add up, bit for bit, to dh_ntk's T; dh_minsr_matrix against the float64
torch assembly of optimizers.minsr_direction; minsr_direction_sharded at world size 1 against
minsr_direction.

Shapes: test_gpu_ntk.case, B = 2 * tile walkers + 3 — three dense tile rows, the last partial,
and owners that change inside the one 128-walker tile of the per-walker-row launches.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from deephall_amd.optimizers import minsr_direction, minsr_direction_sharded, minsr_matrix
from helpers import make_params, make_walkers, oracle_config, to_device_params
from test_gpu_ntk import GATE_X, NAMES, case
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
_parts = {}


def parts_of(name, nparts, cuda):
    """Every part of T for one config and part count, computed once (upper triangle, no mirror)."""
    if (name, nparts) not in _parts:
        c = case(name, cuda)
        _parts[name, nparts] = [c["model"].ntk(c["params"], c["xd"], c["ctd"], part=p, nparts=nparts, mirror=False)
                                for p in range(nparts)]
    return _parts[name, nparts]


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_parts_have_disjoint_owned_support(cuda, name, nparts):
    c = case(name, cuda)
    B, model = c["B"], c["model"]
    parts = parts_of(name, nparts, cuda)
    owner = torch.tensor([model.ntk_owner(cuda, w, nparts) for w in range(B)], device=cuda)
    assert owner.tolist() == [(w // c["tw"]) % nparts for w in range(B)]
    upper = torch.triu(torch.ones(B, B, dtype=torch.bool, device=cuda))
    count = torch.zeros(B, B, dtype=torch.int32, device=cuda)
    for p, Tp in enumerate(parts):
        nz = Tp != 0
        count += nz.int()
        allowed = upper & (owner == p)[:, None]
        assert not (nz & ~allowed).any(), (name, nparts, p)
        # inside its support a part holds exactly dh_ntk's entries
        assert torch.equal(Tp[allowed], c["T"][allowed])
        assert nz.any()
    assert int(count.max()) == 1
    # the union of the supports is the support of the whole upper triangle
    assert torch.equal(count.bool(), (c["T"] != 0) & upper)


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_sum_of_parts_mirrored_is_ntk(cuda, name, nparts):
    c = case(name, cuda)
    parts = parts_of(name, nparts, cuda)
    for order in (range(nparts), reversed(range(nparts))):
        S = torch.zeros_like(c["T"])
        for p in order:
            S += parts[p]
        assert not torch.equal(S, c["T"])  # the lower triangle is still empty
        assert torch.equal(c["model"].ntk_mirror(S), c["T"])


@pytest.mark.parametrize("name", NAMES)
def test_one_part_of_one_and_repeats(cuda, name):
    c = case(name, cuda)
    model = c["model"]
    U = model.ntk(c["params"], c["xd"], c["ctd"], part=0, nparts=1, mirror=False)
    assert (torch.tril(U, -1) == 0).all()
    assert torch.equal(torch.triu(U), torch.triu(c["T"]))
    assert torch.equal(model.ntk_mirror(U.clone()), c["T"])
    assert torch.equal(model.ntk(c["params"], c["xd"], c["ctd"], part=0, nparts=1, mirror=True), c["T"])
    lp = torch.empty(c["B"], 2, device=cuda)
    again = model.ntk(c["params"], c["xd"], c["ctd"], logpsi=lp, part=1, nparts=3, mirror=False)
    assert torch.equal(again, parts_of(name, 3, cuda)[1])
    assert torch.equal(lp, c["lp"])  # log psi covers every walker, whatever the part
    with pytest.raises(RuntimeError, match="part"):
        model.ntk(c["params"], c["xd"], c["ctd"], part=3, nparts=3)


def assembly64(T, valid, damping):
    """A = C T C / n + damping I as optimizers.minsr_direction assembles it (float64 torch)."""
    M = T.shape[0]
    B = M // 2
    T = T.double()
    v = valid.double()
    n = v.sum().clamp(min=1.0)

    def centre(a):
        a = a * v
        return a - v * (a.sum(-1, keepdim=True) / n)

    T4 = centre(T.view(2, B, 2, B))
    T4 = centre(T4.permute(2, 3, 0, 1)).permute(2, 3, 0, 1)
    return T4.reshape(M, M) / n + float(damping) * torch.eye(M, dtype=torch.float64, device=T.device)


# Bg = 12 and 70: rows of 24 and 140 floats, the vector paths (float4 row sums, float2 assembly)
# with a tail in the thread loop and half boundaries at 12 and 70 (70 is inside a float4);
# Bg = 7: the scalar paths (2 Bg % 4 != 0)
@pytest.mark.parametrize("Bg", [12, 70, 7])
@pytest.mark.parametrize("name", ["C1", "MIX", "MIX32"])
def test_minsr_matrix(cuda, name, Bg):
    """max |A - A_ref| <= 1e-12 max |A_ref| against the float64 torch assembly: both sides are
    float64 sums of at most 140 terms in different orders — about 100 roundings of 1.1e-16.
    Measured on the MI355X: between 4.7e-17 and 2.4e-16 over the nine cases."""
    c = case(name, cuda)
    x = torch.tensor(make_walkers(Bg, c["ocfg"].nelec, seed=77), device=cuda)
    ct = torch.zeros(2 * Bg, 2, device=cuda)
    ct[:Bg, 0] = 1.0
    ct[Bg:, 1] = 1.0
    T = c["model"].ntk(c["params"], torch.cat([x, x]), ct)
    valid = torch.ones(Bg, dtype=torch.bool, device=cuda)
    bad = [3, Bg - 1]
    valid[bad] = False
    damping = 0.37
    A = minsr_matrix(T, valid, damping)
    ref = assembly64(T, valid, damping)
    err = float((A - ref).abs().max() / ref.abs().max())
    print(f"minsr_matrix {name} Bg = {Bg}: max |A - A_ref| / max |A_ref| = {err:.3e}")
    assert A.dtype == torch.float64 and torch.isfinite(A).all()
    assert err <= 1e-12
    assert torch.equal(A, A.t())
    for b in bad:
        for r in (b, Bg + b):
            e = torch.zeros(2 * Bg, dtype=torch.float64, device=cuda)
            e[r] = damping
            assert torch.equal(A[r], e) and torch.equal(A[:, r], e)
    assert torch.equal(minsr_matrix(T, valid, damping), A)
    # no valid walker at all: n = 1, A = damping I
    none = minsr_matrix(T, torch.zeros(Bg, dtype=torch.bool, device=cuda), damping)
    assert torch.equal(none, damping * torch.eye(2 * Bg, dtype=torch.float64, device=cuda))


def test_sharded_direction_on_one_rank(cuda):
    """test_gpu_minsr.py's case (MIX, one layer, B = 12, one NaN diff, lambda = the mean diagonal of
    the centred matrix, here read off dh_minsr_matrix with damping 0): minsr_direction_sharded
    without a process group against minsr_direction.  The two differ in the float64 rounding of
    the assembly alone, ahead of a solve of condition number at most 2 B + 1 = 25, so the
    direction passes the gate that file holds the same quantity to against the oracle,
    25 * 4 e0 + 3e-5, by a wide margin.  Measured on the MI355X: 0 (the float32 directions are
    identical; gate 6.79e-04)."""
    ocfg = oracle_config("MIX", num_layers=1)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    B = 12
    x = torch.tensor(make_walkers(B, ocfg.nelec, seed=5), device=cuda)
    diff = np.random.default_rng(23).standard_normal((B, 2)).astype(np.float32)
    diff[7] = np.nan
    diff = torch.tensor(diff, device=cuda)
    ct = torch.zeros(2 * B, 2, device=cuda)
    ct[:B, 0] = 1.0
    ct[B:, 1] = 1.0
    valid = ~torch.isnan(diff).any(dim=1)
    lam = float(torch.diagonal(minsr_matrix(model.ntk(params, torch.cat([x, x]), ct), valid, 0.0)).mean())
    ref = minsr_direction(model, params, x, diff, lam).flat.double()
    keep = {}
    got = minsr_direction_sharded(model, params, x, diff, lam, keep=keep).flat.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    gate = 25 * GATE_X * case("MIX", cuda)["e0"] + 3e-5
    print(f"sharded direction on one rank: err = {err:.3e}, gate = {gate:.3e}, lambda = {lam:.3e}")
    assert torch.isfinite(got).all() and float(ref.abs().max()) > 0
    assert err <= gate
    assert set(keep) == {"T", "A", "y"} and torch.equal(keep["T"], keep["T"].t())
