"""GPU parity of the HIP path (through the C ABI) against the float64 oracle.

Tolerances (f32 kernels vs the f64 restatement; the reference itself is f32):
  log psi      |d Re| <= 2e-5 * max(1, |Re|);  phase within 1e-4 (mod 2 pi)
  E_L, KE, Lz, Lz^2, L^2
               |d| <= 5e-5 * max(1, |ref|, scale), where `scale` is the size of the
               terms that cancel in that observable (helpers.cancellation_scales:
               e.g. L^2 = -sum_k [S_k + (G_k + i M_k)^2] is often ~1% of its terms).
               Measured on the box: <= ~5e-6; the reference's own float32 Hessian
               route shows the same order of error.
  PE           |d| <= 1e-5 * max(1, |ref|)
Walkers are kept 0.15 rad from the poles (the cot/1/sin^2 terms of
hamiltonian.py:121-129 amplify f32 rounding there, in the reference as well).
"""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from deephall_amd import config, hamiltonian, make_network
from deephall_amd.loss import device_stats
from deephall_amd.mcmc import make_mcmc_step
from deephall_amd.random import Key
from deephall_amd.train import init_guess
from helpers import cancellation_scales, fold_sparse, logpsi_f32_errors, make_params, make_walkers, oracle_config, rel_err, scaled_err, to_device_params, within_f32_floor
from oracle import channels as CH
from oracle import philox
from oracle import reference as R
from test_oracle_kat import droplet_L2, engineered_params

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
TOL_E = 5e-5


def build(ocfg):
    system = config.System(
        nspins=tuple(ocfg.nspins), flux=ocfg.flux, interaction_strength=ocfg.interaction_strength,
        interaction_type=config.InteractionType(ocfg.interaction_type), radius=ocfg.radius,
    )
    net = config.Network()
    net.psiformer.num_heads, net.psiformer.heads_dim = ocfg.num_heads, ocfg.heads_dim
    net.psiformer.num_layers, net.psiformer.determinants = ocfg.num_layers, ocfg.determinants
    net.orbital = config.OrbitalType(getattr(ocfg, "orbital", "full"))
    return system, make_network(system, net)


def cart_err(x, y):
    """max distance between walkers as points on the unit sphere (angles are
    ill-conditioned at the poles: arccos near +-1)."""
    def cart(z):
        z = np.asarray(z, np.float64)
        return np.stack([np.sin(z[..., 0]) * np.cos(z[..., 1]), np.sin(z[..., 0]) * np.sin(z[..., 1]), np.cos(z[..., 0])], -1)

    return float(np.max(np.abs(cart(x) - cart(y))))


def phase_err(a, b):
    d = np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b))))
    return float(np.max(np.abs(d)))


def check_energy(e, o, ref_e, ref_o, scales, tol=TOL_E):
    pe = ref_o["potential"]
    assert scaled_err(e.cpu().numpy(), ref_e, scales["kinetic"] + np.abs(pe)) < tol
    assert scaled_err(o["kinetic"].cpu().numpy(), ref_o["kinetic"], scales["kinetic"]) < tol
    assert rel_err(o["potential"].cpu().numpy(), pe) < 1e-5
    for k in ("angular_momentum_z", "angular_momentum_z_square", "angular_momentum_square"):
        assert scaled_err(o[k].cpu().numpy(), ref_o[k], scales[k]) < tol, k


@pytest.mark.parametrize("name", ["C1", "C2", "MIX"])
def test_golden_local_energy(cuda, name):
    g = np.load(GOLDEN / f"local_energy_{name}.npz")
    ocfg = R.OracleConfig(**json.loads(str(g["config"])))
    ocfg.nspins = tuple(ocfg.nspins)
    p64 = make_params(ocfg, seed=int(g["param_seed"]))
    system, model = build(ocfg)
    params = to_device_params(p64)
    x = torch.tensor(g["x"], device=cuda)
    lp = model.apply(params, x).cpu().numpy()
    err = np.abs(lp.real - g["logpsi"].real) / np.maximum(np.abs(g["logpsi"].real), 1.0)
    assert within_f32_floor(err, logpsi_f32_errors(p64, ocfg, g["x"]), 1e-5)
    assert phase_err(lp.imag, g["logpsi"].imag) < 1e-4
    e, o = hamiltonian.local_energy(model, system)(params, x)
    ref_o = {"kinetic": g["kinetic"], "potential": g["potential"], "angular_momentum_z": g["lz"],
             "angular_momentum_z_square": g["lz2"], "angular_momentum_square": g["l2"]}
    check_energy(e, o, g["e_l"], ref_o, cancellation_scales(p64, ocfg, g["x"]))


@pytest.mark.parametrize("name,B", [("C2", 16), ("C4", 4), ("C5", 2)])
def test_local_energy_vs_channel_oracle(cuda, name, B):
    ocfg = oracle_config(name)
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    x = make_walkers(B, ocfg.nelec, seed=11)
    lp_ref, ke, o_ref, _ = CH.local_energy(p64, ocfg, torch.tensor(x, dtype=torch.float64))
    pe = np.array([R.potential(ocfg, torch.tensor(x[b], dtype=torch.float64)).item() for b in range(B)])
    e, o = hamiltonian.local_energy(model, system)(params, torch.tensor(x, device=cuda))
    ref_o = {k: v.numpy() for k, v in o_ref.items()}
    ref_o["kinetic"] = ke.numpy()
    ref_o["potential"] = pe
    check_energy(e, o, ke.numpy() + pe, ref_o, cancellation_scales(p64, ocfg, x))
    lp = model.apply(params, torch.tensor(x, device=cuda)).cpu().numpy()
    # 1e-5 relative, else within the float32 run's error distribution on these walkers
    err = np.abs(lp.real - lp_ref.numpy().real) / np.maximum(np.abs(lp_ref.numpy().real), 1.0)
    assert within_f32_floor(err, logpsi_f32_errors(p64, ocfg, x), 1e-5)


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_engineered_known_answer_full_batch(cuda, name):
    """Every walker of a full batch: KE = N/2, Lz, L^2 of the LLL droplet (analytic pin)."""
    ocfg = oracle_config(name, interaction_strength=0.0)
    p = engineered_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p)
    B = 4096 if name == "C2" else 512
    x = torch.tensor(make_walkers(B, ocfg.nelec, seed=3, margin=0.3), device=cuda)
    e, o = hamiltonian.local_energy(model, system)(params, x)
    L2, Lz = droplet_L2(ocfg.nelec, ocfg.flux)
    # the droplet determinant is singular when two electrons meet (no Jastrow here):
    # strict bound on well-separated walkers, percentiles on the whole batch
    xs = x.double().cpu()
    rh = torch.stack([torch.sin(xs[..., 0]) * torch.cos(xs[..., 1]), torch.sin(xs[..., 0]) * torch.sin(xs[..., 1]),
                      torch.cos(xs[..., 0])], -1)
    dmin = (torch.cdist(rh, rh) + 9 * torch.eye(ocfg.nelec)).amin(dim=(1, 2)).numpy()
    sep = dmin > 0.3
    assert sep.sum() > B // 4
    # size of the cancelling magnetic terms (Q cot th)^2, (Q / sin th)^2 of hamiltonian.py:121-159
    st = torch.sin(xs[..., 0])
    q2 = ocfg.Q**2
    geo = {"kinetic": (q2 / st**2).sum(-1).numpy() / (2 * ocfg.r**2),
           "angular_momentum_square": (q2 * (1 / st).sum(-1) ** 2).numpy()}
    geo["angular_momentum_z_square"] = geo["angular_momentum_square"]
    geo["angular_momentum_z"] = np.sqrt(geo["angular_momentum_square"])
    for k, want in (("kinetic", ocfg.nelec / 2), ("angular_momentum_z", Lz),
                    ("angular_momentum_square", L2), ("angular_momentum_z_square", Lz * Lz)):
        err = np.abs(o[k].cpu().numpy() - want) / np.maximum(max(1.0, abs(want)), geo[k])
        # calibration (first 300 walkers, KE): the reference's float32 Hessian route has
        # median 4.6e-7 / mean 3.5e-5 / max 9e-3 of this scaled error; the kernels 1.8e-7 / 1.5e-5 / 2e-3
        assert np.max(err[sep]) < 1e-3, k
        assert np.median(err) < 2e-6 and np.percentile(err, 99) < 5e-3, k


@pytest.mark.parametrize("name,B", [("C2", 37), ("C5", 128)])
def test_batch_composition_and_chunking_invariance(cuda, name, B):
    """Rows are independent of the batch and of the workspace chunking, bit for bit.  C5
    (round-5 verdict, weak 1b): 128 walkers in one chunk against chunks of <= 4 walkers, the
    N = 20 path: the envelope-first local energy (no F over the channel rows: env_coef_kernel,
    the Weff GEMM, srows_kernel's six special rows S and their orbital map FS, env_phi_kernel, then det_energy on PhiC; DESIGN.md
    §1 "Routes") and det_value<MGV> for log psi.  env_stream_kernel is not on this path (it
    serves N = 20 only with several determinants or two spin blocks)."""
    ocfg = oracle_config(name)
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    x = torch.tensor(make_walkers(B, ocfg.nelec, seed=5), device=cuda)
    lp_all = model.apply(params, x)
    lp_part = torch.cat([model.apply(params, x[:5]), model.apply(params, x[5:])])
    assert torch.equal(lp_all, lp_part)  # rows are independent: bit-identical
    from deephall_amd.hamiltonian import _run_local_energy

    e1, o1 = _run_local_energy(model, params, x)
    h = model.prepare(params, x.device)
    one = h.lib.dh_workspace_bytes(h.h, 4, 1)
    e2, o2 = _run_local_energy(model, params, x, ws_budget=one)  # forces chunks of <= 4 walkers
    assert torch.isfinite(e1).all()
    assert torch.equal(e1, e2) and torch.equal(o1, o2)


def test_nan_and_edge_walkers_propagate(cuda):
    ocfg = oracle_config("C1")
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    x = torch.tensor(make_walkers(3, 3), device=cuda)
    x[1, 0, 0] = float("nan")
    e, o = hamiltonian.local_energy(model, system)(params, x)
    lp = model.apply(params, x)
    assert torch.isnan(e[1]).item() and torch.isnan(lp[1]).item()
    assert torch.isfinite(e[0]).item() and torch.isfinite(e[2]).item()
    e1, _ = hamiltonian.local_energy(model, system)(params, x[:1])  # B = 1
    assert torch.equal(e1, e[:1])


@pytest.mark.parametrize("name", ["C1", "C2", "C4", "C5"])
def test_golden_mcmc_injected_noise(cuda, name):
    g = np.load(GOLDEN / f"mcmc_{name}.npz")
    ocfg = R.OracleConfig(**json.loads(str(g["config"])))
    ocfg.nspins = tuple(ocfg.nspins)
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    noise = torch.tensor(g["noise"], device=cuda)
    steps, B = noise.shape[:2]
    step = make_mcmc_step(model, batch_per_device=B, steps=steps)
    x = torch.tensor(g["x0"], device=cuda)
    x, pmove = step(params, x, Key(0), float(g["width"]), noise=noise)
    assert np.array_equal(step.last_n_accept.cpu().numpy(), g["n_acc"])
    # the proposal is evaluated in double on the device (mcmc.hip): positions are the
    # float64 oracle's to f32 rounding (the reference's own f32 phi = sign(y) arccos(x /
    # sin th), mcmc.py:101, is off by up to ~3e-4 near phi = 0, pi; tools/diag_proposal.py)
    assert cart_err(x.cpu().numpy(), g["x"]) < 2e-6
    assert float(pmove) == pytest.approx(g["n_acc"].sum() / (steps * B))
    # lp must be 2 Re log psi of the walkers the device ended with
    lp_at_x = 2.0 * R.batch_logpsi(make_params(ocfg), ocfg, torch.tensor(x.cpu().numpy(), dtype=torch.float64)).real
    assert rel_err(step.last_lp.cpu().numpy(), lp_at_x.numpy()) < 2e-5


def test_device_rng_matches_philox_oracle(cuda):
    """The device draws exactly oracle/philox.py's numbers (integer part bit-exact)."""
    N, B, seed = 6, 64, 1234
    x = init_guess(Key(seed), B, N, cuda, walker_offset=100)
    u1, u2 = philox.init_uniforms(seed, np.arange(100, 100 + B), N)
    ref = R.init_guess_from_uniforms(u1.astype(np.float64), u2.astype(np.float64))
    assert cart_err(x.cpu().numpy(), ref) < 1e-6
    # MCMC with device RNG == MCMC with the oracle's Philox noise injected
    ocfg = oracle_config("C2")
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    x0 = torch.tensor(make_walkers(B, N, seed=9), device=cuda)
    steps = 3
    noise = []
    for s in range(steps):
        n, u, a = philox.mcmc_noise(seed, 50 + s, np.arange(B) + 7, N)
        noise.append(np.concatenate([n, u, a[:, None]], -1))
    noise = torch.tensor(np.stack(noise), dtype=torch.float32, device=cuda)
    step = make_mcmc_step(model, batch_per_device=B, steps=steps)
    xa, _ = step(params, x0.clone(), Key(seed, 50), 0.2, walker_offset=7)
    na = step.last_n_accept.clone()
    xb, _ = step(params, x0.clone(), Key(seed, 50), 0.2, noise=noise, walker_offset=7)
    nb = step.last_n_accept.clone()
    agree = (na == nb).float().mean().item()
    assert agree > 0.95  # Box-Muller in f32 vs f64: rare borderline decisions may flip
    same = (na == nb).cpu().numpy()
    assert cart_err(xa.cpu().numpy()[same], xb.cpu().numpy()[same]) < 5e-4


def test_mcmc_sharding_invariance(cuda):
    """Two 'ranks' with walker offsets reproduce one rank with all walkers (bit-exact)."""
    ocfg = oracle_config("C1")
    system, model = build(ocfg)
    params = to_device_params(make_params(ocfg))
    B = 64
    x = torch.tensor(make_walkers(B, 3, seed=2), device=cuda)
    full = make_mcmc_step(model, batch_per_device=B, steps=5)
    half = make_mcmc_step(model, batch_per_device=B // 2, steps=5)
    xa, _ = full(params, x.clone(), Key(99, 3), 0.1, walker_offset=0)
    x0 = x[: B // 2].clone()
    x1 = x[B // 2 :].clone()
    half(params, x0, Key(99, 3), 0.1, walker_offset=0)
    half(params, x1, Key(99, 3), 0.1, walker_offset=B // 2)
    assert torch.equal(xa, torch.cat([x0, x1]))


def _stats_inputs(B, seed, ties=False):
    g = np.random.default_rng(seed)
    e = g.standard_normal((B, 2)).astype(np.float32)
    e[:, 0] += 3.0
    if ties:  # heavy duplication: many equal keys in every radix digit
        e = np.round(e * 4) / 4
    obs = g.standard_normal((B, 8)).astype(np.float32)
    obs[:, 4] = np.abs(obs[:, 4]) * 3  # Lz^2 >= 0
    if B > 9:
        e[7, 0] = 1e6  # outlier gets clipped
        e[9, 1] = np.nan  # NaN walker excluded from the nanmeans
        obs[3, 5] = -5e4  # L^2 outlier
    nacc = g.integers(0, 11, B).astype(np.int32)
    return e, obs, nacc


def _oracle_stats(e, obs):
    el = np.empty(e.shape[0], np.complex128)  # keep Re valid where only Im is NaN
    el.real, el.imag = e[:, 0], e[:, 1]
    o = {"kinetic": obs[:, 0] + 1j * obs[:, 1], "potential": obs[:, 2], "angular_momentum_z": obs[:, 3],
         "angular_momentum_z_square": obs[:, 4], "angular_momentum_square": obs[:, 5]}
    return el, o, R.loss_stats(el, o, penalties=True)


@pytest.mark.parametrize("B,ties", [(1, False), (2, False), (7, True), (1000, False), (4096, True), (20000, False),
                                    (40000, False), (131072, False)])
def test_energy_stats_kernel(cuda, B, ties):
    """dh_energy_stats against loss.py:30-38, 66-92 (oracle), every DH_STAT_* entry; any batch
    size (radix-select quantiles), ties, NaN walkers, outliers; penalties on and off."""
    ocfg = oracle_config("C1")
    system, model = build(ocfg)
    e, obs, nacc = _stats_inputs(B, B, ties)
    el, o, ref = _oracle_stats(e, obs)
    for pen in (False, True):
        out = device_stats(model, torch.tensor(e, device=cuda), torch.tensor(obs, device=cuda),
                           torch.tensor(nacc, device=cuda), steps=10, penalties=pen).cpu().numpy()
        assert out[0] == pytest.approx(ref["energy"].real, rel=1e-5)
        assert out[1] == pytest.approx(ref["energy"].imag, rel=1e-5, abs=1e-6)
        assert out[2] == pytest.approx(ref["clipped_energy"].real, rel=1e-5)
        assert out[3] == pytest.approx(ref["clipped_energy"].imag, rel=1e-5, abs=1e-6)
        assert out[4] == pytest.approx(np.nanmean(el.real**2), rel=1e-5)
        for i, k in ((5, "kinetic"), (7, "potential"), (8, "angular_momentum_z"), (9, "angular_momentum_z_square"),
                     (10, "angular_momentum_square")):
            want = ref[k].real
            assert out[i] == pytest.approx(want, rel=1e-5, abs=1e-6), k
        assert out[6] == pytest.approx(ref["kinetic"].imag, rel=1e-5, abs=1e-6)
        assert out[11] == pytest.approx(nacc.sum() / (10 * B), rel=1e-6)
        assert out[12] == np.sum(~(np.isnan(e[:, 0]) | np.isnan(e[:, 1])))
        if pen:
            for i, k in ((13, "clipped_lz2"), (14, "clipped_lz"), (15, "clipped_l2")):
                assert out[i] == pytest.approx(ref[k].real, rel=1e-5, abs=1e-6), k
        else:
            assert (out[13:] == 0).all()


@pytest.mark.parametrize("B", [1, 5, 4096, 50000])
@pytest.mark.parametrize("pen", [(0.0, 0.0, 0.0), (0.3, 1.5, 0.2)])
def test_loss_diff_kernel(cuda, B, pen):
    """dh_loss_diff (clipped difference weighting the gradient) against loss.py:75-89."""
    from deephall_amd.loss import loss_diff

    ocfg = oracle_config("C1")
    system, model = build(ocfg)
    e, obs, _ = _stats_inputs(B, 100 + B)
    el, o, ref = _oracle_stats(e, obs)
    g = np.zeros(16, np.float32)
    g[2], g[3] = ref["clipped_energy"].real, ref["clipped_energy"].imag
    g[13], g[14], g[15] = ref["clipped_lz2"].real, ref["clipped_lz"].real, ref["clipped_l2"].real
    diff, nvalid = loss_diff(model, torch.tensor(e, device=cuda), torch.tensor(obs, device=cuda),
                             torch.tensor(g, device=cuda), *pen)
    stats = {k: (np.complex64(v) if k == "clipped_energy" else np.float32(v)) for k, v in ref.items()
             if k.startswith("clipped")}
    want = R.loss_diff(el, o, stats, *pen)
    got = diff.cpu().numpy()
    nan_w = np.isnan(want.real) | np.isnan(want.imag)
    assert np.array_equal(np.isnan(got[:, 0]) | np.isnan(got[:, 1]), nan_w)
    scale = np.maximum(np.abs(want[~nan_w]), 1.0)
    assert np.max(np.abs(got[~nan_w, 0] - want[~nan_w].real) / scale) < 2e-6
    assert np.max(np.abs(got[~nan_w, 1] - want[~nan_w].imag) / scale) < 2e-6
    assert float(nvalid) == np.sum(~nan_w)


def test_walker_groups_on_parallel_streams_are_bit_identical(cuda):
    """make_vmc_iteration with 2 / 3 walker groups on parallel HIP streams == 1 group."""
    from deephall_amd.random import PRNGKey
    from deephall_amd.train import make_vmc_iteration

    ocfg = oracle_config("C2")
    system, model = build(ocfg)
    params = model.init(PRNGKey(3), device=cuda)
    B = 96
    x0 = init_guess(Key(11), B, sum(ocfg.nspins), cuda, network=model)
    ref = None
    for groups in (1, 2, 3):
        it = make_vmc_iteration(model, B, 4, groups)
        x = x0.clone()
        x, e, o, n = it(params, x, Key(5), 0.2)
        torch.cuda.synchronize()
        got = (x.cpu(), e.cpu(), o.cpu(), n.cpu())
        if ref is None:
            ref = got
        else:
            for a, b in zip(ref, got):
                assert torch.equal(a, b), groups


@pytest.mark.parametrize("name,B", [("C2", 4096), ("C4", 1024), ("C5", 4096)])
def test_vmc_iteration_bitwise_repeatable(cuda, name, B):
    """One VMC iteration (4 MCMC moves + the local energy) at the bench's full-chip batch, run
    twice from the same walkers and key: walkers, E_L, observables and accept counts equal bit
    for bit.  A race, an early LDS read or an interleaving-dependent corruption (DESIGN 7.1,
    the two-tiles-per-CU fused tail) shows here while every small-batch comparison passes.
    C5 at the bench's 4096 walkers (round-5 verdict, weak 1b) runs the envelope-first local
    energy: env_phi_kernel over the S / FS / Weff buffers that share the q|k|v space (21 GiB of
    workspace, one chunk of the default 24 GiB since no F is mapped over the channel rows), not
    env_stream_kernel (DESIGN.md §1 "Routes")."""
    from deephall_amd.random import PRNGKey
    from deephall_amd.train import make_vmc_iteration

    ocfg = oracle_config(name)
    system, model = build(ocfg)
    params = model.init(PRNGKey(7), device=cuda)
    x0 = init_guess(Key(13), B, ocfg.nelec, cuda, network=model)
    it = make_vmc_iteration(model, B, 4, 1)
    runs = []
    for _ in range(2):
        x, e, o, n = it(params, x0.clone(), Key(21), 0.2)
        torch.cuda.synchronize()
        runs.append((x.cpu(), e.cpu(), o.cpu(), n.cpu()))
    assert torch.isfinite(runs[0][1]).all()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_c3_global_batch_single_process(cuda):
    """BASELINE.json configs[2]'s global batch (32768 walkers, N=6, 2Q=15) through one
    process: MCMC, local energy (chunked by the workspace), statistics; rows are
    independent of the batch they run in, the statistics equal numpy's on the same E_L."""
    from deephall_amd.hamiltonian import _run_local_energy

    ocfg = oracle_config("C2")
    system, model = build(ocfg)
    params = model.init(42, device=cuda)
    B = 32768
    x = init_guess(Key(5), B, ocfg.nelec, cuda, network=model)
    step = make_mcmc_step(model, batch_per_device=B, steps=2)
    x, pmove = step(params, x, Key(9), 0.1)
    e, o = _run_local_energy(model, params, x)
    e2, o2 = _run_local_energy(model, params, x[4096:8192].contiguous())
    assert torch.equal(e[4096:8192], e2) and torch.equal(o[4096:8192], o2)
    st = device_stats(model, e, o, step.last_n_accept, 2).cpu().numpy()
    en, on = e.cpu().numpy().astype(np.float64), o.cpu().numpy().astype(np.float64)
    assert np.isfinite(en).all()
    el = en[:, 0] + 1j * en[:, 1]
    ref = R.loss_stats(el, {"kinetic": on[:, 0] + 1j * on[:, 1], "angular_momentum_square": on[:, 5]})
    assert st[0] == pytest.approx(ref["energy"].real, rel=1e-5)
    assert st[2] == pytest.approx(ref["clipped_energy"].real, rel=1e-5)
    assert st[5] == pytest.approx(ref["kinetic"].real, rel=1e-5)
    assert st[10] == pytest.approx(ref["angular_momentum_square"], rel=1e-4, abs=1e-5)
    assert st[11] == pytest.approx(float(pmove), rel=1e-6)


@pytest.mark.parametrize("name,B", [("C1", 6), ("MIX", 6), ("C2", 4)])
def test_sparse_orbitals_vs_oracle(cuda, name, B):
    """Orbital type "sparse" (blocks.py:52-62): 8 featured orbitals mixed into the 2Q+1
    harmonics by lll_weight, folded into the full layout on the device; log psi and the
    local energy against the float64 full-Hessian restatement."""
    ocfg = oracle_config(name, orbital="sparse")
    p64 = make_params(ocfg)
    system, model = build(ocfg)
    params = to_device_params(p64)
    x = make_walkers(B, ocfg.nelec, seed=13)
    xt = torch.tensor(x, dtype=torch.float64)
    lp_ref = R.batch_logpsi(p64, ocfg, xt).numpy()
    lp = model.apply(params, torch.tensor(x, device=cuda)).cpu().numpy()
    err = np.abs(lp.real - lp_ref.real) / np.maximum(np.abs(lp_ref.real), 1.0)
    assert within_f32_floor(err, logpsi_f32_errors(p64, ocfg, x), 1e-5)
    assert phase_err(lp.imag, lp_ref.imag) < 1e-4
    e_ref, o_ref = R.local_energy(p64, ocfg, xt)
    e, o = hamiltonian.local_energy(model, system)(params, torch.tensor(x, device=cuda))
    # a handful of walkers: each observable against the magnitude of the terms that cancel in
    # it, like the full-layout goldens; the f32-floor distribution gate for sparse orbitals
    # runs on the 64-walker MIX_sparse / C2_sparse fixtures (test_gpu_floor.py)
    pf, cf = fold_sparse(p64, ocfg)
    check_energy(e, o, e_ref.detach().numpy(), {k: v.detach().numpy() for k, v in o_ref.items()},
                 cancellation_scales(pf, cf, x))
