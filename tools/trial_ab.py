"""A/B of the parameter-free trial states between two builds of the library (same C ABI).

    DH_LIB_PATH=ab/parent.so python tools/trial_ab.py dump OUT.npz [--host]
    python tools/trial_ab.py diff A.npz B.npz
    DH_LIB_PATH=ab/parent.so python tools/trial_ab.py time

dump: every case below on B = 257 fixed-seed walkers: dh_logpsi, dh_local_energy (e_l, obs) and the
walkers, log-probabilities and accept counts after 3 moves of dh_mcmc_step.  --host (no GPU): the
(rc, dh_last_error()) of every dh_create* call the host tests' refusal tables make.  diff: one line
per case and array, bit for bit.  time: median us per call at B = 4096.  One process, one library.
"""
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
G1, G2, G3, G4, G5 = (0.7, 0.3), (1.9, -2.1), (2.6, 1.2), (1.1, 2.8), (1.5, -0.6)
HARM = dict(interaction_type="harmonic")
AB = dict(base="pfaffian", holes=(G1, G2), pairing=((0,), (1,)))  # one hole in each group
# name -> (class, nspins, flux, state keywords, system keywords, clustered walkers)
CASES = {
    "pfaffian_2_3_p2": ("MooreRead", (2, 0), 3, dict(cf_flux=2)),
    "pfaffian_4_5": ("MooreRead", (4, 0), 5, {}),
    "pfaffian_6_9": ("MooreRead", (6, 0), 9, {}),
    "pfaffian_4_11_p2": ("MooreRead", (4, 0), 11, dict(cf_flux=2)),
    "pfaffian_12_21": ("MooreRead", (12, 0), 21, {}),
    "pfaffian_clustered_6": ("MooreRead", (6, 0), 9, {}, {}, True),
    "pfaffian_clustered_8": ("MooreRead", (8, 0), 13, {}, {}, True),
    "halperin_22_110": ("Halperin", (2, 2), 1, dict(exponents=(1, 1, 0))),
    "halperin_22_332": ("Halperin", (2, 2), 7, {}),
    "halperin_33_332": ("Halperin", (3, 3), 12, {}),
    "halperin_33_332_harmonic": ("Halperin", (3, 3), 12, {}, HARM),
    "halperin_30_330": ("Halperin", (3, 0), 6, dict(exponents=(3, 3, 0))),
    "halperin_55_332": ("Halperin", (5, 5), 22, {}),
    "halperin_1010_111": ("Halperin", (10, 10), 19, dict(exponents=(1, 1, 1))),
    "qh_halperin_22_both": ("Quasihole", (2, 2), 8, dict(holes=(G1,))),
    "qh_halperin_23_up": ("Quasihole", (2, 3), 10, dict(holes=(G1,), species=("up",))),
    "qh_halperin_30_pole": ("Quasihole", (3, 0), 8, dict(exponents=(3, 3, 0), holes=((0.0, 0.0), G2))),
    "qh_pfaffian_4_abelian": ("Quasihole", (4, 0), 6, dict(base="pfaffian", holes=(G1,))),
    "qh_pfaffian_4_ab": ("Quasihole", (4, 0), 6, AB),
    "qh_pfaffian_6_aabb_abelian": ("Quasihole", (6, 0), 12, dict(AB, holes=(G1, G2, G3, G4, G5), pairing=((0, 1), (2, 3)))),
    "qh_pfaffian_12_ab": ("Quasihole", (12, 0), 22, AB),
    "qh_pfaffian_clustered_6": ("Quasihole", (6, 0), 10, AB, {}, True),
    "laughlin_3_6": ("Laughlin", (3, 0), 6, {}),
    "laughlin_qp_4_8_lz1": ("Laughlin", (4, 0), 8, dict(excitation_lz=1.0)),
    "jain_4_6": ("Jain", (4, 0), 6, {}),
    # the timing cases that are not dump cases
    "qh_halperin_33_both": ("Quasihole", (3, 3), 13, dict(holes=(G1,))),
    "qh_pfaffian_6_ab": ("Quasihole", (6, 0), 10, AB),
}
DUMP = [c for c in CASES if c not in ("qh_halperin_33_both", "qh_pfaffian_6_ab")]
TIMED = ["pfaffian_6_9", "halperin_33_332", "qh_halperin_33_both", "qh_pfaffian_6_ab"]


def build(name, B, cuda):
    """(model, params, walkers [B, N, 2] on the GPU) of a case."""
    import torch
    from deephall_amd import config, networks
    from helpers import make_walkers

    cls, nspins, flux, kw, sysk, clustered = (CASES[name] + ({}, False))[:6]
    system = config.System(nspins=nspins, flux=flux, interaction_type=config.InteractionType(sysk.get("interaction_type", "coulomb")))
    model = getattr(networks, cls)(nspins, flux, system=system, **kw)
    N = sum(nspins)
    x = make_walkers(B, N, seed=13, margin=0.05)
    if clustered:  # a pair 1e-3 rad apart, in and out of the pivot order (test_clustered_walkers)
        for w in range(B):
            i, k = ((0, 1), (2, 3), (N - 2, N - 1))[w % 3]
            x[w, k] = x[w, i] + np.float32([6e-4, 8e-4])
    return model, system, model.init(0, device=cuda), torch.tensor(x, device=cuda)


def dump_gpu(out):
    import torch
    from deephall_amd import hamiltonian
    from deephall_amd.mcmc import make_mcmc_step
    from deephall_amd.random import PRNGKey

    cuda, res = torch.device("cuda"), {}
    for name in DUMP:
        model, system, params, x = build(name, 257, cuda)
        e_l, obs = hamiltonian.local_energy(model, system).raw(params, x)
        step = make_mcmc_step(model, batch_per_device=257, steps=3)
        xm, _ = step(params, x.clone(), PRNGKey(2), 0.3)
        arrays = dict(logpsi=torch.view_as_real(model.apply(params, x)), e_l=e_l, obs=obs, mcmc_x=xm,
                      mcmc_lp=step.last_lp, mcmc_nacc=step.last_n_accept)
        for k, v in arrays.items():
            res[f"{name}/{k}"] = v.cpu().numpy()
    np.savez(out, **res)
    print(f"{len(DUMP)} cases, {len(res)} arrays -> {out}")


def dump_host(out):
    """Run the host tests' test_native_validation with their _create recorded."""
    import importlib
    from deephall_amd import _lib

    res, lib, h = {}, _lib.load(), C.c_void_p()

    def keep(key, rc, msg):
        res[key] = np.frombuffer(f"{rc} {msg.decode() if rc else ''}".encode(), dtype=np.uint8)  # rc 0: a stale message

    for state in ("jain", "pfaffian", "halperin", "quasihole"):
        mod = importlib.import_module(f"test_{state}_host")
        inner, n = mod._create, [0]

        def record(*a, _inner=inner, _n=n, _state=state, **kw):
            rc, msg = _inner(*a, **kw)
            keep(f"{_state}/{_n[0]:03d} {a} {kw}", rc, msg)
            _n[0] += 1
            return rc, msg

        mod._create = record
        mod.test_native_validation()
    for fn, a in (("dh_create", ()), ("dh_create_cf", (None, 0)), ("dh_create_halperin", (3, 3, 2)), ("dh_create_quasihole", (None,))):
        keep(f"null/{fn}", getattr(lib, fn)(None, *a, C.byref(h)), lib.dh_last_error())
    np.savez(out, **res)
    print(f"{len(res)} dh_create* calls -> {out}")


def diff(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(Bz.files))
    for k in sorted(set(A.files) & set(Bz.files)):
        x, y = A[k], Bz[k]
        if x.shape != y.shape:
            n = -1
        else:
            v = np.uint8 if x.dtype.itemsize < 4 else np.uint32
            n = 0 if np.array_equal(x.view(v), y.view(v)) else int(np.count_nonzero(x.view(v) != y.view(v)))
        print(f"{k:60s} {'equal' if n == 0 else f'{n} differ' if n > 0 else 'shapes differ'}")
        if n:
            bad.append(k)
    print("ALL EQUAL" if not bad else f"DIFFERENT: {len(bad)} of {len(A.files)}")
    return 1 if bad else 0


def timing():
    """Device events around windows of calls after a warm-up of 250; 5 windows of > 1 s each."""
    import torch
    from deephall_amd.networks.psiformer import _ptr, _stream

    cuda, B, shortest = torch.device("cuda"), 4096, math.inf
    for name in TIMED:
        model, _, params, x = build(name, B, cuda)
        h = model.prepare(params, cuda)
        out, e_l, obs = (torch.empty(B, k, dtype=torch.float32, device=cuda) for k in (2, 2, 8))
        ws = h.workspace(max(h.lib.dh_workspace_bytes(h.h, B, 0), h.lib.dh_workspace_bytes(h.h, B, 1)))
        s = _stream(cuda)
        calls = {"logpsi": lambda: h.lib.dh_logpsi(h.h, _ptr(x), B, _ptr(out), _ptr(ws), ws.numel(), s),
                 "local_energy": lambda: h.lib.dh_local_energy(h.h, _ptr(x), B, _ptr(e_l), _ptr(obs), _ptr(ws), ws.numel(), s)}
        for what, call in calls.items():
            def window(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(n):
                    rc = call()
                b.record()
                b.synchronize()
                assert rc == 0, h.lib.dh_last_error()
                return a.elapsed_time(b) * 1e-3  # s
            window(250)
            n = int(1.3 * 1000 / window(1000)) + 1  # calls of a 1.3 s window (the 1000 calls run a little slow)
            t = [window(n) for _ in range(5)]
            shortest = min(shortest, *t)
            print(f"{name}/{what:14s} {np.median(t) / n * 1e6:9.3f} us  ({n} calls per window)", flush=True)
    print(f"shortest timed window: {shortest:.2f} s")


if __name__ == "__main__":
    mode, args = sys.argv[1], [a for a in sys.argv[2:] if a != "--host"]
    t0 = time.time()
    if mode == "dump":
        (dump_host if "--host" in sys.argv else dump_gpu)(args[0])
    elif mode == "diff":
        sys.exit(diff(*args))
    elif mode == "time":
        timing()
    else:
        sys.exit(__doc__)
    print(f"{mode}: {time.time() - t0:.1f} s, library {os.environ.get('DH_LIB_PATH', 'in tree')}")
