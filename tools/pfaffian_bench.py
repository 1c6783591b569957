"""Moore-Read Pfaffian state: the native kernels (pfaffian.hip) against the callable route
(`MooreReadCallable` through deephall_amd.generic: torch.func derivatives of the torch skew
elimination), and against cf.hip (the Jain state with both levels filled) at equal N.
ms per dh_local_energy batch and per dh_logpsi batch at B = 4096; the callable route runs at
a batch it can afford and is scaled per walker.  Prints one line per N, then both kernels' LDS
per walker (what bounds the walkers that share a CU)."""
import sys
import time

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from deephall_amd import config, hamiltonian, make_network  # noqa: E402
from deephall_amd.networks import MooreReadCallable  # noqa: E402
from helpers import make_walkers  # noqa: E402

B = 4096


def timed(fn, reps=None, window=0.5):
    """Seconds per call after a warm-up; reps None: as many as fill `window` seconds."""
    fn()
    torch.cuda.synchronize()
    if reps is None:
        t = time.perf_counter()
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        reps = max(10, int(window / ((time.perf_counter() - t) / 5)))
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def native(kind, N, flux):
    system = config.System(nspins=(N, 0), flux=flux)
    net = config.Network()
    net.type = config.NetworkType(kind)
    model = make_network(system, net)
    x = torch.tensor(make_walkers(B, N, seed=5, margin=0.05), device="cuda")
    p = model.init(0, device="cuda")
    el = hamiltonian.local_energy(model, system)
    return system, x, timed(lambda: el(p, x)), timed(lambda: model.apply(p, x))


for N, Bc in ((6, 4096), (12, 512), (16, 256)):
    flux = 2 * (N - 1) - 1
    system, x, t_el, t_lp = native("pfaffian", N, flux)
    ref = MooreReadCallable((N, 0), flux, system=system)
    xc = x[:Bc].contiguous()
    elc = hamiltonian.local_energy(ref, system)
    c_el = timed(lambda: elc({}, xc), 2) * B / Bc
    c_lp = timed(lambda: ref(None, xc), 5) * B / Bc
    print(f"pfaffian N={N:2d} 2Q={flux} B={B}: local energy native {t_el * 1e3:8.3f} ms ({B / t_el:,.0f} E_L/s), "
          f"callable {c_el * 1e3:9.1f} ms (measured at B={Bc}), ratio {c_el / t_el:6.1f}x;  "
          f"log psi native {t_lp * 1e3:7.3f} ms, callable {c_lp * 1e3:8.2f} ms, ratio {c_lp / t_lp:6.1f}x", flush=True)
for N in (6, 12):  # cf.hip at equal N: both Lambda levels filled, N = 4 Q1 + 4
    flux = (5 * N - 8) // 2
    _, _, t_el, t_lp = native("jain", N, flux)
    print(f"jain     N={N:2d} 2Q={flux} B={B}: local energy native {t_el * 1e3:8.3f} ms, log psi native {t_lp * 1e3:7.3f} ms",
          flush=True)
for N in (6, 12, 16, 28):
    lds_e, lds_v = 16 * (11 * N * N + 17 * N + 4), 16 * (N * N + 4 * N + 4)
    print(f"pfaffian N={N:2d}: energy kernel {lds_e} B of LDS per walker ({160 * 1024 // lds_e} workgroups per CU by LDS), "
          f"value kernel {lds_v} B ({160 * 1024 // lds_v} by LDS)")
