"""Time dh_ntk, the per-walker gradient Gram matrix of MinSR, on the GPU box (a report, not a gate).

Default: C2 (N = 6, 2Q = 15, D = 256, L = 2) with 2 x 4096 walkers — one MinSR step's call: the
batch doubled, cotangents (1, 0) | (0, 1).  Prints the whole call's time (HIP events around
`reps` calls after a warm-up, five windows: median and spread), the same for dh_logpsi_vjp on
the same walkers (what the forward and reverse passes cost without the Gram products), and the
Gram products' algorithmic rate

    FLOP = 2 * (R^2 / 2) * sum over dense maps (K_in + K_out),  R = walkers * N rows

over the whole call's time and over the call's time less the VJP's, against the 157.3 TF/s f32
matrix peak.  usage: ntk_bench.py [B] [NSPINS FLUX] [reps]"""
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from deephall_amd import config  # noqa: E402
from deephall_amd.networks import make_network  # noqa: E402
from deephall_amd.random import Key, PRNGKey  # noqa: E402
from deephall_amd.train import init_guess  # noqa: E402

PEAK_F32_MATRIX = 157.3e12

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
nspins = (int(sys.argv[2]), 0) if len(sys.argv) > 2 else (6, 0)
flux = int(sys.argv[3]) if len(sys.argv) > 3 else 15
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
if not torch.cuda.is_available():
    sys.exit("ntk_bench.py needs a GPU: no time is reported without one")
model = make_network(config.System(nspins=nspins, flux=flux), config.Network())
spec = model.spec
params = model.init(PRNGKey(42), device="cuda")
x = init_guess(Key(1), B, sum(nspins), "cuda", network=model)
x2 = torch.cat([x, x])
ct = torch.zeros(2 * B, 2, device="cuda")
ct[:B, 0] = 1.0
ct[B:, 1] = 1.0

N, D, L = spec.nelec, spec.num_heads * spec.heads_dim, spec.num_layers
orb_cols = 2 * (spec.flux + 1) * N * spec.ndets * (2 if min(spec.nspins) > 0 else 1)
R = 2 * B * N
ksum = L * ((D + 3 * D) + 3 * (D + D)) + (D + orb_cols) + (4 + D)  # qkv, Wo, Wl, Wm per layer; orbitals; W0
flop = 2.0 * (R * R / 2.0) * ksum


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t = [window(fn) for _ in range(5)]
    return statistics.median(t), min(t), max(t)


ntk = timed(lambda: model.ntk(params, x2, ct))
vjp = timed(lambda: model.vjp(params, x2, ct))
print(f"config nspins {nspins} flux {flux}: {2 * B} walkers, R = {R} rows, tile {model.ntk_tile_walkers(x.device)} walkers, "
      f"sum(K_in + K_out) = {ksum}, Gram FLOP = {flop:.3e}")
print(f"dh_ntk          {ntk[0]:9.2f} ms  (min {ntk[1]:.2f}, max {ntk[2]:.2f}; {reps} calls per window, 5 windows)")
print(f"dh_logpsi_vjp   {vjp[0]:9.2f} ms  (min {vjp[1]:.2f}, max {vjp[2]:.2f})")
whole = flop / (ntk[0] * 1e-3)
print(f"Gram FLOP / whole call: {whole / 1e12:6.1f} TF/s = {whole / PEAK_F32_MATRIX:.3f} of {PEAK_F32_MATRIX / 1e12} TF/s (f32 matrix peak)")
if ntk[0] > vjp[0]:
    net = flop / ((ntk[0] - vjp[0]) * 1e-3)
    print(f"Gram FLOP / (call - VJP): {net / 1e12:6.1f} TF/s = {net / PEAK_F32_MATRIX:.3f} of peak")
