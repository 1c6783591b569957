"""Time dh_ntk, the per-walker gradient Gram matrix of MinSR, on the GPU box (a report, not a gate).

Default: C2 (N = 6, 2Q = 15, D = 256, L = 2) with 2 x 4096 walkers — one MinSR step's call: the
batch doubled, cotangents (1, 0) | (0, 1).  Prints the whole call's time (HIP events around
`reps` calls after a warm-up, five windows: median and spread), the same for dh_logpsi_vjp on
the same walkers (what the forward and reverse passes cost without the Gram products), and the
Gram products' algorithmic rate

    FLOP = 2 * (R^2 / 2) * sum over dense maps (K_in + K_out),  R = walkers * N rows

over the whole call's time and over the call's time less the VJP's, against the 157.3 TF/s f32
matrix peak.

``--parts R`` (repeatable) also times what sharded MinSR adds: dh_ntk_part(0 of 1) + dh_ntk_mirror
(the same work as dh_ntk), dh_ntk_part(p of R) for every p on this one GPU — the slowest against
1 / R of the whole — and dh_minsr_matrix against the float64 torch assembly of
optimizers.minsr_direction and against its traffic of 16 M^2 bytes (T read twice, A written once).
``--jvp`` also times SPRING's call: dh_ntk_jvp with T against dh_ntk_part(0 of 1), dh_ntk_jvp
without T against dh_logpsi_vjp, and the JVP's 2 R P FLOP over the differences.
usage: ntk_bench.py [B] [NSPINS FLUX] [reps] [--parts R]... [--jvp]"""
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

want_jvp = "--jvp" in sys.argv
if want_jvp:
    sys.argv.remove("--jvp")
parts_list = []
while "--parts" in sys.argv:
    i = sys.argv.index("--parts")
    parts_list.append(int(sys.argv[i + 1]))
    del sys.argv[i:i + 2]
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

if want_jvp:
    # SPRING's call: dh_ntk_jvp (T and jv in one reverse walk) against dh_ntk_part(0 of 1), the same
    # Gram work without the direction; the JVP-only call against dh_logpsi_vjp
    v = torch.randn_like(params.flat)
    nparam = sum(int(p.numel()) for p in params.values())
    jflop = 2.0 * R * nparam
    part = timed(lambda: model.ntk(params, x2, ct, part=0, nparts=1, mirror=False))
    both = timed(lambda: model.ntk_jvp(params, x2, ct, v, mirror=False))
    only = timed(lambda: model.jvp(params, x2, ct, v))
    print(f"dh_ntk_part(0 of 1) {part[0]:9.2f} ms  (min {part[1]:.2f}, max {part[2]:.2f})")
    print(f"dh_ntk_jvp (with T) {both[0]:9.2f} ms  (min {both[1]:.2f}, max {both[2]:.2f}): {both[0] / part[0]:.4f} of "
          f"dh_ntk_part(0 of 1)")
    print(f"dh_ntk_jvp (T null) {only[0]:9.2f} ms  (min {only[1]:.2f}, max {only[2]:.2f}); "
          f"dh_logpsi_vjp {vjp[0]:.2f} ms")
    print(f"JVP FLOP = 2 R P = {jflop:.3e} (P = {nparam})")
    for label, dt in (("(with T) - dh_ntk_part", both[0] - part[0]), ("(T null) - dh_logpsi_vjp", only[0] - vjp[0])):
        if dt > 0:
            rate = jflop / (dt * 1e-3)
            print(f"JVP FLOP / ({label} = {dt:.2f} ms): {rate / 1e12:6.1f} TF/s = {rate / PEAK_F32_MATRIX:.3f} of peak "
                  f"(the difference also holds the packing, cvec and row-dot launches)")

if parts_list:
    from deephall_amd.optimizers import minsr_matrix  # noqa: E402

    one = timed(lambda: model.ntk(params, x2, ct, part=0, nparts=1, mirror=True))
    print(f"dh_ntk_part(0 of 1) + dh_ntk_mirror {one[0]:9.2f} ms  (min {one[1]:.2f}, max {one[2]:.2f}): "
          f"{one[0] / ntk[0]:.4f} of dh_ntk")
    for R_ in parts_list:
        ts = [timed(lambda p=p: model.ntk(params, x2, ct, part=p, nparts=R_, mirror=False)) for p in range(R_)]
        med = [t[0] for t in ts]
        print(f"dh_ntk_part(p of {R_}): " + " ".join(f"{m:.2f}" for m in med) + " ms")
        print(f"  slowest {max(med):.2f} ms = {max(med) / (ntk[0] / R_):.3f} of dh_ntk / {R_} ({ntk[0] / R_:.2f} ms); "
              f"fastest {min(med):.2f} ms; less the VJP's {vjp[0]:.2f} ms every part repeats: "
              f"{(max(med) - vjp[0]) / ((ntk[0] - vjp[0]) / R_):.3f} of the Gram products' share")

    def matrix_bench(T, label):
        M = T.shape[0]
        Bg = M // 2
        valid = torch.ones(Bg, dtype=torch.bool, device="cuda")
        valid[Bg // 3] = False

        def torch_assembly():
            Td = T.double()
            v = valid.double()
            n = v.sum().clamp(min=1.0)

            def centre(a):
                a = a * v
                return a - v * (a.sum(-1, keepdim=True) / n)

            T4 = centre(Td.view(2, Bg, 2, Bg))
            T4 = centre(T4.permute(2, 3, 0, 1)).permute(2, 3, 0, 1)
            return T4.reshape(M, M) / n + 1e-3 * torch.eye(M, dtype=torch.float64, device="cuda")

        ref = torch_assembly()
        err = float((minsr_matrix(T, valid, 1e-3) - ref).abs().max() / ref.abs().max())
        del ref
        fused = timed(lambda: minsr_matrix(T, valid, 1e-3))
        eager = timed(torch_assembly)
        byts = 16.0 * M * M
        print(f"dh_minsr_matrix ({label}, M = {M}) {fused[0]:9.3f} ms  (min {fused[1]:.3f}, max {fused[2]:.3f}): "
              f"{byts / (fused[0] * 1e-3) / 1e12:.2f} TB/s of 16 M^2 = {byts / 1e9:.2f} GB; "
              f"torch assembly {eager[0]:.2f} ms (min {eager[1]:.2f}, max {eager[2]:.2f}), {eager[0] / fused[0]:.1f} x; "
              f"max |difference| / max |A| {err:.2e}")

    matrix_bench(model.ntk(params, x2, ct), "this call's T")
    # twice the walkers (two ranks' gathered batch): a synthetic symmetric T, past the 256 MiB Infinity Cache
    S = torch.randn(4 * B, 4 * B, device="cuda")
    S = S + S.t()
    matrix_bench(S, "synthetic T of twice the walkers")
