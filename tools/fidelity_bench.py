"""Time the dh_fidelity_partial + dh_fidelity_residual pair (B walkers, Re d ~ N(0, 3^2) + 500,
Im d ~ U(-50, 50), 3 % invalid walkers):  python tools/fidelity_bench.py [B] [calls] [repeats].
The figure to put beside tools/stats_bench.py's dh_energy_stats at the same B."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

import torch  # noqa: E402

from deephall_amd import _lib  # noqa: E402
from deephall_amd.networks.psiformer import _ptr  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    lpsi = torch.stack([-20 + 5 * torch.randn(B, generator=g), 6.28 * (torch.rand(B, generator=g) - 0.5)], -1)
    d = torch.stack([500 + 3 * torch.randn(B, generator=g), 100 * (torch.rand(B, generator=g) - 0.5)], -1)
    lphi = lpsi + d
    lpsi[::33, 0] = float("nan")
    lpsi, lphi = lpsi.cuda().contiguous(), lphi.cuda().contiguous()
    part = torch.empty(_lib.DH_NFID, dtype=torch.float64, device="cuda")
    resid = torch.empty(B, 2, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def partial():
        return lib.dh_fidelity_partial(_ptr(lpsi), _ptr(lphi), B, _ptr(part), st)

    def residual():
        return lib.dh_fidelity_residual(_ptr(lpsi), _ptr(lphi), B, _ptr(part), _ptr(resid), st)

    def pair():
        return partial() | residual()

    for name, fn in (("partial", partial), ("residual", residual), ("pair", pair)):
        for _ in range(10):
            assert fn() == 0
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times.append(1000 * t0.elapsed_time(t1) / calls)
        times.sort()
        print(f"B={B} dh_fidelity {name}: {times[len(times) // 2]:.1f} us per call "
              f"(min {times[0]:.1f}, max {times[-1]:.1f}; {repeats} x {calls} calls)")


if __name__ == "__main__":
    main()
