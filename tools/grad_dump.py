"""Every output of the gradient-side entry points (dh_logpsi_vjp, dh_kfac_vjp, dh_ntk, dh_ntk_part,
dh_ntk_jvp) for seeded inputs, through the library named by DH_LIB_PATH, saved to one .npz, so two
builds can be compared bitwise:  DH_LIB_PATH=ab/X.so python tools/grad_dump.py out.npz
(then ``python tools/grad_dump.py --compare a.npz b.npz``: numpy.array_equal on uint32 views).

The cases are the smallest that reach every branch of the reverse walk (csrc/api_grad.cpp): the
split-bf16 and the exact-f32 backward GEMMs (D = 256 / 16), one and two spin blocks, "full" and
"sparse" orbitals, several weight-gradient chunks and LayerNorm blocks (540 rows), walker chunks
(acc = 1), the Fisher pass with and without a cotangent, Gram tiles with a partial last one, parts,
and the JVP with and without T."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

# (config, orbital type, walkers, layers or None for the default, walker-chunk size or None)
VJP_CASES = [("C1", "full", 8, None, None), ("MIX", "full", 8, None, None), ("C1", "sparse", 6, None, None),
             ("MIX", "sparse", 6, None, None), ("C2", "full", 90, 2, None), ("C2", "full", 24, None, 7)]
KFAC_CASES = [("C1", "full", 8, 2, None), ("MIX", "full", 8, 1, None), ("C2", "full", 90, 2, None),
              ("C1", "sparse", 8, 1, None), ("MIX", "sparse", 6, 1, None), ("C2", "sparse", 4, 1, None),
              ("C1", "full", 24, 2, 7)]
NTK_CASES = [("C1", 8), ("MIX", 8), ("C2", 90)]


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B.files))
           if k not in A.files or k not in B.files or A[k].shape != B[k].shape
           or not np.array_equal(A[k].view(np.uint32), B[k].view(np.uint32))]
    print(f"{len(A.files)} arrays in {a}, {len(B.files)} in {b}: " + (f"DIFFERENT: {bad}" if bad else "all bit-identical"))
    return 1 if bad else 0


def main():
    import torch
    from deephall_amd import config, make_network
    from deephall_amd.networks import psiformer as pf
    from helpers import make_params, make_walkers, oracle_config, to_device_params

    cuda = torch.device("cuda")
    out = {}

    def setup(name, B, seed, **over):
        ocfg = oracle_config(name, **{k: v for k, v in over.items() if v is not None})
        system = config.System(nspins=tuple(ocfg.nspins), flux=ocfg.flux)
        net = config.Network()
        net.psiformer.num_heads, net.psiformer.heads_dim = ocfg.num_heads, ocfg.heads_dim
        net.psiformer.num_layers, net.psiformer.determinants = ocfg.num_layers, ocfg.determinants
        net.orbital = config.OrbitalType(getattr(ocfg, "orbital", "full"))
        model = make_network(system, net)
        params = to_device_params(make_params(ocfg))
        x = torch.tensor(make_walkers(B, ocfg.nelec, seed=seed), device=cuda)
        ct = torch.tensor(np.random.default_rng(seed + 1).standard_normal((B, 2)), dtype=torch.float32, device=cuda)
        return model, params, x, ct

    def chunked(tag, model, params, x, chunk, size_fn, call):
        """call() with the VJP workspace capped at `chunk` walkers' worth (None: uncapped).  The handle's
        cached workspace is dropped first (a larger one from an earlier case of the same network would be
        handed back and the call would not chunk); prints the walkers per chunk the library then takes
        (its rule: halve, rounding up, until a chunk's workspace fits) and requires more than one chunk."""
        old = pf.VJP_WORKSPACE_BYTES
        try:
            if chunk:
                h = model.prepare(params, x.device)
                pf.VJP_WORKSPACE_BYTES = getattr(h.lib, size_fn)(h.h, chunk)
                h.ws.clear()
            call()
            if chunk:
                got = h.workspace(0).numel()
                B = per = x.shape[0]
                while per > 1 and getattr(h.lib, size_fn)(h.h, per) > got:
                    per = (per + 1) // 2
                print(f"{tag}: workspace {got} bytes, {per} walkers per chunk, {-(-B // per)} chunks")
                assert per < B, f"{tag}: the call did not chunk"
                h.ws.clear()  # the next case sizes its own
        finally:
            pf.VJP_WORKSPACE_BYTES = old

    def keep(key, t):
        torch.cuda.synchronize()
        out[key] = t.detach().float().cpu().numpy().copy()

    for i, (name, orbital, B, L, chunk) in enumerate(VJP_CASES):
        model, params, x, ct = setup(name, B, 100 + i, orbital=orbital, num_layers=L)
        tag = f"vjp/{name}_{orbital}_B{B}" + (f"_L{L}" if L else "") + (f"_chunk{chunk}" if chunk else "")
        g = pf.ParamTree.zeros(model.spec, cuda)
        lp = torch.zeros(B, 2, device=cuda)
        chunked(tag, model, params, x, chunk, "dh_vjp_workspace_bytes",
                lambda: model.vjp(params, x, ct, out=g, logpsi=lp))
        keep(tag + "/grad", g.flat)
        keep(tag + "/logpsi", lp)

    for i, (name, orbital, B, L, chunk) in enumerate(KFAC_CASES):
        model, params, x, ct = setup(name, B, 200 + i, orbital=orbital, num_layers=L)
        tag = f"kfac/{name}_{orbital}_B{B}_L{L}" + (f"_chunk{chunk}" if chunk else "")
        nstats = model.kfac_layout(cuda)["nstats"]
        for with_ct in (True, False):
            g = pf.ParamTree.zeros(model.spec, cuda) if with_ct else None
            stats = torch.zeros(nstats, device=cuda)
            lp = torch.zeros(B, 2, device=cuda)
            sub = tag + ("/ct" if with_ct else "/noct")
            chunked(sub, model, params, x, chunk, "dh_kfac_workspace_bytes",
                    lambda: model.kfac_vjp(params, x, ct if with_ct else None, g, stats, logpsi=lp))
            keep(sub + "/stats", stats)
            keep(sub + "/logpsi", lp)
            if with_ct:
                keep(sub + "/grad", g.flat)

    for i, (name, B) in enumerate(NTK_CASES):
        model, params, x, ct = setup(name, B, 300 + i)
        tag = f"ntk/{name}_B{B}"
        v = torch.tensor(np.random.default_rng(400 + i).standard_normal(pf.ref_offsets(model.spec)[-1]),
                         dtype=torch.float32, device=cuda)
        lp = torch.zeros(B, 2, device=cuda)
        keep(tag + "/ntk/T", model.ntk(params, x, ct, logpsi=lp))
        keep(tag + "/ntk/logpsi", lp)
        for p in range(3):
            keep(tag + f"/part{p}of3/T", model.ntk(params, x, ct, part=p, nparts=3, mirror=False))
        for p in range(2):
            T, jv = model.ntk_jvp(params, x, ct, v, part=p, nparts=2, mirror=False)
            keep(tag + f"/jvp{p}of2/T", T)
            keep(tag + f"/jvp{p}of2/jv", jv)
        lp = torch.zeros(B, 2, device=cuda)
        keep(tag + "/jvp_noT/jv", model.jvp(params, x, ct, v, logpsi=lp))
        keep(tag + "/jvp_noT/logpsi", lp)

    np.savez(sys.argv[1], **out)
    bad = sum(int((~np.isfinite(a)).sum()) for a in out.values())
    print(sys.argv[1], f"{len(out)} arrays, non-finite entries: {bad}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
