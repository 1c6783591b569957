"""One-body density matrix resolved by Landau level: rho in the basis Y_{Q,Q+n,m}, n < levels.

Not in the reference, whose one_rdm.py projects onto the lowest level only (its
make_monopole_harm has the general l but is called with l = Q): ``one_rdm``'s trace says how
much weight left the lowest Landau level, this estimator says where it went.

    rho_ij = 4 pi < sum_a psi(R_a') / psi(R) Y_i(r_a) conj(Y_j(r')) >

with r' uniform on the sphere and R_a' the walker with electron a at r'.  The orbitals are
level-major, m ascending inside a level: norb = levels (flux + 1) + levels (levels - 1).
The displaced rows (``dh_rdm_displace``), the harmonics and the reduction over walkers and
points (``dh_rdm_accumulate``: double, a fixed order, samples with a non-finite log-amplitude or
ratio dropped as ``estimator._batch_mean`` drops NaN walkers) are HIP kernels (csrc/rdm.hip);
only rho [S, norb, norb] leaves the device.

Options: ``levels`` (default 2, 1..4) Landau levels in the basis; ``points`` (default 1) draws
of r' per walker per step, each costing B N forward rows — more draws cut the variance of the r'
integral without a longer walk; ``by_spin`` (default false) rho as an up and a down block.  The
points of a step are ONE ``init_guess`` draw of points x B single-electron walkers with the
step's key (point p of walker b is draw p B + b: ``init_guess`` reads the key's seed, not its
counter, so advancing the key would repeat the point); with points = 1 that is ``one_rdm``'s r'.
Step value ``ll_rdm`` [1, S, norb, norb] complex128 (the sample mean; the driver averages axis
0); state ``samples`` (the (walker, point) samples kept, summed over steps).
"""

from __future__ import annotations

import math

import torch

from ...train import init_guess
from .._native import rdm_ll_sums
from ..estimator import Estimator, Observable

MAX_LEVELS = 4
CHUNK_POINTS = 4  # points per wavefunction call: about 4 B N displaced rows in flight


def ll_options(options) -> tuple[int, int, bool]:
    """(levels, points, by_spin) of the estimator options, validated."""
    options = options or {}
    levels, points = options.get("levels", 2), options.get("points", 1)
    if not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"ll_rdm: levels must be an int in 1..{MAX_LEVELS}, got {levels!r}")
    if not isinstance(points, int) or points < 1:
        raise ValueError(f"ll_rdm: points must be a positive int, got {points!r}")
    return levels, points, bool(options.get("by_spin", False))


def level_slices(flux: int, levels: int) -> list[slice]:
    """The orbitals of each level: level n holds flux + 1 + 2 n of them."""
    out, start = [], 0
    for n in range(levels):
        out.append(slice(start, start + flux + 1 + 2 * n))
        start += flux + 1 + 2 * n
    return out


def orbital_lz(flux: int, levels: int) -> torch.Tensor:
    """t = Q + m of every orbital (an integer): -n..flux + n in level n."""
    return torch.cat([torch.arange(-n, flux + n + 1) for n in range(levels)])


class LLRDM(Observable):
    def shapeof(self, system) -> tuple[int, ...]:
        levels, _, by_spin = ll_options(self.options)
        norb = levels * (system["flux"] + 1) + levels * (levels - 1)
        return (2 if by_spin else 1, norb, norb)


class LLRDMEstimator(Estimator):
    observable_type = LLRDM

    def __init__(self, adaptor, system, estimator_options, observable_options):
        self.levels, self.points, self.by_spin = ll_options(estimator_options)
        super().__init__(adaptor, system, estimator_options,
                         {**(observable_options or {}), "levels": self.levels, "by_spin": self.by_spin})
        self.flux = int(system["flux"])
        self.nspins = (int(system["spins"][0]), int(system["spins"][1]))

    def empty_val_state(self, steps: int):
        return {"ll_rdm": torch.zeros((steps, *self.observable.shape), dtype=torch.complex128)}, {"samples": 0}

    def accumulate(self, params, x: torch.Tensor, r_prime: torch.Tensor):
        """(sum over the kept samples of 4 pi u conj(v) [S, norb, norb] complex128 on the device, the
        number kept) for walkers x [B, N, 2] and points r_prime [P, B, 2]."""
        return rdm_ll_sums(lambda rows: self.adaptor.call_network(params, rows), x, r_prime, self.nspins[0],
                           self.flux, self.levels, self.by_spin, CHUNK_POINTS)

    def evaluate(self, i, params, key, data, system, state, aux_data):
        del i, aux_data, system
        x = data.reshape(-1, *data.shape[-2:])
        B = x.shape[0]
        r_prime = init_guess(key, self.points * B, 1, x.device, network=self.adaptor.model)[:, 0, :]
        rho, nvalid = self.accumulate(params, x, r_prime.reshape(self.points, B, 2))
        state["samples"] = state["samples"] + nvalid
        return {"ll_rdm": (rho / nvalid).cpu()[None]}, state  # nvalid = 0: NaN, which the driver's mean drops

    def digest(self, all_values, state):
        del state
        steps = all_values["ll_rdm"]                                   # [steps, S, norb, norb]
        rho = steps.mean(dim=0)
        blocks = level_slices(self.flux, self.levels)
        diag = torch.diagonal(steps, dim1=-2, dim2=-1).real            # [steps, S, norb]
        occ_steps = torch.stack([diag[..., sl].sum(-1) for sl in blocks], dim=-1)  # [steps, S, levels]
        occ = occ_steps.mean(dim=0)
        n = steps.shape[0]
        err = occ_steps.std(dim=0, unbiased=True) / math.sqrt(n) if n > 1 else torch.full_like(occ, math.nan)
        nelec = sum(self.nspins)
        dagger = rho.conj().transpose(-1, -2)
        lz = orbital_lz(self.flux, self.levels)
        off = (lz[:, None] != lz[None, :]).to(rho.real.dtype)          # 1 where m != m'
        norm = torch.linalg.norm(rho)
        return {
            "ll_rdm": rho,
            "occupations": occ,
            "occupations_err": err,
            "lll_weight": occ[..., 0].sum() / nelec,
            "residual": nelec - occ.sum(),
            "diagonal": torch.diagonal(rho, dim1=-2, dim2=-1),
            "trace": torch.diagonal(rho, dim1=-2, dim2=-1).sum(-1),
            "natural_occupations": torch.linalg.eigvalsh((rho + dagger) / 2),
            "hermiticity": torch.linalg.norm(rho - dagger) / norm if norm > 0 else torch.zeros(()).double(),
            "lz_offdiag": (rho.abs() * off).max(),
        }


DEFAULT = LLRDMEstimator  # Useful in CLI
