"""Thin wrappers of the NetObs kernels (csrc/netobs.hip).  No CPU path: the library must load."""

from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from ..networks.psiformer import _ptr, _stream


def _check_cuda(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("NetObs estimators run on the GPU (HIP kernels); got a CPU tensor")
    return t.contiguous().float()


def histograms(x: torch.Tensor, density_bins: int = 0, pair_bins: int = 0):
    """Unnormalised theta histogram and 1/sin-weighted pair-angle histogram of walkers x[B, N, 2]."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    dens = torch.zeros(max(density_bins, 1), dtype=torch.float32, device=x.device)
    pair = torch.zeros(max(pair_bins, 1), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.dh_histograms(_ptr(x), B, N, density_bins, pair_bins, _ptr(dens), _ptr(pair), _stream(x.device)))
    return dens[:density_bins], pair[:pair_bins]


def monopole_orbitals(points: torch.Tensor, flux: int) -> torch.Tensor:
    """Y_{Q,Q,m}(points), m = -Q..Q: complex64 [..., flux + 1] (one_rdm.py:31-54)."""
    pts = _check_cuda(points)
    shape = pts.shape[:-1]
    flat = pts.reshape(-1, 2)
    out = torch.empty(flat.shape[0], flux + 1, 2, dtype=torch.float32, device=pts.device)
    lib = _lib.load()
    _lib.check(lib.dh_monopole_orbitals(_ptr(flat), flat.shape[0], int(flux), _ptr(out), _stream(pts.device)))
    return torch.view_as_complex(out).reshape(*shape, flux + 1)


# ---- Renyi-2 swap estimator (csrc/swap.hip) ----------------------------------------------------

def _swap_args(x: torch.Tensor, thetas, nspins):
    x = _check_cuda(x)
    B, N, _ = x.shape
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    th = [float(t) for t in thetas]
    return x, B, N, n_up, n_dn, (C.c_float * len(th))(*th), len(th)


def swap_classify(x: torch.Tensor, thetas, nspins):
    """sector[A, P] int32 (-1: unmatched) and counts[A, K] int32 of pairs (p, p + P), P = B // 2."""
    x, B, N, n_up, n_dn, th, A = _swap_args(x, thetas, nspins)
    K = (n_up + 1) * (n_dn + 1)
    sector = torch.empty(A, B // 2, dtype=torch.int32, device=x.device)
    counts = torch.zeros(A, K, dtype=torch.int32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.dh_swap_classify(_ptr(x), B, N, n_up, n_dn, th, A, _ptr(sector), _ptr(counts), _stream(x.device)))
    return sector, counts


def swap_compact(x: torch.Tensor, thetas, nspins, sector: torch.Tensor):
    """(M, start[A + 1], pair[M], xs[2 M, N, 2]): the matched pairs' rows and swapped configurations.

    Reads M back from the device (one synchronisation); pair and xs are views of buffers sized for
    every pair matched."""
    x, B, N, n_up, n_dn, th, A = _swap_args(x, thetas, nspins)
    P = B // 2
    lib = _lib.load()
    start = torch.empty(A + 1, dtype=torch.int32, device=x.device)
    pair = torch.empty(A * P, dtype=torch.int32, device=x.device)
    xs = torch.empty(2 * A * P, N, 2, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(lib.dh_swap_workspace_bytes(B, A)), 1), dtype=torch.uint8, device=x.device)
    _lib.check(lib.dh_swap_compact(_ptr(x), B, N, n_up, n_dn, th, A, _ptr(sector), _ptr(start), _ptr(pair), _ptr(xs),
                                   _ptr(ws), ws.numel(), _stream(x.device)))
    M = int(start[A].item())
    return M, start, pair[:M], xs[:2 * M]


def swap_reduce(logpsi: torch.Tensor, logpsi_s: torch.Tensor | None, nspins, M: int, pair, sector, start):
    """sums[A, K] complex128 from logpsi[B, 2] and logpsi_s[2 M, 2] float32 (dh_logpsi's layout)."""
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    A, K = sector.shape[0], (n_up + 1) * (n_dn + 1)
    logpsi = _check_cuda(logpsi)
    logpsi_s = _check_cuda(logpsi_s) if M else None
    sums = torch.empty(A, K, 2, dtype=torch.float64, device=logpsi.device)
    lib = _lib.load()
    _lib.check(lib.dh_swap_reduce(_ptr(logpsi), _ptr(logpsi_s), logpsi.shape[0], n_up + n_dn, n_up, n_dn, A, int(M),
                                  _ptr(pair if M else None), _ptr(sector), _ptr(start), _ptr(sums),
                                  _stream(logpsi.device)))
    return torch.view_as_complex(sums)


def _log_pairs(lp: torch.Tensor) -> torch.Tensor:
    """Complex log psi [rows] -> float32 [rows, 2] (re, im), as dh_logpsi writes it."""
    return torch.view_as_real(lp.to(torch.complex64)).contiguous()


def swap_purity(apply, x: torch.Tensor, thetas, nspins):
    """Swap-estimator sums of walkers x[B, N, 2] paired (p, p + B // 2) over the caps theta < thetas[a].

    ``apply`` gives complex log psi of [rows, N, 2]: one call on x, one batched call on the 2 M
    swapped rows of the matched pairs (skipped when M = 0).  Returns sums[A, K] complex128 —
    sums.sum(-1) / (B // 2) estimates Tr rho_A^2 — and counts[A, K] int64, the sector counts of
    all 2 (B // 2) pair members."""
    x = _check_cuda(x)
    sector, counts = swap_classify(x, thetas, nspins)
    M, start, pair, xs = swap_compact(x, thetas, nspins, sector)
    logpsi = _log_pairs(apply(x))
    logpsi_s = _log_pairs(apply(xs)) if M else None
    return swap_reduce(logpsi, logpsi_s, nspins, M, pair, sector, start), counts.long()


# ---- total spin by up-down exchange (csrc/spin.hip) -----------------------------------------------

def spin_exchange(x: torch.Tensor, nspins, pair0: int = 0, pair1: int | None = None) -> torch.Tensor:
    """xs[pair1 - pair0, B, N, 2]: xs[p - pair0, b] is walker b of x[B, N, 2] with the slots of pair
    p = i n_dn + (j - n_up) (an up slot i, a down slot j) exchanged.  pair1 None: all n_up n_dn pairs."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    pair1 = n_up * n_dn if pair1 is None else int(pair1)
    xs = torch.empty(max(pair1 - int(pair0), 0), B, N, 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dh_spin_exchange(_ptr(x), B, N, n_up, n_dn, int(pair0), pair1, _ptr(xs), _stream(x.device)))
    return xs


def spin_workspace(B: int, nspins, device) -> torch.Tensor:
    """The buffer dh_spin_ratios fills and dh_spin_reduce reads (float64: 16-byte aligned)."""
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    nbytes = int(_lib.load().dh_spin_workspace_bytes(int(B), n_up, n_dn))
    if nbytes < 1:
        raise ValueError(f"spin_square: B = {B}, nspins = {tuple(nspins)} outside B >= 1, 1 <= N <= 32, B n_up n_dn < 2^31")
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def spin_ratios(logpsi: torch.Tensor, logpsi_s: torch.Tensor, nspins, pair0: int, pair1: int, ws: torch.Tensor):
    """Store exp(logpsi_s - logpsi) of the pairs [pair0, pair1) in ws; logpsi [B, 2] and logpsi_s
    [(pair1 - pair0) B, 2] float32 (dh_logpsi's layout; rows as spin_exchange orders them)."""
    logpsi, logpsi_s = _check_cuda(logpsi), _check_cuda(logpsi_s)
    B = logpsi.shape[0]
    if logpsi.shape != (B, 2) or logpsi_s.shape != ((int(pair1) - int(pair0)) * B, 2):
        raise ValueError(f"spin_ratios: shapes {tuple(logpsi.shape)}, {tuple(logpsi_s.shape)} do not fit the "
                         f"pairs {pair0}..{pair1}")
    _lib.check(_lib.load().dh_spin_ratios(_ptr(logpsi), _ptr(logpsi_s), B, int(nspins[0]), int(nspins[1]), int(pair0),
                                          int(pair1), _ptr(ws), ws.numel() * 8, _stream(logpsi.device)))


def spin_reduce(logpsi: torch.Tensor, nspins, ws: torch.Tensor):
    """(s2[B] complex128, S^2_loc per walker and NaN for an invalid one; pairs[n_up, n_dn]
    complex128, the valid walkers' sums of each pair's ratio; total, their sum of s2; nvalid) once
    every pair is in ws.  nvalid is read back from the device (one synchronisation)."""
    logpsi = _check_cuda(logpsi)
    B = logpsi.shape[0]
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    dev = logpsi.device
    s2 = torch.empty(B, 2, dtype=torch.float64, device=dev)
    pairs = torch.zeros(n_up, n_dn, 2, dtype=torch.float64, device=dev)
    total = torch.empty(2, dtype=torch.float64, device=dev)
    nvalid = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().dh_spin_reduce(_ptr(logpsi), B, n_up, n_dn, _ptr(ws), ws.numel() * 8, _ptr(s2),
                                          _ptr(pairs) if n_up * n_dn else None, _ptr(total), _ptr(nvalid), _stream(dev)))
    return torch.view_as_complex(s2), torch.view_as_complex(pairs), torch.view_as_complex(total), int(nvalid.item())


def spin_square_sums(apply, x: torch.Tensor, nspins, max_rows: int | None = None):
    """spin_reduce's results with the log-amplitudes from ``apply`` (complex log psi of
    [rows, N, 2]): one call on x, then the exchanged rows of whole pairs, at most ``max_rows``
    rows (and at least one pair) per call; None: all n_up n_dn pairs in one call."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    P = int(nspins[0]) * int(nspins[1])
    ws = spin_workspace(B, nspins, x.device)
    logpsi = _log_pairs(apply(x))
    step = P if max_rows is None else max(1, int(max_rows) // B)
    for p0 in range(0, P, max(step, 1)):
        p1 = min(p0 + step, P)
        xs = spin_exchange(x, nspins, p0, p1)
        spin_ratios(logpsi, _log_pairs(apply(xs.reshape(-1, N, 2))), nspins, p0, p1, ws)
    return spin_reduce(logpsi, nspins, ws)


# ---- Landau-level-resolved one-body density matrix (csrc/rdm.hip) --------------------------------

def rdm_norb(flux: int, levels: int) -> int:
    """Orbitals Y_{Q,Q+n,m} of the levels n < levels: levels (flux + 1) + levels (levels - 1)."""
    norb = int(_lib.load().dh_rdm_norb(int(flux), int(levels)))
    if norb < 1:
        raise ValueError(f"ll_rdm: flux {flux} outside 0..126 or levels {levels} outside 1..{_lib.DH_RDM_MAX_LEVELS}")
    return norb


def monopole_harmonics(points: torch.Tensor, flux: int, levels: int) -> torch.Tensor:
    """Y_{Q,Q+n,m}(points), level-major, m ascending: complex64 [..., norb]; level 0 is monopole_orbitals."""
    pts = _check_cuda(points)
    shape = pts.shape[:-1]
    flat = pts.reshape(-1, 2)
    norb = rdm_norb(flux, levels)
    out = torch.empty(flat.shape[0], norb, 2, dtype=torch.float32, device=pts.device)
    lib = _lib.load()
    _lib.check(lib.dh_monopole_harmonics(_ptr(flat), flat.shape[0], int(flux), int(levels), _ptr(out),
                                         _stream(pts.device)))
    return torch.view_as_complex(out).reshape(*shape, norb)


def rdm_displace(x: torch.Tensor, r_prime: torch.Tensor) -> torch.Tensor:
    """xp[P, B, N, N, 2]: xp[p, b, a] is walker b of x[B, N, 2] with electron a at r_prime[p, b]."""
    x, r_prime = _check_cuda(x), _check_cuda(r_prime)
    B, N, _ = x.shape
    P = r_prime.shape[0]
    if r_prime.shape != (P, B, 2):
        raise ValueError(f"rdm_displace: r_prime must be [P, {B}, 2], got {tuple(r_prime.shape)}")
    xp = torch.empty(P, B, N, N, 2, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.dh_rdm_displace(_ptr(x), _ptr(r_prime), B, N, P, _ptr(xp), _stream(x.device)))
    return xp


def rdm_accumulate(x: torch.Tensor, r_prime: torch.Tensor, logpsi: torch.Tensor, logpsi_p: torch.Tensor, n_up: int,
                   flux: int, levels: int, by_spin: bool = False):
    """(rho[S, norb, norb] complex128, nvalid): the SUM over the kept (walker, point) samples of
    4 pi u_i conj(v_j) from x[B, N, 2], r_prime[P, B, 2], logpsi[B, 2] and logpsi_p[P B N, 2]
    float32 (dh_logpsi's layout; rows as rdm_displace orders them).  S = 2 (up, down) when by_spin.
    nvalid is read back from the device (one synchronisation)."""
    x, r_prime = _check_cuda(x), _check_cuda(r_prime)
    logpsi, logpsi_p = _check_cuda(logpsi), _check_cuda(logpsi_p)
    B, N, _ = x.shape
    P = r_prime.shape[0]
    if r_prime.shape != (P, B, 2) or logpsi.shape != (B, 2) or logpsi_p.shape != (P * B * N, 2):
        raise ValueError(f"rdm_accumulate: shapes {tuple(r_prime.shape)}, {tuple(logpsi.shape)}, "
                         f"{tuple(logpsi_p.shape)} do not fit x {tuple(x.shape)}")
    norb, S = rdm_norb(flux, levels), 2 if by_spin else 1
    lib = _lib.load()
    rho = torch.empty(S, norb, norb, 2, dtype=torch.float64, device=x.device)
    nvalid = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(int(lib.dh_rdm_workspace_bytes(B, N, int(flux), int(levels), P)), 1), dtype=torch.uint8,
                     device=x.device)
    _lib.check(lib.dh_rdm_accumulate(_ptr(x), _ptr(r_prime), _ptr(logpsi), _ptr(logpsi_p), B, N, int(n_up), int(flux),
                                     int(levels), P, int(bool(by_spin)), _ptr(rho), _ptr(nvalid), _ptr(ws), ws.numel(),
                                     _stream(x.device)))
    return torch.view_as_complex(rho), int(nvalid.item())


def rdm_ll_sums(apply, x: torch.Tensor, r_prime: torch.Tensor, n_up: int, flux: int, levels: int,
                by_spin: bool = False, chunk_points: int = 4):
    """rdm_accumulate's (rho, nvalid) with the log-amplitudes from ``apply`` (complex log psi of
    [rows, N, 2]): one call on x, then the displaced rows of ``chunk_points`` points at a time, so
    at most chunk_points B N rows are in flight."""
    x, r_prime = _check_cuda(x), _check_cuda(r_prime)
    B, N, _ = x.shape
    logpsi = _log_pairs(apply(x))
    parts = []
    for p0 in range(0, r_prime.shape[0], chunk_points):
        xp = rdm_displace(x, r_prime[p0:p0 + chunk_points])
        parts.append(_log_pairs(apply(xp.reshape(-1, N, 2))))
    return rdm_accumulate(x, r_prime, logpsi, torch.cat(parts), n_up, flux, levels, by_spin)


# ---- pair amplitudes (csrc/pairamp.hip) -------------------------------------------------------------

def _pair_points(x: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor, who: str):
    x, r1, r2 = _check_cuda(x), _check_cuda(r1), _check_cuda(r2)
    B, N, _ = x.shape
    P = r1.shape[0]
    if r1.shape != (P, B, 2) or r2.shape != (P, B, 2):
        raise ValueError(f"{who}: r1 and r2 must be [P, {B}, 2], got {tuple(r1.shape)}, {tuple(r2.shape)}")
    return x, r1, r2, B, N, P


def pair_displace(x: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor, pair0: int = 0,
                  pair1: int | None = None) -> torch.Tensor:
    """xp[pair1 - pair0, P, B, N, 2]: xp[q - pair0, p, b] is walker b of x[B, N, 2] with electron i at
    r1[p, b] and electron j at r2[p, b], q the pair (i < j) in lexicographic order.  pair1 None: all
    N (N - 1) / 2 pairs."""
    x, r1, r2, B, N, P = _pair_points(x, r1, r2, "pair_displace")
    pair1 = N * (N - 1) // 2 if pair1 is None else int(pair1)
    xp = torch.empty(max(pair1 - int(pair0), 0), P, B, N, 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().dh_pair_displace(_ptr(x), _ptr(r1), _ptr(r2), B, N, P, int(pair0), pair1, _ptr(xp),
                                            _stream(x.device)))
    return xp


def pair_kernel(points: torch.Tensor, flux: int) -> torch.Tensor:
    """(4 pi)^2 K_L(r1, r2; r1', r2'), L = 0..flux: complex128 [n, flux + 1] for points[n, 4, 2]."""
    pts = _check_cuda(points)
    n = pts.shape[0]
    if pts.shape != (n, 4, 2):
        raise ValueError(f"pair_kernel: points must be [n, 4, 2], got {tuple(pts.shape)}")
    out = torch.empty(n, int(flux) + 1, 2, dtype=torch.float64, device=pts.device)
    _lib.check(_lib.load().dh_pair_kernel(_ptr(pts), n, int(flux), _ptr(out), _stream(pts.device)))
    return torch.view_as_complex(out)


def pair_accumulate(x: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor, logpsi: torch.Tensor, logpsi_p: torch.Tensor,
                    n_up: int, flux: int):
    """(A[3, flux + 1] complex128, nvalid): the SUM over the kept (walker, point) samples and the
    up-up, up-down, down-down pairs of (4 pi)^2 K_L psi(R_{ij -> r1 r2}) / psi(R), from x[B, N, 2],
    r1, r2 [P, B, 2], logpsi[B, 2] and logpsi_p[pairs P B, 2] float32 (dh_logpsi's layout; rows as
    pair_displace orders them).  nvalid is read back from the device (one synchronisation)."""
    x, r1, r2, B, N, P = _pair_points(x, r1, r2, "pair_accumulate")
    logpsi, logpsi_p = _check_cuda(logpsi), _check_cuda(logpsi_p)
    if logpsi.shape != (B, 2) or logpsi_p.shape != (N * (N - 1) // 2 * P * B, 2):
        raise ValueError(f"pair_accumulate: shapes {tuple(logpsi.shape)}, {tuple(logpsi_p.shape)} do not fit x "
                         f"{tuple(x.shape)} and {P} points")
    lib = _lib.load()
    nbytes = int(lib.dh_pair_workspace_bytes(B, N, int(flux), P))
    if nbytes < 1:
        raise ValueError(f"pair_accumulate: B = {B}, N = {N}, flux = {flux}, P = {P} outside B, P >= 1, 1 <= N <= 32, "
                         "0 <= flux <= 126, P B <= 2^30, P B N (N - 1) / 2 < 2^31")
    A = torch.empty(3, int(flux) + 1, 2, dtype=torch.float64, device=x.device)
    nvalid = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    if logpsi_p.numel() == 0:  # N = 1: no pair and no row, but the call wants a pointer
        logpsi_p = logpsi
    _lib.check(lib.dh_pair_accumulate(_ptr(x), _ptr(r1), _ptr(r2), _ptr(logpsi), _ptr(logpsi_p), B, N, int(n_up),
                                      int(flux), P, _ptr(A), _ptr(nvalid), _ptr(ws), ws.numel() * 8,
                                      _stream(x.device)))
    return torch.view_as_complex(A), int(nvalid.item())


def pair_amplitude_sums(apply, x: torch.Tensor, r1: torch.Tensor, r2: torch.Tensor, n_up: int, flux: int,
                        max_rows: int | None = None):
    """pair_accumulate's (A, nvalid) with the log-amplitudes from ``apply`` (complex log psi of
    [rows, N, 2]): one call on x, then the displaced rows of whole pairs, at most ``max_rows`` rows
    (and at least one pair) per call; None: all pairs in one call."""
    x, r1, r2, B, N, P = _pair_points(x, r1, r2, "pair_amplitude_sums")
    npairs = N * (N - 1) // 2
    logpsi = _log_pairs(apply(x))
    step = npairs if max_rows is None else max(1, int(max_rows) // (P * B))
    parts = []
    for q0 in range(0, npairs, max(step, 1)):
        xp = pair_displace(x, r1, r2, q0, min(q0 + step, npairs))
        parts.append(_log_pairs(apply(xp.reshape(-1, N, 2))))
    logpsi_p = torch.cat(parts) if parts else torch.empty(0, 2, dtype=torch.float32, device=x.device)
    return pair_accumulate(x, r1, r2, logpsi, logpsi_p, n_up, flux)


# ---- static structure factor (csrc/sfactor.hip) ---------------------------------------------------

def sf_nlm(lmax: int) -> int:
    """Multipoles 0 <= M <= L <= lmax at lm = L (L + 1) / 2 + M: (lmax + 1)(lmax + 2) / 2."""
    nlm = int(_lib.load().dh_sf_nlm(int(lmax)))
    if nlm < 1:
        raise ValueError(f"structure_factor: lmax {lmax} outside 0..{_lib.DH_SF_MAX_L}")
    return nlm


def sf_pairs(x: torch.Tensor, n_up: int, lmax: int) -> torch.Tensor:
    """T[B, 3, lmax + 1] float64: the sums of P_L(cos gamma_ij) over the pairs i < j of walkers
    x[B, N, 2] that are both up, up and down, both down.  NaN rows for a walker with a non-finite
    coordinate."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    T = torch.empty(B, 3, int(lmax) + 1, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().dh_sf_pairs(_ptr(x), B, N, int(n_up), int(lmax), _ptr(T), _stream(x.device)))
    return T


def sf_multipoles(x: torch.Tensor, n_up: int, lmax: int) -> torch.Tensor:
    """rho[B, 2, nlm] complex128: sum_i Y_LM(theta_i, phi_i) over the up (0) and the down (1)
    electrons of each walker.  NaN rows for a walker with a non-finite coordinate."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    rho = torch.empty(B, 2, sf_nlm(lmax), 2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().dh_sf_multipoles(_ptr(x), B, N, int(n_up), int(lmax), _ptr(rho), _stream(x.device)))
    return torch.view_as_complex(rho)


def _sf_accumulate_packed(x: torch.Tensor, n_up: int, lmax: int, multipoles: bool):
    """(out, lmax + 1, nlm): one float64 device buffer filled by dh_sf_accumulate, [pair sums
    3 (lmax + 1), padded to even | rho sums 4 nlm (re, im), with multipoles | nvalid as int32]."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    lib = _lib.load()
    nl, nlm = int(lmax) + 1, sf_nlm(lmax)
    nbytes = int(lib.dh_sf_workspace_bytes(B, N, int(lmax)))
    if nbytes < 1:
        raise ValueError(f"structure_factor: B = {B}, N = {N} outside B >= 1, 1 <= N <= 32, B N < 2^31")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    nrho = 4 * nlm if multipoles else 0
    r0 = 3 * nl + (3 * nl) % 2  # an even offset: the complex view needs it
    out = torch.zeros(r0 + nrho + 1, dtype=torch.float64, device=x.device)
    pairs, rho, nvalid = out[:3 * nl], out[r0:r0 + nrho], out[r0 + nrho:]
    _lib.check(lib.dh_sf_accumulate(_ptr(x), B, N, int(n_up), int(lmax), int(bool(multipoles)), _ptr(pairs),
                                    _ptr(rho) if multipoles else None, _ptr(nvalid), _ptr(ws), ws.numel() * 8,
                                    _stream(x.device)))
    return out, nl, nlm


def _sf_unpack(out: torch.Tensor, nl: int, nlm: int, multipoles: bool):
    r0 = 3 * nl + (3 * nl) % 2
    pairs = out[:3 * nl].reshape(3, nl)
    rho = torch.view_as_complex(out[r0:r0 + 4 * nlm].reshape(2, nlm, 2)) if multipoles else None
    return pairs, rho, int(out[-1:].view(torch.int32)[0].item())


def sf_accumulate(x: torch.Tensor, n_up: int, lmax: int, multipoles: bool = True):
    """(pair_sums[3, lmax + 1] float64, rho_sums[2, nlm] complex128 or None, nvalid): sf_pairs and
    sf_multipoles summed over the walkers whose coordinates are all finite, without the per-walker
    arrays; device tensors.  nvalid is read back from the device (one synchronisation)."""
    out, nl, nlm = _sf_accumulate_packed(x, n_up, lmax, multipoles)
    return _sf_unpack(out, nl, nlm, multipoles)


def sf_accumulate_host(x: torch.Tensor, n_up: int, lmax: int, multipoles: bool = True):
    """sf_accumulate's results as host tensors, brought over in one device read."""
    out, nl, nlm = _sf_accumulate_packed(x, n_up, lmax, multipoles)
    return _sf_unpack(out.cpu(), nl, nlm, multipoles)


# ---- density around an axis (csrc/impurity.hip) ----------------------------------------------------

def axis_histogram(x: torch.Tensor, nspins, axis, bins: int) -> torch.Tensor:
    """counts[2, bins] int64 on the device: the up (row 0) and down (row 1) electrons of walkers
    x[B, N, 2] by the cosine u of their angle from ``axis`` = (theta, phi), in ``bins`` bins of equal
    area, bin k being 1 - 2 (k + 1) / bins < u <= 1 - 2 k / bins.  Non-finite coordinates are dropped."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    n_up, n_dn = int(nspins[0]), int(nspins[1])
    if n_up + n_dn != N:
        raise ValueError(f"axis_histogram: walkers of {N} electrons, nspins = {(n_up, n_dn)}")
    counts = torch.zeros(2, max(int(bins), 1), dtype=torch.int32, device=x.device)  # the kernel's unsigned
    _lib.check(_lib.load().dh_axis_histogram(_ptr(x), B, n_up, n_dn, float(axis[0]), float(axis[1]), int(bins),
                                             _ptr(counts), _stream(x.device)))
    return counts.long() & 0xFFFFFFFF


# ---- quasihole overlap matrix (csrc/quasihole.hip hole_logs_kernel, csrc/holes.hip) ---------------

class HoleTable:
    """K configurations of the pinned holes of one quasihole system, checked by ``dh_hole_table``:
    ``cfg`` and ``configs`` (the C structs), ``host`` (the packed table, uint8) and its device copies."""

    def __init__(self, cfg: _lib.DhConfig, configs: _lib.DhHoleConfigs, host: torch.Tensor):
        self.cfg, self.configs, self.host = cfg, configs, host
        self.n_configs, self.n_holes = int(configs.n_configs), int(configs.n_holes)
        self.nelec = int(cfg.n_up) + int(cfg.n_dn)
        self._device = {}

    @property
    def spinors(self) -> torch.Tensor:
        """[n_configs, n_holes, 2] complex128: (U, V) of hole a of configuration c, as the kernels hold them."""
        n = _lib.DH_HOLE_MAX_CONFIGS * _lib.DH_QUASIHOLE_MAX_HOLES * 4
        uv = self.host[:8 * n].view(torch.float64).reshape(_lib.DH_HOLE_MAX_CONFIGS, _lib.DH_QUASIHOLE_MAX_HOLES, 2, 2)
        return torch.view_as_complex(uv[:self.n_configs, :self.n_holes].contiguous())

    @property
    def kinds(self) -> torch.Tensor:
        """[n_configs, n_holes] int32: DH_HOLE_* of hole a of configuration c."""
        n = _lib.DH_HOLE_MAX_CONFIGS * _lib.DH_QUASIHOLE_MAX_HOLES
        kind = self.host[32 * n:36 * n].view(torch.int32).reshape(_lib.DH_HOLE_MAX_CONFIGS, _lib.DH_QUASIHOLE_MAX_HOLES)
        return kind[:self.n_configs, :self.n_holes]

    def on(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = self.host.to(device)
        return self._device[device]


def hole_configs(configs) -> _lib.DhHoleConfigs:
    """dh_hole_configs from quasihole states ``(base, (m_up, m_dn, n), p, ((theta, phi, kind), ...))``
    (``networks.quasihole.check_quasihole``): base, exponents and p of the first, the holes of each."""
    configs = list(configs)
    hc = _lib.DhHoleConfigs()
    hc.n_configs = len(configs)
    if not configs:
        return hc
    if len(configs) > _lib.DH_HOLE_MAX_CONFIGS:
        raise ValueError(f"Holes: need 1 <= n_configs <= {_lib.DH_HOLE_MAX_CONFIGS}, got {len(configs)}")
    base, (m_up, m_dn, n), p, holes0 = configs[0]
    hc.base = _lib.QUASIHOLE_BASES[base]
    hc.m_up, hc.m_dn, hc.n_inter, hc.p = int(m_up), int(m_dn), int(n), int(p)
    hc.n_holes = len(holes0)
    for c, state in enumerate(configs):
        if (state[0], tuple(state[1]), state[2]) != (base, (m_up, m_dn, n), p) or len(state[3]) != len(holes0):
            raise ValueError(f"Holes: configuration {c} differs from configuration 0 in its base, exponents, p or "
                             "number of holes")
        if len(state[3]) > _lib.DH_QUASIHOLE_MAX_HOLES:
            raise ValueError(f"Holes: need 1 <= n_holes <= {_lib.DH_QUASIHOLE_MAX_HOLES}, got {len(state[3])}")
        for a, (theta, phi, kind) in enumerate(state[3]):
            hc.holes[c][a][0], hc.holes[c][a][1] = float(theta), float(phi)
            hc.kind[c][a] = _lib.HOLE_KINDS[kind]
    return hc


def hole_table(spec_or_cfg, configs) -> HoleTable:
    """The checked table of ``configs`` (quasihole states, or a ready ``DhHoleConfigs``) for the system of a
    ``NetworkSpec`` or a ``DhConfig``.  Host only: no device call."""
    cfg = spec_or_cfg if isinstance(spec_or_cfg, _lib.DhConfig) else spec_or_cfg.to_c()
    hc = configs if isinstance(configs, _lib.DhHoleConfigs) else hole_configs(configs)
    lib = _lib.load()
    host = torch.zeros(int(lib.dh_hole_table_bytes()), dtype=torch.uint8)
    _lib.check(lib.dh_hole_table(C.byref(cfg), C.byref(hc), host.data_ptr(), host.numel()))
    return HoleTable(cfg, hc, host)


def hole_logs(x: torch.Tensor, table: HoleTable) -> torch.Tensor:
    """L[B, K] complex128 on the device: log psi_c of walkers x[B, N, 2] for the K configurations of ``table``;
    L[:, c] rounded to complex64 is ``dh_logpsi`` of the quasihole state with configuration c."""
    x = _check_cuda(x)
    B, N, _ = x.shape
    if N != table.nelec:
        raise ValueError(f"hole_logs: walkers of {N} electrons, a table for {table.nelec}")
    dev = table.on(x.device)
    L = torch.empty(B, table.n_configs, 2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().dh_hole_logs(C.byref(table.cfg), C.byref(table.configs), _ptr(x), B, _ptr(dev), dev.numel(),
                                        _ptr(L), _stream(x.device)))
    return torch.view_as_complex(L)


def hole_gram(L: torch.Tensor, shift: torch.Tensor | None = None):
    """(S[K, K] complex128 on the device, nvalid): S[c, c'] = sum_b conj(r[b, c]) r[b, c'] over the walkers
    whose logs L[B, K] are all finite, r[b, c] = exp(L[b, c] - L[b, 0] - shift[c]); shift [K] real, None: zeros.
    nvalid is read back from the device (one synchronisation)."""
    if not L.is_cuda:
        raise RuntimeError("NetObs estimators run on the GPU (HIP kernels); got a CPU tensor")
    Lr = torch.view_as_real(L.to(torch.complex128)).contiguous()
    B, K, _ = Lr.shape
    shift = (torch.zeros(K, dtype=torch.float64, device=L.device) if shift is None
             else torch.as_tensor(shift, dtype=torch.float64).to(L.device).contiguous())
    if shift.shape != (K,):
        raise ValueError(f"hole_gram: shift must be [{K}], got {tuple(shift.shape)}")
    lib = _lib.load()
    nbytes = int(lib.dh_hole_workspace_bytes(B, K))
    if nbytes < 1:
        raise ValueError(f"hole_gram: B = {B}, K = {K} outside B >= 1, 1 <= K <= {_lib.DH_HOLE_MAX_CONFIGS}, B K < 2^31")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=L.device)
    S = torch.empty(K, K, 2, dtype=torch.float64, device=L.device)
    nvalid = torch.empty(1, dtype=torch.int32, device=L.device)
    _lib.check(lib.dh_hole_gram(_ptr(Lr), B, K, _ptr(shift), _ptr(S), _ptr(nvalid), _ptr(ws), ws.numel() * 8,
                                _stream(L.device)))
    return torch.view_as_complex(S), int(nvalid.item())


# ---- subspace matrices of K states (csrc/subspace.hip) ---------------------------------------------

def subspace_sums(logs: torch.Tensor, e_l: torch.Tensor, ke: torch.Tensor, shift: torch.Tensor | None = None):
    """(out[3, K, K] complex128 on the device, nvalid): out[0] = S, out[1] = H, out[2] = T with
    S[c, c'] = sum_b conj(r_c) r_c', H the same sum weighted by e_l[c', b], T by ke[c', b], over the walkers
    whose inputs and ratios are all finite; r_c = exp(logs[c] - logs[0] - shift[c]).  logs, e_l, ke
    [K, B, 2] float32 (re, im; dh_local_energy's layout, stacked by state), shift [K] real, None: zeros.
    nvalid is read back from the device (one synchronisation)."""
    logs, e_l, ke = _check_cuda(logs), _check_cuda(e_l), _check_cuda(ke)
    if logs.dim() != 3 or logs.shape[2] != 2 or e_l.shape != logs.shape or ke.shape != logs.shape:
        raise ValueError(f"subspace_sums: logs, e_l, ke must be [K, B, 2] alike, got {tuple(logs.shape)}, "
                         f"{tuple(e_l.shape)}, {tuple(ke.shape)}")
    K, B, _ = logs.shape
    shift = (torch.zeros(K, dtype=torch.float64, device=logs.device) if shift is None
             else torch.as_tensor(shift, dtype=torch.float64).to(logs.device).contiguous())
    if shift.shape != (K,):
        raise ValueError(f"subspace_sums: shift must be [{K}], got {tuple(shift.shape)}")
    lib = _lib.load()
    nbytes = int(lib.dh_subspace_workspace_bytes(B, K))
    if nbytes < 1:
        raise ValueError(f"subspace_sums: B = {B}, K = {K} outside B >= 1, 1 <= K <= {_lib.DH_SUBSPACE_MAX_STATES}, "
                         "K B < 2^31")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=logs.device)
    out = torch.empty(3, K, K, 2, dtype=torch.float64, device=logs.device)
    nvalid = torch.empty(1, dtype=torch.int32, device=logs.device)
    _lib.check(lib.dh_subspace_accumulate(_ptr(logs), _ptr(e_l), _ptr(ke), B, K, _ptr(shift), _ptr(out), _ptr(nvalid),
                                          _ptr(ws), ws.numel() * 8, _stream(logs.device)))
    return torch.view_as_complex(out), int(nvalid.item())
