// Pair amplitudes in the lowest Landau level (netobs/observables/pair_amplitude.py; not in the
// reference): A_L, the mean number of electron pairs with total pair angular momentum L, that is
// relative angular momentum m = 2Q - L, flux = 2Q.
//
// Spinor of a point: u = cos(theta / 2) e^{i phi / 2}, v = sin(theta / 2) e^{-i phi / 2} (the gauge
// of the monopole harmonics), <p|q> = u_p conj(u_q) + v_p conj(v_q).  For a pair (r1, r2) and a
// primed pair (r1', r2'):
//     a = <1|1'><2|2'>,  b = <1|2'><2|1'>,  d = w12 conj(w1'2'),  w12 = u1 v2 - v1 u2  (d = a - b),
// and the projector onto pair angular momentum L, summed over M, is
//     (4 pi)^2 K_L = n_L d^(2Q - L) p_L,
//     p_0 = 1,  p_1 = a + b,  L p_L = (2L - 1)(a + b) p_{L-1} - (L - 1) d^2 p_{L-2},
//     n_L = (2Q + 1)^2 (2L + 1) / (2Q + L + 1)  C(2Q, L) / C(2Q + L, L)   (host, double, lgamma).
// Nothing divides by d (0 when r1 = r2): w12 rounds each product on its own, so d is then exactly
// 0 and only L = 2Q survives.  The recurrence runs upward in L and the powers of d downward, so a
// thread walks L in tiles of kPairTile: the tile's lowest power by squaring, the others by
// multiplication into registers (constant indices: no scratch), then the tile's p_L.
//
//   displace    one thread per float2 of xp[pair1 - pair0][P][B][N]: walker b with electron i at
//               r1[p][b] and electron j at r2[p][b], pair q = (i < j) in lexicographic order;
//               coordinates are copied.
//   kernel      one thread per quadruple: out[n][flux + 1] complex double, NaN for a quadruple
//               with a non-finite coordinate.
//   accumulate  valid: one thread per sample (sample = p B + b) reads its own log and its pairs'
//               logs; a non-finite log or ratio drops the sample whole (ok[sample] = 0; nvalid is
//               an integer atomic, whose value does not depend on the order).
//               terms: grid (chunks of kPairNT samples, pairs), one thread per sample: the ratio
//               exp(logpsi_p - logpsi) times (4 pi)^2 K_L, a tile of L at a time, block_sum over
//               the workgroup, part[pair][chunk][L].
//               finish: one workgroup per (class, L): the partials of the class's pairs (up-up,
//               up-down, down-down by the slots below or above n_up) in a fixed order, block_sum.
// Double from the log difference on, no float atomics: two calls give identical bits.  Every
// load is guarded by sample < samples; the limits are the callers' to check (dh_internal.h).
#include <cmath>

#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kPairNT = 256;   // samples per workgroup of the terms kernel
constexpr int kPairTile = 8;   // L per tile: 92 VGPRs and no scratch in the terms kernel (16: 256)

struct PairNorms {
  double n[kPairMaxFlux + 1];
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cscale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }

struct Spinor {
  double2 u, v;
};

__device__ __forceinline__ Spinor spinor(float2 r) {
  double st, ct, sp, cp;
  sincos(0.5 * (double)r.x, &st, &ct);
  sincos(0.5 * (double)r.y, &sp, &cp);
  return {make_double2(ct * cp, ct * sp), make_double2(st * cp, -(st * sp))};
}

// <p|q>
__device__ __forceinline__ double2 bracket(const Spinor& p, const Spinor& q) {
  return make_double2(p.u.x * q.u.x + p.u.y * q.u.y + (p.v.x * q.v.x + p.v.y * q.v.y),
                      p.u.y * q.u.x - p.u.x * q.u.y + (p.v.y * q.v.x - p.v.x * q.v.y));
}

// u_p v_q - v_p u_q; every product rounded before it is added, so wedge(p, p) is exactly 0
__device__ __forceinline__ double2 wedge(const Spinor& p, const Spinor& q) {
#pragma clang fp contract(off)
  const double rr = p.u.x * q.v.x, ii = p.u.y * q.v.y, ri = p.u.x * q.v.y, ir = p.u.y * q.v.x;
  const double srr = p.v.x * q.u.x, sii = p.v.y * q.u.y, sir = p.v.y * q.u.x, sri = p.v.x * q.u.y;
  return make_double2((rr - ii) - (srr - sii), (ri + ir) - (sir + sri));
}

struct PairGeom {
  double2 s, d, d2;  // a + b, d, d^2
};

__device__ __forceinline__ PairGeom pair_geom(float2 r1, float2 r2, float2 r1p, float2 r2p) {
  const Spinor s1 = spinor(r1), s2 = spinor(r2), t1 = spinor(r1p), t2 = spinor(r2p);
  const double2 a = cmul(bracket(s1, t1), bracket(s2, t2)), b = cmul(bracket(s1, t2), bracket(s2, t1));
  const double2 w = wedge(s1, s2), wp = wedge(t1, t2);
  const double2 d = make_double2(w.x * wp.x + w.y * wp.y, w.y * wp.x - w.x * wp.y);  // w conj(wp)
  return {make_double2(a.x + b.x, a.y + b.y), d, cmul(d, d)};
}

// d^e, e >= 0, by squaring
__device__ __forceinline__ double2 cpow(double2 d, int e) {
  double2 r = make_double2(1.0, 0.0);
  for (; e > 0; e >>= 1) {
    if (e & 1) r = cmul(r, d);
    d = cmul(d, d);
  }
  return r;
}

// k[l] = (4 pi)^2 K_L at L = L0 + l (0 past flux).  p and pm are p_{L0-1} and p_{L0-2} on entry
// (1 and 0 at L0 = 0) and the last two of the tile on return.
__device__ __forceinline__ void pair_tile(const PairGeom& g, int flux, int L0, const PairNorms& nrm, double2& p,
                                          double2& pm, double2 (&k)[kPairTile]) {
  // pw[l] = d^(flux - L0 - l): the lowest exponent of the tile first, the rest upward from it
  const int e0 = max(flux - L0 - (kPairTile - 1), 0);
  double2 pw[kPairTile];
  double2 cur = cpow(g.d, e0);
#pragma unroll
  for (int l = kPairTile - 1; l >= 0; --l) {
    if (flux - L0 - l > e0) cur = cmul(cur, g.d);
    pw[l] = cur;
  }
#pragma unroll
  for (int l = 0; l < kPairTile; ++l) {
    const int L = L0 + l;
    if (L > flux) {
      k[l] = make_double2(0.0, 0.0);
      continue;
    }
    if (L > 0) {
      const double rl = 1.0 / L;
      const double2 sp = cmul(g.s, p), dp = cmul(g.d2, pm);
      const double c1 = (2 * L - 1) * rl, c2 = (L - 1) * rl;
      pm = p;
      p = make_double2(c1 * sp.x - c2 * dp.x, c1 * sp.y - c2 * dp.y);
    }
    k[l] = cscale(nrm.n[L], cmul(pw[l], p));
  }
}

__device__ __forceinline__ bool finite2(float2 r) { return isfinite(r.x) && isfinite(r.y); }

__global__ __launch_bounds__(256) void pair_displace_kernel(const float2* __restrict__ x, const float2* __restrict__ r1,
                                                            const float2* __restrict__ r2, int B, int N, int P,
                                                            int pair0, size_t total, PairSlots slots,
                                                            float2* __restrict__ xp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;  // total = (pair1 - pair0) P B N
  const int e = (int)(idx % N);
  const size_t row = idx / N;  // ((q - pair0) P + p) B + b
  const size_t b = row % B;
  const size_t qp = row / B;
  const size_t smp = (qp % P) * B + b;
  const int q = pair0 + (int)(qp / P);
  xp[idx] = e == slots.i[q] ? r1[smp] : e == slots.j[q] ? r2[smp] : x[b * N + e];
}

__global__ __launch_bounds__(256) void pair_kernel_kernel(const float2* __restrict__ pts, int n, int flux,
                                                          PairNorms nrm, double2* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const float2* r = pts + 4 * (size_t)t;
  const bool ok = finite2(r[0]) && finite2(r[1]) && finite2(r[2]) && finite2(r[3]);
  const PairGeom g = pair_geom(r[0], r[1], r[2], r[3]);
  double2 p = make_double2(1.0, 0.0), pm = make_double2(0.0, 0.0);
  double2* o = out + (size_t)t * (flux + 1);
  for (int L0 = 0; L0 <= flux; L0 += kPairTile) {
    double2 k[kPairTile];
    pair_tile(g, flux, L0, nrm, p, pm, k);
#pragma unroll
    for (int l = 0; l < kPairTile; ++l)
      if (L0 + l <= flux) o[L0 + l] = ok ? k[l] : make_double2(quiet_nan(), quiet_nan());
  }
}

// ok[sample] and nvalid: all of a sample's log-amplitudes pass here
__global__ __launch_bounds__(256) void pair_valid_kernel(const float* __restrict__ logpsi,
                                                         const float* __restrict__ logpsi_p, int B, int npairs,
                                                         int samples, int32_t* __restrict__ ok,
                                                         int32_t* __restrict__ nvalid) {
  const int smp = blockIdx.x * 256 + threadIdx.x;
  if (smp >= samples) return;
  const float* lp = logpsi + 2 * (size_t)(smp % B);
  bool good = isfinite(lp[0]) && isfinite(lp[1]);
  for (int q = 0; q < npairs; ++q) {
    const float* lq = logpsi_p + 2 * ((size_t)q * samples + smp);
    good = good && isfinite(lq[0]) && isfinite(lq[1]) && isfinite(exp((double)lq[0] - (double)lp[0]));
  }
  ok[smp] = good ? 1 : 0;
  if (good) atomicAdd(nvalid, 1);
}

// grid (chunks, npairs); part[pair][chunk][flux + 1]
__global__ __launch_bounds__(kPairNT) void pair_terms_kernel(const float2* __restrict__ x,
                                                             const float2* __restrict__ r1,
                                                             const float2* __restrict__ r2,
                                                             const float* __restrict__ logpsi,
                                                             const float* __restrict__ logpsi_p,
                                                             const int32_t* __restrict__ ok, int B, int N, int flux,
                                                             int samples, PairNorms nrm, PairSlots slots,
                                                             double2* __restrict__ part) {
  const int q = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int smp = chunk * kPairNT + threadIdx.x;
  const bool live = smp < samples && ok[smp] != 0;
  PairGeom g = {};
  double2 w = make_double2(0.0, 0.0);
  if (live) {
    const size_t b = smp % B;
    g = pair_geom(x[b * N + slots.i[q]], x[b * N + slots.j[q]], r1[smp], r2[smp]);
    const float* lp = logpsi + 2 * b;
    const float* lq = logpsi_p + 2 * ((size_t)q * samples + smp);
    w = amp_ratio((double)lq[0] - (double)lp[0], (double)lq[1] - (double)lp[1]);
  }
  double2 p = make_double2(1.0, 0.0), pm = make_double2(0.0, 0.0);
  double2* out = part + ((size_t)q * chunks + chunk) * (flux + 1);
  for (int L0 = 0; L0 <= flux; L0 += kPairTile) {
    double2 k[kPairTile];
    pair_tile(g, flux, L0, nrm, p, pm, k);
    double acc[2 * kPairTile];
#pragma unroll
    for (int l = 0; l < kPairTile; ++l) {
      const double2 t = cmul(k[l], w);
      acc[2 * l] = live ? t.x : 0.0;  // a dead thread's geometry is all zeros: k is finite
      acc[2 * l + 1] = live ? t.y : 0.0;
    }
    int cnt = 0;
    block_sum<kPairNT, 2 * kPairTile>(acc, cnt);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int l = 0; l < kPairTile; ++l)
        if (L0 + l <= flux) out[L0 + l] = make_double2(acc[2 * l], acc[2 * l + 1]);
    }
    __syncthreads();  // block_sum's LDS is free for the next tile
  }
}

// grid 3 (flux + 1): A[c][L] = the partials of the pairs of class c, entry e = pair chunks + chunk
// by thread e % 256 in ascending e, then block_sum
__global__ __launch_bounds__(256) void pair_finish_kernel(const double2* __restrict__ part, int npairs, int chunks,
                                                          int flux, int n_up, PairSlots slots,
                                                          double2* __restrict__ A) {
  const int c = blockIdx.x / (flux + 1), L = blockIdx.x % (flux + 1);
  double acc[2] = {0.0, 0.0};
  const long long entries = (long long)npairs * chunks;
  for (long long e = threadIdx.x; e < entries; e += 256) {
    const int q = (int)(e / chunks);
    const int cls = slots.j[q] < n_up ? 0 : slots.i[q] < n_up ? 1 : 2;
    if (cls != c) continue;
    const double2 v = part[(size_t)e * (flux + 1) + L];
    acc[0] += v.x;
    acc[1] += v.y;
  }
  int cnt = 0;
  block_sum<256, 2>(acc, cnt);
  if (threadIdx.x == 0) A[blockIdx.x] = make_double2(acc[0], acc[1]);
}

PairNorms pair_norms(int flux) {
  PairNorms nrm{};
  auto log_binom = [](int n, int k) { return std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0); };
  for (int L = 0; L <= flux; ++L)
    nrm.n[L] = (flux + 1.0) * (flux + 1.0) * (2 * L + 1.0) / (flux + L + 1.0) *
               std::exp(log_binom(flux, L) - log_binom(flux + L, L));
  return nrm;
}

size_t pair_ok_bytes(int64_t samples) { return ((size_t)samples * sizeof(int32_t) + 63) / 64 * 64; }

}  // namespace

PairSlots pair_slots(int N) {
  PairSlots s{};
  int q = 0;
  for (int i = 0; i < N; ++i)
    for (int j = i + 1; j < N; ++j, ++q) {
      s.i[q] = (unsigned char)i;
      s.j[q] = (unsigned char)j;
    }
  return s;
}

size_t pair_workspace_bytes(int64_t samples, int N, int flux) {
  const size_t chunks = (size_t)((samples + kPairNT - 1) / kPairNT), npairs = (size_t)N * (N - 1) / 2;
  return pair_ok_bytes(samples) + npairs * chunks * (flux + 1) * sizeof(double2);
}

void launch_pair_displace(const float* x, const float* r1, const float* r2, int B, int N, int P, int pair0, int pair1,
                          float* xp, hipStream_t s) {
  const size_t total = (size_t)(pair1 - pair0) * P * B * N;
  hipLaunchKernelGGL(pair_displace_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(r1),
                     reinterpret_cast<const float2*>(r2), B, N, P, pair0, total, pair_slots(N),
                     reinterpret_cast<float2*>(xp));
}

void launch_pair_kernel(const float* points, int n, int flux, double* out, hipStream_t s) {
  hipLaunchKernelGGL(pair_kernel_kernel, dim3((n + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const float2*>(points), n, flux, pair_norms(flux),
                     reinterpret_cast<double2*>(out));
}

hipError_t launch_pair_accumulate(const float* x, const float* r1, const float* r2, const float* logpsi,
                                  const float* logpsi_p, int B, int N, int n_up, int flux, int P, double* A,
                                  int32_t* nvalid, void* workspace, hipStream_t s) {
  const int samples = P * B, npairs = N * (N - 1) / 2, chunks = (samples + kPairNT - 1) / kPairNT;
  int32_t* ok = static_cast<int32_t*>(workspace);
  double2* part = reinterpret_cast<double2*>(static_cast<char*>(workspace) + pair_ok_bytes(samples));
  const hipError_t e = hipMemsetAsync(nvalid, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  const PairSlots slots = pair_slots(N);
  hipLaunchKernelGGL(pair_valid_kernel, dim3((samples + 255) / 256), dim3(256), 0, s, logpsi, logpsi_p, B, npairs,
                     samples, ok, nvalid);
  if (npairs > 0)  // N = 1 has no pair: the finish kernel then writes zeros
    hipLaunchKernelGGL(pair_terms_kernel, dim3(chunks, npairs), dim3(kPairNT), 0, s,
                       reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(r1),
                       reinterpret_cast<const float2*>(r2), logpsi, logpsi_p, ok, B, N, flux, samples,
                       pair_norms(flux), slots, part);
  hipLaunchKernelGGL(pair_finish_kernel, dim3(3 * (flux + 1)), dim3(256), 0, s, part, npairs, chunks, flux, n_up,
                     slots, reinterpret_cast<double2*>(A));
  return hipSuccess;
}

}  // namespace dh
