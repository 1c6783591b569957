// Landau-level-resolved one-body density matrix (netobs/observables/ll_rdm.py; not in the
// reference, whose one_rdm.py only ever evaluates make_monopole_harm at l = Q).
//
// Basis: the monopole harmonics Y_{Q,l,m}, Q = flux / 2, l = Q + n for the levels n = 0..L-1,
// m = -l..l; level-major, m ascending inside a level, norb = L (flux + 1) + L (L - 1).  With
// t = Q + m (an integer, -n..flux + n), x = clip(cos theta, +-(1 - 1e-4)), u = 1 - x, v = 1 + x,
// only the s with non-zero binomials of one_rdm.py:36-51 survive, s = smin..smax,
// smin = max(0, -t), smax = min(n, flux + n - t), and the powers of the s = smax / s = smin
// terms factor out:
//     Y = u^(|flux - t| / 2) v^(|t| / 2) e^{i m phi} sum_j c_j u^(d - j) v^j,  d = smax - smin <= n,
//     c_j = norm 2^-l (-1)^(k - s) C(n, s) C(flux + n, k - s),  s = smin + j,  k = l - m = flux + n - t,
//     norm^2 = (2l + 1) / (4 pi)  k! (2l - k)! / (n! (flux + n)!).
// The power factor and the phase depend on m alone, not on the level: a point evaluates them
// once per m and reuses them for the <= L orbitals of that m.  The c_j (kRdmCoef per orbital,
// zero-padded) are computed on the host in double, once per (device, flux, levels), and kept in a
// device table for the life of the process (a few KB each).  All device math is double.
//
//   harmonics   one thread per (point, m): out[n][norb] complex float32, dh_monopole_orbitals'
//               format.
//   displace    one thread per float2 of xp[P][B][N][N]: row (p B + b) N + a is walker b with
//               electron a at r_prime[p][b]; coordinates are copied.
//   accumulate  pass 1, one workgroup per kRdmSmp samples (sample = p B + b): the N + 1 points'
//               (u, v, log u / 2, log v / 2, phi) and the N ratios exp(logpsi_p - logpsi) go to
//               LDS, then one thread per (sample, m) writes U[s][sample][i] = sum over the
//               electrons a of spin s of ratio_a Y_i(r_a) and V[sample][j] = Y_j(r') as double
//               complex.  A sample with a non-finite log-amplitude or ratio writes zeros and is
//               not counted in nvalid (an integer atomic: its value does not depend on the order).
//               pass 2, rho[s] = 4 pi U[s]^T conj(V): 32 x 32 tiles of rho, the samples split in
//               rdm_nsplit contiguous chunks, 2 x 2 complex outputs per thread from LDS stages of
//               16 samples, plain double FMAs; each (split, tile) writes its partial sums, and a
//               last kernel adds the splits in order.  No float atomics: two calls give identical
//               bits.  Every load is guarded by sample < samples and orbital < norb.
// [samples][norb][norb] is never formed: the workspace is U, V and the split partials.
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kRdmCoef = kRdmMaxLevels;  // coefficients per orbital: d + 1 <= levels
constexpr int kRdmSmp = 4;               // samples per pass-1 workgroup
constexpr int kRdmMaxN = 32;
constexpr int kTile = 32;                // pass 2: rho tile edge
constexpr int kStage = 16;               // pass 2: samples per LDS stage
constexpr int kMaxSplit = 16;

__host__ __device__ inline int level_offset(int flux, int n) { return n * (flux + 1) + n * (n - 1); }

// a point's level-independent part: u, v, log(u) / 2, log(v) / 2, phi
struct RdmPoint {
  double u, v, hlu, hlv, phi;
};

__device__ __forceinline__ RdmPoint rdm_point(float theta, float phi) {
  const double x = fmin(fmax(cos((double)theta), -1.0 + 1e-4), 1.0 - 1e-4);
  return {1.0 - x, 1.0 + x, 0.5 * log1p(-x), 0.5 * log1p(x), (double)phi};
}

// the orbitals of t = Q + m at one point, levels nmin..levels-1: y[n] (re, im)
__device__ __forceinline__ void rdm_harmonics_of_m(const RdmPoint& pt, int flux, int levels, int t, int nmin,
                                                   const double* __restrict__ coef, double (*y)[2]) {
  const double w = exp(abs(flux - t) * pt.hlu + abs(t) * pt.hlv);
  double s, c;
  sincos((t - 0.5 * flux) * pt.phi, &s, &c);
  const int smin = max(0, -t);
#pragma unroll  // constant indices keep y in registers
  for (int n = 0; n < kRdmMaxLevels; ++n) {
    if (n < nmin || n >= levels) continue;
    const int d = min(n, flux + n - t) - smin;
    const double* cj = coef + (size_t)(level_offset(flux, n) + t + n) * kRdmCoef;
    double acc = cj[0], vp = 1.0;
    for (int j = 1; j <= d; ++j) {
      vp *= pt.v;
      acc = acc * pt.u + cj[j] * vp;
    }
    y[n][0] = w * acc * c;
    y[n][1] = w * acc * s;
  }
}

// levels n >= nmin hold t: -n <= t <= flux + n
__device__ __forceinline__ int rdm_nmin(int flux, int t) { return max(0, max(-t, t - flux)); }

__global__ __launch_bounds__(256) void rdm_harmonics_kernel(const float* __restrict__ pts, int npts, int flux,
                                                            int levels, const double* __restrict__ coef,
                                                            float* __restrict__ out) {
  const int mt = flux + 2 * levels - 1;  // values of t
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)npts * mt) return;
  const size_t p = idx / mt;
  const int t = (int)(idx - p * mt) - (levels - 1);
  const int norb = level_offset(flux, levels), nmin = rdm_nmin(flux, t);
  const RdmPoint pt = rdm_point(pts[2 * p], pts[2 * p + 1]);
  double y[kRdmMaxLevels][2];
  rdm_harmonics_of_m(pt, flux, levels, t, nmin, coef, y);
  float2* o = reinterpret_cast<float2*>(out) + p * norb;
#pragma unroll
  for (int n = 0; n < kRdmMaxLevels; ++n)
    if (n >= nmin && n < levels) o[level_offset(flux, n) + t + n] = make_float2((float)y[n][0], (float)y[n][1]);
}

__global__ __launch_bounds__(256) void rdm_displace_kernel(const float2* __restrict__ x,
                                                           const float2* __restrict__ r_prime, int B, int N,
                                                           size_t total, float2* __restrict__ xp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;  // total = P B N N
  const int e = (int)(idx % N);
  const size_t row = idx / N;  // (p B + b) N + a
  const int a = (int)(row % N);
  const size_t smp = row / N;  // p B + b
  const size_t b = smp % B;
  xp[idx] = e == a ? r_prime[smp] : x[b * N + e];
}

__global__ __launch_bounds__(256) void rdm_uv_kernel(const float* __restrict__ x, const float* __restrict__ r_prime,
                                                     const float* __restrict__ logpsi,
                                                     const float* __restrict__ logpsi_p, int B, int N, int n_up,
                                                     int flux, int levels, int samples, int by_spin,
                                                     const double* __restrict__ coef, double2* __restrict__ U,
                                                     double2* __restrict__ V, int32_t* __restrict__ nvalid) {
  __shared__ RdmPoint pts[kRdmSmp][kRdmMaxN + 1];
  __shared__ double ratio[kRdmSmp][kRdmMaxN][2];
  __shared__ int ok[kRdmSmp];
  const int tid = threadIdx.x;
  const int smp0 = blockIdx.x * kRdmSmp;
  if (tid < kRdmSmp) ok[tid] = 1;
  __syncthreads();
  for (int w = tid; w < kRdmSmp * (N + 1); w += 256) {
    const int sl = w / (N + 1), a = w - sl * (N + 1);
    const int smp = smp0 + sl;
    if (smp >= samples) continue;
    const int b = smp % B;
    if (a == N) {
      pts[sl][N] = rdm_point(r_prime[2 * (size_t)smp], r_prime[2 * (size_t)smp + 1]);
      continue;
    }
    const float* xa = x + ((size_t)b * N + a) * 2;
    pts[sl][a] = rdm_point(xa[0], xa[1]);
    const float* lp = logpsi + 2 * (size_t)b;
    const float* lq = logpsi_p + ((size_t)smp * N + a) * 2;
    const double dr = (double)lq[0] - (double)lp[0], di = (double)lq[1] - (double)lp[1];
    const double2 r = amp_ratio(dr, di);
    ratio[sl][a][0] = r.x;
    ratio[sl][a][1] = r.y;
    // all of this sample's log-amplitudes pass here: log psi by every a, log psi(R_a') by its own
    if (!(isfinite(lp[0]) && isfinite(lp[1]) && isfinite(lq[0]) && isfinite(lq[1]) && isfinite(exp(dr)))) ok[sl] = 0;
  }
  __syncthreads();
  if (tid < kRdmSmp && smp0 + tid < samples && ok[tid]) atomicAdd(nvalid, 1);
  const int mt = flux + 2 * levels - 1, norb = level_offset(flux, levels);
  for (int w = tid; w < kRdmSmp * mt; w += 256) {
    const int sl = w / mt, t = w - sl * mt - (levels - 1);
    const int smp = smp0 + sl;
    if (smp >= samples) continue;
    const int nmin = rdm_nmin(flux, t);
    double u[2][kRdmMaxLevels][2] = {};
    double v[kRdmMaxLevels][2] = {};
    if (ok[sl]) {
      double y[kRdmMaxLevels][2];
      for (int a = 0; a < N; ++a) {
        rdm_harmonics_of_m(pts[sl][a], flux, levels, t, nmin, coef, y);
        const double rr = ratio[sl][a][0], ri = ratio[sl][a][1];
        const bool down = by_spin && a >= n_up;
#pragma unroll
        for (int n = 0; n < kRdmMaxLevels; ++n) {
          if (n < nmin || n >= levels) continue;
          const double re = rr * y[n][0] - ri * y[n][1], im = rr * y[n][1] + ri * y[n][0];
          u[0][n][0] += down ? 0.0 : re;
          u[0][n][1] += down ? 0.0 : im;
          u[1][n][0] += down ? re : 0.0;
          u[1][n][1] += down ? im : 0.0;
        }
      }
      rdm_harmonics_of_m(pts[sl][N], flux, levels, t, nmin, coef, v);
    }
#pragma unroll
    for (int n = 0; n < kRdmMaxLevels; ++n) {
      if (n < nmin || n >= levels) continue;
      const size_t at = (size_t)smp * norb + level_offset(flux, n) + t + n;
      V[at] = make_double2(v[n][0], v[n][1]);
      U[at] = make_double2(u[0][n][0], u[0][n][1]);
      if (by_spin) U[(size_t)samples * norb + at] = make_double2(u[1][n][0], u[1][n][1]);
    }
  }
}

// grid (tiles x tiles, nsplit, S); part[split][s][norb][norb]
__global__ __launch_bounds__(256) void rdm_product_kernel(const double2* __restrict__ U, const double2* __restrict__ V,
                                                          int samples, int norb, int chunk, int tiles,
                                                          double2* __restrict__ part) {
  __shared__ double2 su[kStage][kTile];
  __shared__ double2 sv[kStage][kTile];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = (blockIdx.x / tiles) * kTile, j0 = (blockIdx.x % tiles) * kTile;
  const int split = blockIdx.y, s = blockIdx.z, S = gridDim.z;
  const int k0 = (int)min((long long)split * chunk, (long long)samples);
  const int k1 = (int)min((long long)k0 + chunk, (long long)samples);
  const double2* Us = U + (size_t)s * samples * norb;
  double acc[2][2][2] = {};
  for (int kk = k0; kk < k1; kk += kStage) {
    for (int e = tid; e < kStage * kTile; e += 256) {
      const int kr = e / kTile, c = e - kr * kTile;
      const int smp = kk + kr;
      const bool in = smp < k1;
      su[kr][c] = in && i0 + c < norb ? Us[(size_t)smp * norb + i0 + c] : make_double2(0.0, 0.0);
      sv[kr][c] = in && j0 + c < norb ? V[(size_t)smp * norb + j0 + c] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int kr = 0; kr < kStage; ++kr) {
      const double2 a[2] = {su[kr][ty], su[kr][ty + 16]};
      const double2 b[2] = {sv[kr][tx], sv[kr][tx + 16]};
      for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q) {  // a conj(b)
          acc[p][q][0] += a[p].x * b[q].x + a[p].y * b[q].y;
          acc[p][q][1] += a[p].y * b[q].x - a[p].x * b[q].y;
        }
    }
    __syncthreads();
  }
  double2* out = part + ((size_t)split * S + s) * norb * norb;
  for (int p = 0; p < 2; ++p)
    for (int q = 0; q < 2; ++q) {
      const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
      if (i < norb && j < norb) out[(size_t)i * norb + j] = make_double2(acc[p][q][0], acc[p][q][1]);
    }
}

// rho[idx] = 4 pi x the splits' partials added in order; n = S norb norb
__global__ __launch_bounds__(256) void rdm_finish_kernel(const double2* __restrict__ part, int nsplit, size_t n,
                                                         double2* __restrict__ rho) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  double re = 0.0, im = 0.0;
  for (int k = 0; k < nsplit; ++k) {
    const double2 v = part[(size_t)k * n + idx];
    re += v.x;
    im += v.y;
  }
  rho[idx] = make_double2(kFourPi * re, kFourPi * im);
}

double log_binom(int n, int k) { return std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0); }

}  // namespace

int rdm_norb(int flux, int levels) { return level_offset(flux, levels); }

static std::vector<double> rdm_coefficients(int flux, int levels) {
  std::vector<double> c((size_t)rdm_norb(flux, levels) * kRdmCoef, 0.0);
  for (int n = 0; n < levels; ++n)
    for (int t = -n; t <= flux + n; ++t) {
      const int k = flux + n - t, two_l = flux + 2 * n;  // k = l - m
      const double lognorm = 0.5 * (std::log((two_l + 1.0) / kFourPi) + std::lgamma(k + 1.0) +
                                    std::lgamma(two_l - k + 1.0) - std::lgamma(n + 1.0) -
                                    std::lgamma(flux + n + 1.0)) -
                             0.5 * two_l * M_LN2;
      const int smin = std::max(0, -t), smax = std::min(n, k);
      double* cj = c.data() + (size_t)(level_offset(flux, n) + t + n) * kRdmCoef;
      for (int s = smin; s <= smax; ++s) {
        const double mag = std::exp(lognorm + log_binom(n, s) + log_binom(flux + n, k - s));
        cj[s - smin] = ((k - s) & 1) ? -mag : mag;
      }
    }
  return c;
}

// the device copy of rdm_coefficients, made at the first use on each device and kept
hipError_t rdm_table(int flux, int levels, const double** table) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int>, double*> cache;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find({dev, flux, levels});
  if (it == cache.end()) {
    const std::vector<double> c = rdm_coefficients(flux, levels);
    double* d = nullptr;
    if ((e = hipMalloc(&d, c.size() * sizeof(double))) != hipSuccess) return e;
    if ((e = hipMemcpy(d, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) {
      (void)hipFree(d);
      return e;
    }
    it = cache.emplace(std::make_tuple(dev, flux, levels), d).first;
  }
  *table = it->second;
  return hipSuccess;
}

int rdm_nsplit(int64_t samples, int flux, int levels) {
  const int64_t tiles1 = (rdm_norb(flux, levels) + kTile - 1) / kTile;
  const int64_t want = (512 + 2 * tiles1 * tiles1 - 1) / (2 * tiles1 * tiles1);  // about 512 workgroups
  const int64_t most = (samples + 4 * kStage - 1) / (4 * kStage);                // at least 4 stages each
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, most, kMaxSplit}));
}

size_t rdm_workspace_bytes(int64_t samples, int flux, int levels) {
  const size_t norb = rdm_norb(flux, levels);
  const size_t uv = 3 * (size_t)samples * norb;  // U up, U down, V
  const size_t part = (size_t)rdm_nsplit(samples, flux, levels) * 2 * norb * norb;
  return (uv + part) * sizeof(double2);
}

void launch_monopole_harmonics(const float* pts, int n, int flux, int levels, const double* table, float* out,
                               hipStream_t s) {
  const size_t total = (size_t)n * (flux + 2 * levels - 1);
  hipLaunchKernelGGL(rdm_harmonics_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pts, n, flux,
                     levels, table, out);
}

void launch_rdm_displace(const float* x, const float* r_prime, int B, int N, int P, float* xp, hipStream_t s) {
  const size_t total = (size_t)P * B * N * N;
  hipLaunchKernelGGL(rdm_displace_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(r_prime), B, N, total,
                     reinterpret_cast<float2*>(xp));
}

hipError_t launch_rdm_accumulate(const float* x, const float* r_prime, const float* logpsi, const float* logpsi_p,
                                 int B, int N, int n_up, int flux, int levels, int P, int by_spin,
                                 const double* table, double* rho, int32_t* nvalid, void* workspace, hipStream_t s) {
  const int samples = P * B, norb = rdm_norb(flux, levels), S = by_spin ? 2 : 1;
  const int nsplit = rdm_nsplit(samples, flux, levels), tiles = (norb + kTile - 1) / kTile;
  double2* U = static_cast<double2*>(workspace);
  double2* V = U + 2 * (size_t)samples * norb;
  double2* part = V + (size_t)samples * norb;
  const hipError_t e = hipMemsetAsync(nvalid, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rdm_uv_kernel, dim3((samples + kRdmSmp - 1) / kRdmSmp), dim3(256), 0, s, x, r_prime, logpsi,
                     logpsi_p, B, N, n_up, flux, levels, samples, by_spin, table, U, V, nvalid);
  // contiguous chunks of whole stages
  const int chunk = ((samples + nsplit - 1) / nsplit + kStage - 1) / kStage * kStage;
  hipLaunchKernelGGL(rdm_product_kernel, dim3(tiles * tiles, nsplit, S), dim3(256), 0, s, U, V, samples, norb, chunk,
                     tiles, part);
  const size_t n = (size_t)S * norb * norb;
  hipLaunchKernelGGL(rdm_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, nsplit, n,
                     reinterpret_cast<double2*>(rho));
  return hipSuccess;
}

}  // namespace dh
