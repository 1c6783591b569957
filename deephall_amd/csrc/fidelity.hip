// Fidelity of the network with a trial state on the network's own walkers (pretrain.py;
// not in the reference).  With d_b = log phi(x_b) - log psi(x_b), x_b ~ |psi|^2:
//
//   F = |<phi|psi>|^2 / (<phi|phi> <psi|psi>) = |mean_b e^{d_b}|^2 / mean_b |e^{d_b}|^2
//
//   fidelity_partial_kernel (dh_fidelity_partial): the shifted sums of one batch (or one rank's
//     shard): m = max Re d over the valid walkers, S = sum z_b with z_b = e^{d_b - m} (complex),
//     S2 = sum |z_b|^2 = sum e^{2 (Re d_b - m)}, n = the number of valid walkers.  Trial states
//     carry no normalisation, Re d reaches hundreds: nothing is exponentiated before the shift.
//   fidelity_residual_kernel (dh_fidelity_residual): eps_b = 1 - n z_b / S from the combined
//     sums, the weight of conj(d log psi) in the gradient of -log F.
//
// Arithmetic: the estimators' convention (estimator_common.h), z_b by amp_ratio.  |z_b|^2 is taken
// from the rounded parts of the z_b that enters S, and the residual's quotient from products
// rounded one by one (no fused multiply-add), so a single walker gives F = 1 and eps = 0 exactly.
// One 1024-thread workgroup reduces a batch: each thread its strided walkers in order, a wave by
// wave_sum, then thread q adds component q of the 16 waves in order.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kNT = 1024;
constexpr int kNW = kNT / 64;

// d = log phi - log psi of walker i; false when any of the four floats is not finite
__device__ __forceinline__ bool fid_d(const float* __restrict__ lpsi, const float* __restrict__ lphi, int i,
                                      double& dr, double& di) {
  const float ar = lpsi[2 * (size_t)i], ai = lpsi[2 * (size_t)i + 1];
  const float br = lphi[2 * (size_t)i], bi = lphi[2 * (size_t)i + 1];
  dr = (double)br - (double)ar;
  di = (double)bi - (double)ai;
  return isfinite(ar) && isfinite(ai) && isfinite(br) && isfinite(bi);
}

// z = e^{dr - m} (cos di, sin di)
__device__ __forceinline__ void fid_term(double dr, double di, double m, double& zr, double& zi) {
  const double2 z = amp_ratio(dr - m, di);
  zr = z.x;
  zi = z.y;
}

// a b + c d with each product and the sum rounded on its own (the compiler's default would
// contract one product into a fused multiply-add)
__device__ __forceinline__ double dot2(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double q = c * d;
  return p + q;
}

__global__ __launch_bounds__(kNT) void fidelity_partial_kernel(const float* __restrict__ lpsi,
                                                               const float* __restrict__ lphi, int B,
                                                               double* __restrict__ part) {
  __shared__ double wmax[kNW];
  __shared__ double wsum[kNW][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double mx = -INFINITY;
  for (int i = tid; i < B; i += kNT) {
    double dr, di;
    if (fid_d(lpsi, lphi, i, dr, di)) mx = fmax(mx, dr);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wmax[w] = mx;
  __syncthreads();
  double m = wmax[0];
  for (int j = 1; j < kNW; ++j) m = fmax(m, wmax[j]);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // S re, S im, S2, n
  if (m > -INFINITY) {  // block-uniform: at least one valid walker, and m is finite
    for (int i = tid; i < B; i += kNT) {
      double dr, di;
      if (!fid_d(lpsi, lphi, i, dr, di)) continue;
      double zr, zi;
      fid_term(dr, di, m, zr, zi);
      acc[0] += zr;
      acc[1] += zi;
      acc[2] += dot2(zr, zr, zi, zi);
      acc[3] += 1.0;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) wsum[w][q] = v;
  }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int j = 0; j < kNW; ++j) t += wsum[j][tid];
    part[1 + tid] = t;
  }
  if (tid == 0) part[0] = m;
}

__global__ __launch_bounds__(256) void fidelity_residual_kernel(const float* __restrict__ lpsi,
                                                                const float* __restrict__ lphi, int B,
                                                                const double* __restrict__ total,
                                                                float* __restrict__ resid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const double m = total[0], sr = total[1], si = total[2], n = total[4];
  const double den = dot2(sr, sr, si, si);  // |S|^2 <= n^2: no overflow
  double dr, di;
  const bool ok = fid_d(lpsi, lphi, i, dr, di);
  float er = NAN, ei = NAN;
  if (ok && n > 0.0 && den > 0.0) {
    double zr, zi;
    fid_term(dr, di, m, zr, zi);
    // q = z / S = z conj(S) / |S|^2
    const double qr = dot2(zr, sr, zi, si) / den;
    const double qi = dot2(zi, sr, -zr, si) / den;
    er = (float)(1.0 - n * qr);
    ei = (float)(-(n * qi));
  }
  resid[2 * (size_t)i] = er;
  resid[2 * (size_t)i + 1] = ei;
}

}  // namespace

void launch_fidelity_partial(const float* logpsi, const float* logphi, int B, double* part, hipStream_t s) {
  hipLaunchKernelGGL(fidelity_partial_kernel, dim3(1), dim3(kNT), 0, s, logpsi, logphi, B, part);
}

void launch_fidelity_residual(const float* logpsi, const float* logphi, int B, const double* total, float* resid,
                              hipStream_t s) {
  hipLaunchKernelGGL(fidelity_residual_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logpsi, logphi, B, total,
                     resid);
}

}  // namespace dh
