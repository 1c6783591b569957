// Device code shared by fidelity.hip (one trial state, pretraining) and orthogonal.hip (K frozen
// states, the overlap penalty): d = log phi - log psi of a walker, z = e^{d - m}, the products that
// are rounded one by one, the shifted sums of one workgroup and the residual's quotient.  Both files
// call the same functions, so row k of dh_ortho_partial and dh_fidelity_partial on state k are the
// same instruction sequence on the same numbers.
#pragma once
#include "estimator_common.h"

namespace dh {

constexpr int kFidNT = 1024;
constexpr int kFidNW = kFidNT / 64;

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

// The shifted sums (m, S re, S im, S2, n) of B walkers into part[DH_NFID], by one workgroup of
// kFidNT threads: each thread its strided walkers in order, a wave by wave_sum, then thread q adds
// component q of the 16 waves in order.
__device__ __forceinline__ void fid_partial_block(const float* __restrict__ lpsi, const float* __restrict__ lphi,
                                                  int B, double* __restrict__ part) {
  __shared__ double wmax[kFidNW];
  __shared__ double wsum[kFidNW][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double mx = -INFINITY;
  for (int i = tid; i < B; i += kFidNT) {
    double dr, di;
    if (fid_d(lpsi, lphi, i, dr, di)) mx = fmax(mx, dr);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wmax[w] = mx;
  __syncthreads();
  double m = wmax[0];
  for (int j = 1; j < kFidNW; ++j) m = fmax(m, wmax[j]);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // S re, S im, S2, n
  if (m > -INFINITY) {  // block-uniform: at least one valid walker, and m is finite
    for (int i = tid; i < B; i += kFidNT) {
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
    for (int j = 0; j < kFidNW; ++j) t += wsum[j][tid];
    part[1 + tid] = t;
  }
  if (tid == 0) part[0] = m;
}

// eps = 1 - n z / S of a valid walker from the sums total[DH_NFID] (n > 0, den = |S|^2 > 0):
// q = z / S = z conj(S) / |S|^2 from products rounded one by one
__device__ __forceinline__ void fid_eps(double dr, double di, double m, double sr, double si, double den, double n,
                                        double& er, double& ei) {
  double zr, zi;
  fid_term(dr, di, m, zr, zi);
  const double qr = dot2(zr, sr, zi, si) / den;
  const double qi = dot2(zi, sr, -zr, si) / den;
  er = 1.0 - n * qr;
  ei = -(n * qi);
}

}  // namespace dh
