// Device code shared by the estimator kernels (spin.hip, holes.hip, swap.hip, rdm.hip, fidelity.hip,
// sfactor.hip, subspace.hip).  Their convention, stated once: from the subtraction of two log psi on everything is
// double; every sum over walkers runs in a fixed order with no float atomics, so two calls give
// identical bits; an invalid walker (a non-finite log or ratio) is NaN in the per-walker array and
// skipped in the sums.  Nothing here adds a product to anything: each includer may contract a
// product feeding an add differently (sfactor.hip is built with contraction off), so the arithmetic
// around these calls stays in the kernel that owns it.
#pragma once
#include "device_common.h"

namespace dh {

constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kFourPi = 12.566370614359172953850573533118;

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// e^{dr + i di}, the phase folded into [-pi, pi] first
__device__ __forceinline__ double2 amp_ratio(double dr, double di) {
  const double m = exp(dr);
  double s, c;
  sincos(remainder(di, kTwoPi), &s, &c);
  return make_double2(m * c, m * s);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The ordered sum of a workgroup of NT threads: acc[NA] and cnt hold each thread's own sums on
// entry and the workgroup's in thread 0 on return.  A wave by xor shuffles (32, 16, ..., 1), lane 0
// of each wave to LDS, one barrier, then thread 0 adds the waves in ascending index.  (swap.hip and
// fidelity.hip carry no count and end with thread q adding component q: the same bits by another
// instruction sequence, which they keep.)
template <int NT, int NA>
__device__ __forceinline__ void block_sum(double (&acc)[NA], int& cnt) {
  constexpr int NW = NT / 64;
  __shared__ double wsum[NW][NA];
  __shared__ int wcnt[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    for (int q = 0; q < NA; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
    cnt += __shfl_xor(cnt, off, 64);
  }
  if (lane == 0) {
    for (int q = 0; q < NA; ++q) wsum[w][q] = acc[q];
    wcnt[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < NA; ++q) acc[q] = 0.0;
    cnt = 0;
    for (int j = 0; j < NW; ++j) {
      for (int q = 0; q < NA; ++q) acc[q] += wsum[j][q];
      cnt += wcnt[j];
    }
  }
}

}  // namespace dh
