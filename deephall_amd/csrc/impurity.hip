// One-body impurity potential and the density around an axis (hamiltonian.py external term,
// netobs/observables/axis_density.py; not in the reference).  Walkers x[B][N][2] float32
// (theta, phi), the slots below n_up up and the rest down; every unit vector is formed once, in
// double, from the upcast angles, as hamiltonian_tail forms its pair geometry.
//
//   external_kernel   U(b) = sum_a sum_{i in species(a)} U_a(r_i) with u = r_i . r_a, the squared
//                     chord over 2 R^2 t = max(1 - u, 0), and
//                       gaussian  U_a = s exp(-(R^2 / w^2) t)        (= s exp(-c^2 / (2 w^2)))
//                       charge    U_a = s / sqrt(2 R^2 t + h^2)      (= s / sqrt(c^2 + h^2)).
//                     One wave per walker: lane i owns electron i and adds its impurities in
//                     table order, then the lanes are added by xor shuffles (32, 16, ..., 1; the
//                     lanes past N hold 0).  Nothing in that order depends on B or on the
//                     walker's place in the batch, and no float atomic is used, so a walker's
//                     value is the same bits alone and in any batch.  The table (unit vectors
//                     and the two coefficients of each impurity, computed on the host in double)
//                     is a kernel argument.  A walker with a non-finite coordinate is NaN.
//   axis_hist_kernel  u = r_i . a for every electron, binned by equal area: t = (1 - u) bins / 2,
//                     bin floor(t) clamped to 0 .. bins - 1 (so bin k is (1 - 2(k+1)/bins,
//                     1 - 2k/bins] and the last one is closed at u = -1), NaN dropped.  Integer
//                     counts in LDS per workgroup, then one integer vector atomic per non-empty
//                     bin: integer sums do not depend on the order.
#include <cmath>

#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

__device__ __forceinline__ double3 unit_vector(const float* __restrict__ xe) {
  double st, ct, sp, cp;
  sincos((double)xe[0], &st, &ct);
  sincos((double)xe[1], &sp, &cp);
  return make_double3(st * cp, st * sp, ct);
}

__device__ __forceinline__ double dot3(double3 r, double ax, double ay, double az) {
  return fma(r.x, ax, fma(r.y, ay, r.z * az));
}

// 256 threads: wave w of workgroup g is walker 4 g + w
__global__ __launch_bounds__(256) void external_kernel(const float* __restrict__ x, int B, int N, int n_up,
                                                       ImpurityTable tab, float* __restrict__ e_l,
                                                       float* __restrict__ ext) {
  const int lane = threadIdx.x & 63;
  const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= (size_t)B) return;  // a whole wave: no shuffle below is divergent
  const float* xb = x + b * 2 * N;
  double sum = 0.0;
  bool bad = false;
  if (lane < N) {
    bad = !isfinite(xb[2 * lane]) || !isfinite(xb[2 * lane + 1]);
    const double3 r = unit_vector(xb + 2 * lane);
    const int mine = lane < n_up ? kImpurityUp : kImpurityDown;
    for (int a = 0; a < tab.n; ++a) {
      if (tab.species[a] != kImpurityBoth && tab.species[a] != mine) continue;
      const double t = fmax(1.0 - dot3(r, tab.ax[a], tab.ay[a], tab.az[a]), 0.0);
      // p: R^2 / w^2 (gaussian), 2 R^2 (charge); q: unused (gaussian), h^2 (charge)
      const double u = tab.kind[a] == kImpurityGaussian ? exp(-(tab.p[a] * t)) : 1.0 / sqrt(fma(tab.p[a], t, tab.q[a]));
      sum += tab.strength[a] * u;
    }
  }
  sum = wave_sum(sum);
  if (__any(bad)) sum = quiet_nan();
  if (lane == 0) {
    ext[b] = (float)sum;
    if (e_l) e_l[2 * b] = (float)((double)e_l[2 * b] + sum);
  }
}

// thread t takes the electrons t, t + stride, ... of the flat list [B N]; LDS: unsigned [2][bins]
__global__ __launch_bounds__(256) void axis_hist_kernel(const float* __restrict__ x, int total, int N, int n_up,
                                                        double ax, double ay, double az, int bins,
                                                        unsigned* __restrict__ counts) {
  extern __shared__ unsigned ah[];
  for (int k = threadIdx.x; k < 2 * bins; k += 256) ah[k] = 0u;
  __syncthreads();
  const double scale = 0.5 * (double)bins;
  const int stride = gridDim.x * 256;
  // e + stride may pass 2^31 - 1: the loop variable is 64-bit, the index below it is not
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < (long long)total; e += stride) {
    const double u = dot3(unit_vector(x + 2 * e), ax, ay, az);
    if (u != u) continue;  // NaN (a non-finite angle) is dropped
    const double t = (1.0 - u) * scale;
    const int k = t <= 0.0 ? 0 : t >= (double)bins ? bins - 1 : (int)t;
    const int row = (int)(e % N) < n_up ? 0 : 1;
    atomicAdd(ah + row * bins + k, 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * bins; k += 256)
    if (ah[k] != 0u) atomicAdd(counts + k, ah[k]);
}

}  // namespace

void impurity_vector(double theta, double phi, double* v) {
  v[0] = std::sin(theta) * std::cos(phi);
  v[1] = std::sin(theta) * std::sin(phi);
  v[2] = std::cos(theta);
}

void launch_external_potential(const float* x, int B, int N, int n_up, const ImpurityTable& tab, float* e_l,
                               float* ext, hipStream_t s) {
  hipLaunchKernelGGL(external_kernel, dim3((B - 1) / 4 + 1), dim3(256), 0, s, x, B, N, n_up, tab, e_l, ext);
}

void launch_axis_histogram(const float* x, int B, int N, int n_up, double axis_theta, double axis_phi, int bins,
                           unsigned* counts, hipStream_t s) {
  double a[3];
  impurity_vector(axis_theta, axis_phi, a);
  const int total = B * N;  // < 2^31: the caller's check
  const int grid = std::min((total - 1) / 256 + 1, 2048);
  hipLaunchKernelGGL(axis_hist_kernel, dim3(grid), dim3(256), (size_t)2 * bins * sizeof(unsigned), s, x, total, N,
                     n_up, a[0], a[1], a[2], bins, counts);
}

}  // namespace dh
