// Total-spin estimator (netobs/observables/spin_square.py; not in the reference).  With the slots
// below n_up up and the rest down, and R_{i<->j} the walker R with the coordinates of an up slot i
// and a down slot j exchanged,
//
//   S^2_loc(R) = ((n_up - n_dn) / 2)^2 + N / 2 - sum_{i up, j down} psi(R_{i<->j}) / psi(R),
//
// which is S (S + 1) on every walker of a total-spin eigenstate.  Pair p = i n_dn + (j - n_up),
// P = n_up n_dn pairs; a caller may send them through the wavefunction in windows [pair0, pair1).
//
//   exchange  one thread per float2 of xs[(pair1 - pair0) B][N]: row (p - pair0) B + b is walker b
//             with slots i and j of pair p exchanged.  Coordinates are copied, never recomputed.
//   ratios    one thread per (p, b) of a window: amp_ratio of log psi(R_p) - log psi(R) into
//             ratio[p][b], the workspace; a non-finite log or ratio is stored as NaN.
//             Elementwise: what a pair stores does not depend on the window it arrived in.
//   walker    after every pair has been stored, one thread per walker: the walker is valid when
//             its own log and its P ratios are finite; s2[b] = S^2_loc with the pairs added in
//             ascending p, NaN for an invalid walker; valid[b] to the workspace.
//   sums      one workgroup per pair, and one more for the total: the sum over the valid walkers
//             of ratio[p][b] (of s2[b], with nvalid as an integer count) by block_sum.
// The estimators' convention (estimator_common.h): two calls give identical bits, and so do one
// window of all pairs and one window per pair.  P = 0 (one species empty) launches neither
// exchange nor ratios, and S^2_loc = (N / 2)(N / 2 + 1) exactly.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kSumNT = 256;

__global__ __launch_bounds__(256) void spin_exchange_kernel(const float2* __restrict__ x, int B, int N, int n_up,
                                                            int n_dn, int pair0, size_t total,
                                                            float2* __restrict__ xs) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;  // total = (pair1 - pair0) B N
  const int e = (int)(idx % N);
  const size_t row = idx / N;  // (p - pair0) B + b
  const size_t b = row % B;
  const int p = pair0 + (int)(row / B);
  const int i = p / n_dn, j = n_up + p % n_dn;
  const int src = e == i ? j : e == j ? i : e;
  xs[idx] = x[b * N + src];
}

__global__ __launch_bounds__(256) void spin_ratio_kernel(const float* __restrict__ lp, const float* __restrict__ lps,
                                                         int B, int pair0, size_t total,
                                                         double2* __restrict__ ratio) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;  // total = (pair1 - pair0) B
  const size_t b = idx % B;
  const float* l0 = lp + 2 * b;
  const float* l1 = lps + 2 * idx;
  const double dr = (double)l1[0] - (double)l0[0], di = (double)l1[1] - (double)l0[1];
  const double2 r = amp_ratio(dr, di);
  const double re = r.x, im = r.y;
  const bool ok = isfinite(l0[0]) && isfinite(l0[1]) && isfinite(l1[0]) && isfinite(l1[1]) && isfinite(re) && isfinite(im);
  const double nan = quiet_nan();
  ratio[(size_t)pair0 * B + idx] = ok ? make_double2(re, im) : make_double2(nan, nan);
}

__global__ __launch_bounds__(256) void spin_walker_kernel(const float* __restrict__ lp,
                                                          const double2* __restrict__ ratio, int B, int P, double c0,
                                                          double2* __restrict__ s2, int32_t* __restrict__ valid) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  bool ok = isfinite(lp[2 * (size_t)b]) && isfinite(lp[2 * (size_t)b + 1]);
  double sr = 0.0, si = 0.0;
  for (int p = 0; p < P; ++p) {
    const double2 r = ratio[(size_t)p * B + b];
    ok = ok && isfinite(r.x) && isfinite(r.y);
    sr += r.x;
    si += r.y;
  }
  s2[b] = ok ? make_double2(c0 - sr, -si) : make_double2(quiet_nan(), quiet_nan());
  valid[b] = ok ? 1 : 0;
}

// block p < P: pairs[p] = the valid walkers' sum of ratio[p]; block P: total and nvalid from s2
__global__ __launch_bounds__(kSumNT) void spin_sum_kernel(const double2* __restrict__ ratio,
                                                          const double2* __restrict__ s2,
                                                          const int32_t* __restrict__ valid, int B, int P,
                                                          double2* __restrict__ pairs, double2* __restrict__ total,
                                                          int32_t* __restrict__ nvalid) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const double2* src = p < P ? ratio + (size_t)p * B : s2;
  double sum[2] = {0.0, 0.0};
  int cnt = 0;
  for (int b = tid; b < B; b += kSumNT) {
    if (!valid[b]) continue;
    const double2 v = src[b];
    sum[0] += v.x;
    sum[1] += v.y;
    ++cnt;
  }
  block_sum<kSumNT>(sum, cnt);
  if (tid == 0) {
    if (p < P) {
      pairs[p] = make_double2(sum[0], sum[1]);
    } else {
      *total = make_double2(sum[0], sum[1]);
      *nvalid = cnt;
    }
  }
}

}  // namespace

// ratio [P][B] double2, then valid [B] int32
size_t spin_workspace_bytes(int B, int P) { return ((size_t)P * B * 2) * sizeof(double) + (size_t)B * sizeof(int32_t); }

void launch_spin_exchange(const float* x, int B, int N, int n_up, int n_dn, int pair0, int pair1, float* xs,
                          hipStream_t s) {
  const size_t total = (size_t)(pair1 - pair0) * B * N;  // >= 1: the caller's check
  hipLaunchKernelGGL(spin_exchange_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<const float2*>(x), B, N, n_up, n_dn, pair0, total, reinterpret_cast<float2*>(xs));
}

void launch_spin_ratios(const float* logpsi, const float* logpsi_s, int B, int pair0, int pair1, void* workspace,
                        hipStream_t s) {
  const size_t total = (size_t)(pair1 - pair0) * B;
  hipLaunchKernelGGL(spin_ratio_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, logpsi, logpsi_s, B,
                     pair0, total, static_cast<double2*>(workspace));
}

void launch_spin_reduce(const float* logpsi, int B, int n_up, int n_dn, void* workspace, double* s2, double* pairs,
                        double* total, int32_t* nvalid, hipStream_t s) {
  const int P = n_up * n_dn, N = n_up + n_dn;
  double2* ratio = static_cast<double2*>(workspace);
  int32_t* valid = reinterpret_cast<int32_t*>(ratio + (size_t)P * B);
  const double c0 = 0.25 * (n_up - n_dn) * (n_up - n_dn) + 0.5 * N;
  hipLaunchKernelGGL(spin_walker_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logpsi, ratio, B, P, c0,
                     reinterpret_cast<double2*>(s2), valid);
  hipLaunchKernelGGL(spin_sum_kernel, dim3(P + 1), dim3(kSumNT), 0, s, ratio, reinterpret_cast<const double2*>(s2),
                     valid, B, P, reinterpret_cast<double2*>(pairs), reinterpret_cast<double2*>(total), nvalid);
}

}  // namespace dh
