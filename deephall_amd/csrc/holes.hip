// Overlap matrix of K quasihole configurations on the walkers of one of them
// (netobs/observables/hole_overlap.py; not in the reference).  With L[b][c] = log psi_c(R_b) in
// double (dh_hole_logs, quasihole.hip) and a real shift[c] of the caller's,
//
//   r[b][c] = exp(L[b][c] - L[b][0] - shift[c]),   S[c][c'] = sum_b conj(r[b][c]) r[b][c'],
//
// the sum over the valid walkers: <psi_c | psi_c'> up to a common factor when the walkers sample
// |psi_0|^2.
//
//   ratios  one thread per walker: the walker is valid when its 2 K log entries and its K ratios
//           are finite; r into the workspace as ratio[c][b] (NaN for an invalid walker), valid[b].
//   sums    one workgroup per (c, c'), and one more for the count, by block_sum.
// The estimators' convention (estimator_common.h): two calls give identical bits.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kSumNT = 256;

__global__ __launch_bounds__(256) void hole_ratio_kernel(const double2* __restrict__ L, int B, int K,
                                                         const double* __restrict__ shift,
                                                         double2* __restrict__ ratio, int32_t* __restrict__ valid) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double2* row = L + (size_t)b * K;
  const double2 l0 = row[0];
  bool ok = true;
  for (int c = 0; c < K; ++c) ok = ok && isfinite(row[c].x) && isfinite(row[c].y);
  // an overflowing ratio would poison the sums: its walker is dropped with the rest
  for (int c = 0; c < K; ++c) ok = ok && isfinite(exp(row[c].x - l0.x - shift[c]));
  for (int c = 0; c < K; ++c) {
    const double2 r = amp_ratio(row[c].x - l0.x - shift[c], row[c].y - l0.y);
    ratio[(size_t)c * B + b] = ok ? r : make_double2(quiet_nan(), quiet_nan());
  }
  valid[b] = ok ? 1 : 0;
}

// block q < K K: S[c][c'] with c = q / K, c' = q % K; block K K: nvalid
__global__ __launch_bounds__(kSumNT) void hole_sum_kernel(const double2* __restrict__ ratio,
                                                          const int32_t* __restrict__ valid, int B, int K,
                                                          double2* __restrict__ S, int32_t* __restrict__ nvalid) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const bool count = q == K * K;
  const double2* ra = ratio + (size_t)(count ? 0 : q / K) * B;
  const double2* rb = ratio + (size_t)(count ? 0 : q % K) * B;
  double sum[2] = {0.0, 0.0};
  int cnt = 0;
  for (int b = tid; b < B; b += kSumNT) {
    if (!valid[b]) continue;
    const double2 u = ra[b], v = rb[b];
    sum[0] += u.x * v.x + u.y * v.y;  // conj(u) v
    sum[1] += u.x * v.y - u.y * v.x;
    ++cnt;
  }
  block_sum<kSumNT>(sum, cnt);
  if (tid == 0) {
    if (count)
      *nvalid = cnt;
    else
      S[q] = make_double2(sum[0], sum[1]);
  }
}

}  // namespace

// ratio [K][B] double2, then valid [B] int32
size_t hole_workspace_bytes(int B, int K) { return ((size_t)K * B * 2) * sizeof(double) + (size_t)B * sizeof(int32_t); }

void launch_hole_gram(const double* L, int B, int K, const double* shift, double* S, int32_t* nvalid, void* workspace,
                      hipStream_t s) {
  double2* ratio = static_cast<double2*>(workspace);
  int32_t* valid = reinterpret_cast<int32_t*>(ratio + (size_t)K * B);
  hipLaunchKernelGGL(hole_ratio_kernel, dim3((B + 255) / 256), dim3(256), 0, s, reinterpret_cast<const double2*>(L), B,
                     K, shift, ratio, valid);
  hipLaunchKernelGGL(hole_sum_kernel, dim3(K * K + 1), dim3(kSumNT), 0, s, ratio, valid, B, K,
                     reinterpret_cast<double2*>(S), nvalid);
}

}  // namespace dh
