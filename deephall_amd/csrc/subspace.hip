// Overlap, Hamiltonian and kinetic matrices of K wavefunctions on the walkers of the first of them
// (netobs/observables/subspace.py; not in the reference).  Stacked by state c, state 0 the one the
// walkers sample: logs[c][b] = (log|psi_c|, arg psi_c), e_l[c][b] = E_L of psi_c and ke[c][b] its
// kinetic part, all float32 pairs as dh_local_energy writes them, and a real shift[c] of the
// caller's.  With
//
//   r_c(b) = exp(logs[c][b] - logs[0][b] - shift[c]),
//   S[c][c'] = sum_b conj(r_c) r_c',   H[c][c'] = sum_b conj(r_c) r_c' E_c'(b),
//   T[c][c'] = sum_b conj(r_c) r_c' KE_c'(b)
//
// over the valid walkers, the operator on the ket: <psi_c | O | psi_c'> up to a common factor.
//
//   ratios  one thread per walker: the walker is valid when its 6 K inputs and its K ratios are
//           finite; r into the workspace as ratio[c][b] (NaN for an invalid walker), valid[b].
//   sums    one workgroup per (c, c') adds the six doubles of S, H and T in one pass over b, and one
//           more the count, by block_sum.
// The estimators' convention (estimator_common.h): two calls give identical bits.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kSumNT = 256;

__device__ __forceinline__ bool finite2(float2 v) { return isfinite(v.x) && isfinite(v.y); }

__global__ __launch_bounds__(256) void subspace_ratio_kernel(const float2* __restrict__ logs,
                                                             const float2* __restrict__ e_l,
                                                             const float2* __restrict__ ke, int B, int K,
                                                             const double* __restrict__ shift,
                                                             double2* __restrict__ ratio, int32_t* __restrict__ valid) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float2 l0 = logs[b];
  bool ok = true;
  for (int c = 0; c < K; ++c) {
    const size_t at = (size_t)c * B + b;
    ok = ok && finite2(logs[at]) && finite2(e_l[at]) && finite2(ke[at]);
  }
  // an overflowing ratio would poison the sums: its walker is dropped with the rest
  for (int c = 0; c < K; ++c) ok = ok && isfinite(exp((double)logs[(size_t)c * B + b].x - (double)l0.x - shift[c]));
  for (int c = 0; c < K; ++c) {
    const float2 l = logs[(size_t)c * B + b];
    const double2 r = amp_ratio((double)l.x - (double)l0.x - shift[c], (double)l.y - (double)l0.y);
    ratio[(size_t)c * B + b] = ok ? r : make_double2(quiet_nan(), quiet_nan());
  }
  valid[b] = ok ? 1 : 0;
}

// block q < K K: S, H, T [c][c'] with c = q / K, c' = q % K; block K K: nvalid
__global__ __launch_bounds__(kSumNT) void subspace_sum_kernel(const double2* __restrict__ ratio,
                                                              const int32_t* __restrict__ valid,
                                                              const float2* __restrict__ e_l,
                                                              const float2* __restrict__ ke, int B, int K,
                                                              double2* __restrict__ out, int32_t* __restrict__ nvalid) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const bool count = q == K * K;
  const size_t bra = (size_t)(count ? 0 : q / K) * B, ket = (size_t)(count ? 0 : q % K) * B;
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int b = tid; b < B; b += kSumNT) {
    if (!valid[b]) continue;
    const double2 u = ratio[bra + b], v = ratio[ket + b];
    const double wr = u.x * v.x + u.y * v.y;  // conj(u) v
    const double wi = u.x * v.y - u.y * v.x;
    const float2 e = e_l[ket + b], t = ke[ket + b];  // the operator acts on the ket
    const double er = e.x, ei = e.y, tr = t.x, ti = t.y;
    sum[0] += wr;
    sum[1] += wi;
    sum[2] += wr * er - wi * ei;
    sum[3] += wr * ei + wi * er;
    sum[4] += wr * tr - wi * ti;
    sum[5] += wr * ti + wi * tr;
    ++cnt;
  }
  block_sum<kSumNT>(sum, cnt);
  if (tid == 0) {
    if (count) {
      *nvalid = cnt;
    } else {
      const size_t kk = (size_t)K * K;
      out[q] = make_double2(sum[0], sum[1]);
      out[kk + q] = make_double2(sum[2], sum[3]);
      out[2 * kk + q] = make_double2(sum[4], sum[5]);
    }
  }
}

}  // namespace

// ratio [K][B] double2, then valid [B] int32
size_t subspace_workspace_bytes(int B, int K) {
  return ((size_t)K * B * 2) * sizeof(double) + (size_t)B * sizeof(int32_t);
}

void launch_subspace_accumulate(const float* logs, const float* e_l, const float* ke, int B, int K, const double* shift,
                                double* out, int32_t* nvalid, void* workspace, hipStream_t s) {
  double2* ratio = static_cast<double2*>(workspace);
  int32_t* valid = reinterpret_cast<int32_t*>(ratio + (size_t)K * B);
  const float2* e2 = reinterpret_cast<const float2*>(e_l);
  const float2* k2 = reinterpret_cast<const float2*>(ke);
  hipLaunchKernelGGL(subspace_ratio_kernel, dim3((B + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const float2*>(logs), e2, k2, B, K, shift, ratio, valid);
  hipLaunchKernelGGL(subspace_sum_kernel, dim3(K * K + 1), dim3(kSumNT), 0, s, ratio, valid, e2, k2, B, K,
                     reinterpret_cast<double2*>(out), nvalid);
}

}  // namespace dh
