// Overlap penalty against K frozen lower states on the network's own walkers (orthogonal.py; not
// in the reference).  With d_kb = log phi_k(x_b) - log psi(x_b), x_b ~ |psi|^2:
//
//   F_k   = |mean_b e^{d_kb}|^2 / mean_b |e^{d_kb}|^2
//   R_b   = E_L,b - sum_k w_k eps_kb,   eps_kb = 1 - n_k z_kb / S_k,   w_k = lambda_k F_k
//
//   ortho_partial_kernel (dh_ortho_partial): workgroup k writes the shifted sums of state k, row k
//     of part [K][DH_NFID], by fidelity.hip's own reduction (fidelity_common.h): validity, the shift
//     m_k = max Re d_k and the order of addition are per state, and the row is bit for bit what
//     dh_fidelity_partial gives on (log psi, log phi_k).
//   ortho_residual_kernel (dh_ortho_residual): one thread per walker walks k = 0 .. K-1 and takes
//     w_k eps_kb from the local energy (or from 0), in double, rounded once to float32.
//
// The residual's product w_k eps_kb and its subtraction are rounded one by one: with K = 1, w = 1
// and no local energy the output is minus dh_fidelity_residual's, and with every w_k = 0 it is the
// local energy, bit for bit.
#include "dh_internal.h"
#include "fidelity_common.h"

namespace dh {
namespace {

__global__ __launch_bounds__(kFidNT) void ortho_partial_kernel(const float* __restrict__ lpsi,
                                                               const float* __restrict__ lphi, int B,
                                                               double* __restrict__ part) {
  const size_t k = blockIdx.x;
  fid_partial_block(lpsi, lphi + k * 2 * (size_t)B, B, part + k * DH_NFID);
}

// a - w e with the product rounded on its own
__device__ __forceinline__ double sub_scaled(double a, double w, double e) {
#pragma clang fp contract(off)
  const double p = w * e;
  return a - p;
}

__global__ __launch_bounds__(256) void ortho_residual_kernel(const float* __restrict__ lpsi,
                                                             const float* __restrict__ lphi, int B, int K,
                                                             const double* __restrict__ total,
                                                             const double* __restrict__ weight,
                                                             const float* __restrict__ e_l, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double rr = e_l ? (double)e_l[2 * (size_t)i] : 0.0;
  double ri = e_l ? (double)e_l[2 * (size_t)i + 1] : 0.0;
  bool ok = true;
  for (int k = 0; k < K; ++k) {
    const double* t = total + (size_t)k * DH_NFID;
    const double m = t[0], sr = t[1], si = t[2], n = t[4], w = weight[k];
    const double den = dot2(sr, sr, si, si);  // |S|^2 <= n^2: no overflow
    double dr, di;
    const bool valid = fid_d(lpsi, lphi + (size_t)k * 2 * (size_t)B, i, dr, di);
    if (!(valid && n > 0.0 && den > 0.0 && isfinite(w))) {
      ok = false;
      continue;
    }
    double er, ei;
    fid_eps(dr, di, m, sr, si, den, n, er, ei);
    rr = sub_scaled(rr, w, er);
    ri = sub_scaled(ri, w, ei);
  }
  out[2 * (size_t)i] = ok ? (float)rr : NAN;
  out[2 * (size_t)i + 1] = ok ? (float)ri : NAN;
}

}  // namespace

void launch_ortho_partial(const float* logpsi, const float* logphi, int B, int K, double* part, hipStream_t s) {
  hipLaunchKernelGGL(ortho_partial_kernel, dim3(K), dim3(kFidNT), 0, s, logpsi, logphi, B, part);
}

void launch_ortho_residual(const float* logpsi, const float* logphi, int B, int K, const double* total,
                           const double* weight, const float* e_l, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ortho_residual_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logpsi, logphi, B, K, total,
                     weight, e_l, out);
}

}  // namespace dh
