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
// wave_sum, then thread q adds component q of the 16 waves in order.  The device functions live in
// fidelity_common.h, which orthogonal.hip shares.
#include "dh_internal.h"
#include "fidelity_common.h"

namespace dh {
namespace {

constexpr int kNT = kFidNT;

__global__ __launch_bounds__(kNT) void fidelity_partial_kernel(const float* __restrict__ lpsi,
                                                               const float* __restrict__ lphi, int B,
                                                               double* __restrict__ part) {
  fid_partial_block(lpsi, lphi, B, part);
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
    double e_re, e_im;
    fid_eps(dr, di, m, sr, si, den, n, e_re, e_im);
    er = (float)e_re;
    ei = (float)e_im;
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
