// The Moore-Read Pfaffian state at filling 1/2 (and 1/(2p) in general), and its local energy.
//
//   log psi = log Pf(A) + 2 p sum_{i<k} log w_ik,  A_ik = 1 / w_ik (i != k), A_ii = 0,
//   w_ik = u_i v_k - u_k v_i,  u = cos(theta/2) e^(i phi/2),  v = sin(theta/2) e^(-i phi/2)
//
// at flux 2Q = 2 p (N - 1) - 1, N even.  Pf(A) comes from trial_common.h's skew_eliminate (the
// algorithm is explained there): in place on A for the value-only instantiation (dh_logpsi,
// dh_mcmc_step), on [A | I] for the energy, whose right half becomes M with M A M^T = D, D the
// block diagonal of the pivots, and W = A^-1 = M^T D^-1 M (pfaffian_inverse).  The left half
// and so the pivots are those of the value instantiation.  With n(a) the electron
// of coordinate a, d_a[k] = d(1 / w_{n(a) k}) / dx_a (dA_a = e_n d_a^T - d_a e_n^T), y_a = W d_a:
//   d_a log Pf     = sum_k W[k][n(a)] d_a[k] = -y_a[n(a)]
//   d_a d_b log Pf = 1/2 tr(W d2A_ab) - y_a[n(b)] y_b[n(a)] + (d_a . y_b) W[n(b)][n(a)]
//   1/2 tr(W d2A_ab) = sum_k W[k][n] d2(1 / w_nk) / dx_a dx_b        (n(a) = n(b) = n)
//                    = W[n(b)][n(a)] d2(1 / w_{n(a) n(b)}) / dx_a dx_b  (otherwise)
// plus the pair part with weight 2 p as in cf.hip.  The full complex Hessian of log psi goes to
// the kinetic / angular-momentum formulas of hamiltonian.py:115-169 exactly as in laughlin.hip
// and cf.hip.  One 64-thread workgroup per walker, complex double in LDS.
#include "trial_common.h"

namespace dh {
namespace {

// LDS layout in zd units.  Value only: u, v per electron, A [N][N], the two factor columns.
struct PSm {
  int uv, G, misc, W, d, y, g, H, total;
};
__host__ __device__ inline PSm psm_layout(int N, bool energy) {
  PSm L{};
  int o = 0;
  L.uv = o;  // energy: u, v, du[2], dv[2], d2u[3], d2v[3] = 12 per electron
  o += (energy ? 12 : 2) * N;
  L.G = o;  // energy: augmented [A | I] -> [. | M]
  o += (energy ? 2 : 1) * N * N;
  L.misc = o;  // factor columns f0 [N], f1 [N], (energy) 1 / pivot [N], log Pf, pivot column
  o += (energy ? 3 : 2) * N + 4;
  if (energy) {
    L.W = o;
    o += N * N;
    L.d = o;
    o += 2 * N * N;  // d[a][k] = d(1 / w_{n(a) k}) / dx_a
    L.y = o;
    o += 2 * N * N;  // y[a][j] = (W d_a)[j]
    L.g = o;
    o += 2 * N;
    L.H = o;
    o += 4 * N * N;
  }
  L.total = o;
  return L;
}

template <bool ENERGY>
__global__ __launch_bounds__(64) void pfaffian_kernel(const float* __restrict__ x, float* __restrict__ out_lp,
                                                      float* __restrict__ e_l, float* __restrict__ obs, int N, int pj,
                                                      double Q, double radius, double lambda, int interaction) {
  extern __shared__ double smd[];
  zd* sm = reinterpret_cast<zd*>(smd);
  const PSm L = psm_layout(N, ENERGY);
  constexpr int SU = ENERGY ? 12 : 2;
  zd *UV = sm + L.uv, *G = sm + L.G, *f0 = sm + L.misc, *f1 = f0 + N;
  zd* pinv = f1 + N;                       // energy only: 1 / pivot of step k at [k / 2]
  zd* logpf = f1 + (ENERGY ? 2 * N : N);   // one entry
  double* pivd = &logpf[1].re;             // the pivot column of the current step
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int NN = N * N, T = 2 * N, ld = ENERGY ? 2 * N : N;
  const double p2 = 2.0 * pj;
  for (int i = tid; i < N; i += nt)
    uv_derivs<ENERGY>((double)x[2 * (b * N + i)], (double)x[2 * (b * N + i) + 1], UV + SU * i);
  if (tid == 0) *logpf = zd{0.0, 0.0};
  __syncthreads();
  // A (augmented with I) and, for the energy, d[a][k]
  for (int idx = tid; idx < NN; idx += nt) {
    const int i = idx / N, k = idx % N;
    const zd *qi = UV + SU * i, *qk = UV + SU * k;
    zd a{0.0, 0.0};
    if (i != k) a = zinv(qi[0] * qk[1] - qk[0] * qi[1]);
    G[i * ld + k] = a;
    if (ENERGY) {
      G[i * ld + N + k] = zd{i == k ? 1.0 : 0.0, 0.0};
      zd* d = sm + L.d;
      for (int c = 0; c < 2; ++c) {
        const zd wx = qi[2 + c] * qk[1] - qk[0] * qi[4 + c];
        d[(2 * i + c) * N + k] = i == k ? zd{0.0, 0.0} : zd{0.0, 0.0} - wx * a * a;
      }
    }
  }
  __syncthreads();
  // on [A | I], or on A alone for the value: the left block and so the pivots are the same
  skew_eliminate<ENERGY>(G, N, ld, f0, f1, pinv, logpf, pivd, tid, nt);
  // pair part of log psi (value): 2 p sum_{i<j} log w_ij
  const zd lpair = pair_logpsi(UV, SU, N, p2, false, tid, nt);
  if (!ENERGY) {
    if (tid == 0) {
      out_lp[2 * b] = (float)(logpf->re + lpair.re);
      out_lp[2 * b + 1] = (float)remainder(logpf->im + lpair.im, 2.0 * M_PI);
    }
    return;
  }
  zd *W = sm + L.W, *d = sm + L.d, *Y = sm + L.y, *g = sm + L.g, *H = sm + L.H;
  // W = M^T D^-1 M and y[a][j] = (W d_a)[j],  a = 2 e + (0 theta | 1 phi)
  pfaffian_inverse(G, N, pinv, d, W, Y, tid, nt);
  // gradient: Pfaffian + pairs
  for (int a = tid; a < T; a += nt) {
    const int e = a >> 1, c = a & 1;
    zd s = zd{0.0, 0.0} - Y[a * N + e];
    const zd* qe = UV + 12 * e;
    for (int j = 0; j < N; ++j) {
      if (j == e) continue;
      const zd* qj = UV + 12 * j;
      const zd w = qe[0] * qj[1] - qj[0] * qe[1];
      const zd dw = qe[2 + c] * qj[1] - qj[0] * qe[4 + c];
      s = s + p2 * (dw * zinv(w));
    }
    g[a] = s;
  }
  // Hessian: every entry costs one pass over the electrons (the dot product d_a . y_b off the
  // diagonal blocks, the second derivatives of electron n's row on them, where W[n][n] = 0)
  for (int idx = tid; idx < T * T; idx += nt) {
    const int a = idx / T, bb = idx % T, ea = a >> 1, ca = a & 1, eb = bb >> 1, cb = bb & 1;
    zd h = zd{0.0, 0.0} - Y[a * N + eb] * Y[bb * N + ea];
    const zd* qa = UV + 12 * ea;
    if (ea == eb) {
      const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
      for (int j = 0; j < N; ++j) {
        if (j == ea) continue;
        const zd* qj = UV + 12 * j;
        const zd ai = zinv(qa[0] * qj[1] - qj[0] * qa[1]);
        const zd fx = (qa[2 + ca] * qj[1] - qj[0] * qa[4 + ca]) * ai;  // w_x / w
        const zd fy = (qa[2 + cb] * qj[1] - qj[0] * qa[4 + cb]) * ai;
        const zd fxy = (qa[6 + k] * qj[1] - qj[0] * qa[9 + k]) * ai;
        // d2(1/w) = (2 w_x w_y / w^2 - w_xy / w) / w;  d2 log w = w_xy / w - w_x w_y / w^2
        h = h + W[j * N + ea] * ((2.0 * (fx * fy) - fxy) * ai) + p2 * (fxy - fx * fy);
      }
    } else {
      const zd* qb = UV + 12 * eb;
      const zd ai = zinv(qa[0] * qb[1] - qb[0] * qa[1]);
      const zd fx = (qa[2 + ca] * qb[1] - qb[0] * qa[4 + ca]) * ai;  // d/dx_a
      const zd fy = (qa[0] * qb[4 + cb] - qb[2 + cb] * qa[1]) * ai;  // d/dy_b
      const zd fxy = (qa[2 + ca] * qb[4 + cb] - qb[2 + cb] * qa[4 + ca]) * ai;
      zd dy{0.0, 0.0};
      for (int j = 0; j < N; ++j) dy = dy + d[a * N + j] * Y[bb * N + j];
      h = h + W[eb * N + ea] * (dy + (2.0 * (fx * fy) - fxy) * ai) + p2 * (fxy - fx * fy);
    }
    H[idx] = h;
  }
  __syncthreads();
  hamiltonian_tail(x, b, N, g, H, Q, radius, lambda, interaction, logpf, lpair, e_l, obs, tid, nt);
}

}  // namespace

size_t pfaffian_smem_bytes(int N, bool energy) { return (size_t)psm_layout(N, energy).total * 2 * sizeof(double); }

void launch_pfaffian(const Dims& d, const float* x, int p, float* logpsi, float* e_l, float* obs, int nw,
                     hipStream_t s) {
  if (e_l) {
    const size_t bytes = pfaffian_smem_bytes(d.N, true);
    ensure_smem(pfaffian_kernel<true>, bytes);
    hipLaunchKernelGGL(pfaffian_kernel<true>, dim3(nw), dim3(64), bytes, s, x, logpsi, e_l, obs, d.N, p, (double)d.Q,
                       (double)d.r, (double)d.lambda, d.interaction);
  } else {
    const size_t bytes = pfaffian_smem_bytes(d.N, false);
    hipLaunchKernelGGL(pfaffian_kernel<false>, dim3(nw), dim3(64), bytes, s, x, logpsi, e_l, obs, d.N, p, (double)d.Q,
                       (double)d.r, (double)d.lambda, d.interaction);
  }
}

}  // namespace dh
