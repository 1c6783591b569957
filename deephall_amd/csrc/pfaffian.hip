// The Moore-Read Pfaffian state at filling 1/2 (and 1/(2p) in general), and its local energy.
//
//   log psi = log Pf(A) + 2 p sum_{i<k} log w_ik,  A_ik = 1 / w_ik (i != k), A_ii = 0,
//   w_ik = u_i v_k - u_k v_i,  u = cos(theta/2) e^(i phi/2),  v = sin(theta/2) e^(-i phi/2)
//
// at flux 2Q = 2 p (N - 1) - 1, N even.  Pf(A) comes from a skew-symmetric elimination with
// pivoting (Parlett-Reid in 2x2 blocks): at step k = 0, 2, ... the largest |A[k][j]|, j > k, is
// brought to column k + 1 by swapping row and column j with k + 1 (a factor -1), the pivot
// P = A[k][k+1] is multiplied into Pf, and the trailing block takes the rank-2 skew update
//   A[i][j] += (A[i][k] A[k+1][j] - A[i][k+1] A[k][j]) / P,   i, j >= k + 2,
// which is the row operation row_i += (A[i][k] / P) row_{k+1} - (A[i][k+1] / P) row_k alone: the
// matching column operation only clears rows k, k + 1, which are not read again.  The value-only
// instantiation (dh_logpsi, dh_mcmc_step) keeps u, v and A and does this in place.
//
// The energy instantiation applies the same row operations and swaps to [A | I]; the right
// half becomes M with M A M^T = D, D the block diagonal of the pivots, and
//   W = A^-1 = M^T D^-1 M,   W[i][j] = sum_k (M[k+1][i] M[k][j] - M[k][i] M[k+1][j]) / P_k.
// The left half and so the pivots are those of the value instantiation.  With n(a) the electron
// of coordinate a, d_a[k] = d(1 / w_{n(a) k}) / dx_a (dA_a = e_n d_a^T - d_a e_n^T), y_a = W d_a:
//   d_a log Pf     = sum_k W[k][n(a)] d_a[k] = -y_a[n(a)]
//   d_a d_b log Pf = 1/2 tr(W d2A_ab) - y_a[n(b)] y_b[n(a)] + (d_a . y_b) W[n(b)][n(a)]
//   1/2 tr(W d2A_ab) = sum_k W[k][n] d2(1 / w_nk) / dx_a dx_b        (n(a) = n(b) = n)
//                    = W[n(b)][n(a)] d2(1 / w_{n(a) n(b)}) / dx_a dx_b  (otherwise)
// plus the pair part with weight 2 p as in cf.hip.  The full complex Hessian of log psi goes to
// the kinetic / angular-momentum formulas of hamiltonian.py:115-169 exactly as in laughlin.hip
// and cf.hip.  One 64-thread workgroup per walker, complex double in LDS.
#include "dh_internal.h"
#include "device_common.h"

namespace dh {
namespace {

struct zd {
  double re, im;
};
__device__ __forceinline__ zd operator+(zd a, zd b) { return zd{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ zd operator-(zd a, zd b) { return zd{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ zd operator*(zd a, zd b) { return zd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ zd operator*(double s, zd a) { return zd{s * a.re, s * a.im}; }
__device__ __forceinline__ zd zinv(zd b) {
  const double d = b.re * b.re + b.im * b.im;
  return zd{b.re / d, -b.im / d};
}

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

// u, v and their derivatives of electron (th, ph); the first two entries alone if !FULL
template <bool FULL>
__device__ void uv_derivs(double th, double ph, zd* q) {
  double sh, ch, sp, cp;
  sincos(0.5 * th, &sh, &ch);
  sincos(0.5 * ph, &sp, &cp);
  const zd eu{cp, sp}, ev{cp, -sp};  // e^(i phi/2), e^(-i phi/2)
  const zd u = ch * eu, v = sh * ev;
  q[0] = u;
  q[1] = v;
  if (!FULL) return;
  const zd I{0.0, 1.0};
  q[2] = -0.5 * sh * eu;      // du/dth
  q[3] = 0.5 * (I * u);       // du/dph
  q[4] = 0.5 * ch * ev;       // dv/dth
  q[5] = -0.5 * (I * v);      // dv/dph
  q[6] = -0.25 * u;           // d2u/dth2
  q[7] = 0.5 * (I * q[2]);    // d2u/dth dph
  q[8] = -0.25 * u;           // d2u/dph2
  q[9] = -0.25 * v;           // d2v/dth2
  q[10] = -0.5 * (I * q[4]);  // d2v/dth dph
  q[11] = -0.25 * v;          // d2v/dph2
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
  // skew elimination with pivoting (|re| + |im| pivot, as det.hip) on [A | I], or on A alone for
  // the value: the left block and so the pivots are the same
  for (int k = 0; k < N; k += 2) {
    if (tid == 0) {
      double best = -1.0;
      int bj = k + 1;
      for (int j = k + 1; j < N; ++j) {
        const double v = fabs(G[k * ld + j].re) + fabs(G[k * ld + j].im);
        if (v > best) {
          best = v;
          bj = j;
        }
      }
      *pivd = (double)bj;
    }
    __syncthreads();
    const int pc = (int)*pivd;
    if (pc != k + 1) {  // rows, then columns (of the left block)
      for (int c = tid; c < ld; c += nt) {
        const zd t = G[(k + 1) * ld + c];
        G[(k + 1) * ld + c] = G[pc * ld + c];
        G[pc * ld + c] = t;
      }
      __syncthreads();
      for (int r = tid; r < N; r += nt) {
        const zd t = G[r * ld + k + 1];
        G[r * ld + k + 1] = G[r * ld + pc];
        G[r * ld + pc] = t;
      }
      __syncthreads();
    }
    const zd P = G[k * ld + k + 1];
    const zd Pinv = zinv(P);
    if (tid == 0) {
      logpf->re += 0.5 * log(P.re * P.re + P.im * P.im);
      logpf->im += atan2(P.im, P.re) + (pc != k + 1 ? M_PI : 0.0);
      if (ENERGY) pinv[k >> 1] = Pinv;
    }
    for (int r = k + 2 + tid; r < N; r += nt) {
      f0[r] = G[r * ld + k] * Pinv;
      f1[r] = G[r * ld + k + 1] * Pinv;
    }
    __syncthreads();
    for (int idx = tid; idx < N * ld; idx += nt) {
      const int r = idx / ld, c = idx % ld;
      if (r < k + 2 || c < k + 2) continue;
      G[r * ld + c] = G[r * ld + c] + f0[r] * G[(k + 1) * ld + c] - f1[r] * G[k * ld + c];
    }
    __syncthreads();
  }
  // pair part of log psi (value): 2 p sum_{i<j} log w_ij
  double lre = 0.0, lim = 0.0;
  for (int q = tid; q < NN; q += nt) {
    const int i = q / N, j = q % N;
    if (j <= i) continue;
    const zd w = UV[SU * i] * UV[SU * j + 1] - UV[SU * j] * UV[SU * i + 1];
    lre += 0.5 * p2 * log(w.re * w.re + w.im * w.im);
    lim += p2 * atan2(w.im, w.re);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lre += __shfl_xor(lre, o, 64);
    lim += __shfl_xor(lim, o, 64);
  }
  if (!ENERGY) {
    if (tid == 0) {
      out_lp[2 * b] = (float)(logpf->re + lre);
      out_lp[2 * b + 1] = (float)remainder(logpf->im + lim, 2.0 * M_PI);
    }
    return;
  }
  zd *W = sm + L.W, *d = sm + L.d, *Y = sm + L.y, *g = sm + L.g, *H = sm + L.H;
  // W = M^T D^-1 M
  for (int idx = tid; idx < NN; idx += nt) {
    const int i = idx / N, j = idx % N;
    zd s{0.0, 0.0};
    for (int k = 0; k < N; k += 2) {
      const zd *m0 = G + k * ld + N, *m1 = m0 + ld;
      s = s + (m1[i] * m0[j] - m0[i] * m1[j]) * pinv[k >> 1];
    }
    W[idx] = s;
  }
  __syncthreads();
  // y[a][j] = (W d_a)[j],  a = 2 e + (0 theta | 1 phi)
  for (int idx = tid; idx < T * N; idx += nt) {
    const int a = idx / N, j = idx % N;
    zd s{0.0, 0.0};
    for (int k = 0; k < N; ++k) s = s + W[j * N + k] * d[a * N + k];
    Y[idx] = s;
  }
  __syncthreads();
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
  // hamiltonian.py:115-169 with g and the full Hessian; potential (double geometry)
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // KE re, KE im, L2 re, PE
  double lz = 0.0, lz2 = 0.0;
  // per electron terms (one thread per electron i), pair terms over (i, j)
  for (int idx = tid; idx < NN; idx += nt) {
    const int i = idx / N, j = idx % N;
    double sti, cti, spi, cpi, stj, ctj, spj, cpj;
    sincos((double)x[2 * (b * N + i)], &sti, &cti);
    sincos((double)x[2 * (b * N + i) + 1], &spi, &cpi);
    sincos((double)x[2 * (b * N + j)], &stj, &ctj);
    sincos((double)x[2 * (b * N + j) + 1], &spj, &cpj);
    const zd gti = g[2 * i], gpi = g[2 * i + 1], gtj = g[2 * j], gpj = g[2 * j + 1];
    const zd htt = H[(2 * i) * T + 2 * j] + gti * gtj, htp = H[(2 * i) * T + 2 * j + 1] + gti * gpj;
    const zd hpp = H[(2 * i + 1) * T + 2 * j + 1] + gpi * gpj;
    const double phi_i[3] = {-spi, cpi, 0.0}, phi_j[3] = {-spj, cpj, 0.0};
    const double thp_i[3] = {cpi * cti / sti, spi * cti / sti, -1.0}, thp_j[3] = {cpj * ctj / stj, spj * ctj / stj, -1.0};
    const double rj[3] = {stj * cpj, stj * spj, ctj}, ri[3] = {sti * cpi, sti * spi, cti};
    double pp = 0.0, ptp = 0.0, tt = 0.0, mi_mj = 0.0, mj_phi = 0.0, mj_thp = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double mj = Q * (thp_j[k] * ctj + rj[k]), mi = Q * (thp_i[k] * cti + ri[k]);
      pp += phi_i[k] * phi_j[k];
      ptp += phi_i[k] * thp_j[k];
      tt += thp_i[k] * thp_j[k];
      mi_mj += mi * mj;
      mj_phi += mj * phi_i[k];
      mj_thp += mj * thp_i[k];
    }
    // 2 phi_i.thp_j P_tp - phi_i.phi_j P_tt - thp_i.thp_j P_pp - 2i m_j.(phi_i g_t_i - thp_i g_p_i) + m_i.m_j
    zd term = 2.0 * ptp * htp - pp * htt - tt * hpp + zd{mi_mj, 0.0};
    const zd cross = mj_phi * gti - mj_thp * gpi;
    term = term - zd{-2.0 * cross.im, 2.0 * cross.re};  // - 2i * cross
    v[2] += term.re;
    lz2 -= hpp.re;
    if (i == j) {
      const double cot = cti / sti, s2 = sti * sti;
      // square_grad, grad_grad (Laplacian), magnetic (hamiltonian.py:115-133)
      const zd sq = gti * gti + (1.0 / s2) * (gpi * gpi);
      const zd lap = cot * gti + H[(2 * i) * T + 2 * i] + (1.0 / s2) * H[(2 * i + 1) * T + 2 * i + 1];
      const zd mag = zd{(Q * cot) * (Q * cot), 0.0} + zd{0.0, 2.0 * Q * cti / s2} * gpi;
      const zd ke = zd{0.0, 0.0} - lap - sq + mag;
      v[0] += ke.re;
      v[1] += ke.im;
      v[2] -= gti.re * cot;  // - sum g_theta cot theta (real part)
      lz += gpi.im;
      {
        double pe = 0.0;
        for (int jj = i + 1; jj < N; ++jj) {
          double a1, a2, a3, a4;
          sincos((double)x[2 * (b * N + jj)], &a1, &a2);
          sincos((double)x[2 * (b * N + jj) + 1], &a3, &a4);
          const double u = ri[0] * a1 * a4 + ri[1] * a1 * a3 + ri[2] * a2;
          pe += interaction == DH_INTERACTION_COULOMB ? 1.0 / sqrt(2.0 - 2.0 * u) : 1.0 + (Q + 1.0) / Q * u;
        }
        v[3] += pe;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int q = 0; q < 4; ++q) v[q] += __shfl_xor(v[q], o, 64);
    lz += __shfl_xor(lz, o, 64);
    lz2 += __shfl_xor(lz2, o, 64);
  }
  if (tid == 0) {
    const double r2 = radius * radius;
    double pe = v[3];
    if (interaction == DH_INTERACTION_COULOMB) pe /= radius;
    pe *= lambda;
    const double ke_re = v[0] / (2.0 * r2), ke_im = v[1] / (2.0 * r2);
    e_l[2 * b] = (float)(ke_re + pe);
    e_l[2 * b + 1] = (float)ke_im;
    float* ob = obs + 8 * (size_t)b;
    ob[0] = (float)ke_re;
    ob[1] = (float)ke_im;
    ob[2] = (float)pe;
    ob[3] = (float)lz;
    ob[4] = (float)lz2;
    ob[5] = (float)v[2];
    ob[6] = (float)(logpf->re + lre);
    ob[7] = (float)remainder(logpf->im + lim, 2.0 * M_PI);
  }
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
