// Jain composite-fermion states with two Lambda levels, and their local energy.
//
//   log psi = log det E + 2 p sum_{i<k} log w_ik,  w_ik = u_i v_k - u_k v_i,
//   u = cos(theta/2) e^(i phi/2),  v = sin(theta/2) e^(-i phi/2),  Q1 = Q - p (N - 1)
//
// One column of E per occupied orbital (n, m), A = Q1 + m, B = Q1 - m:
//   n = 0:  E_i = u_i^A v_i^B
//   n = 1:  E_i = (A + 1) u_i^A v_i^(B+1) Dv_i - (B + 1) u_i^(A+1) v_i^B Du_i,
//           Du_i = p sum_{k != i} v_k / w_ik,  Dv_i = -p sum_{k != i} u_k / w_ik
//         = -sum_{k != i} h_ik,  h_ik = (al P1_i u_k + be P2_i v_k) / w_ik,
//           P1 = u^A v^(B+1), P2 = u^(A+1) v^B, al = p (A + 1), be = p (B + 1)
// (the LLL-projected second-level orbital; an exponent -1 at the edge m = +-(Q1 + 1) only
// appears with weight 0 and is left out).  At p = 1 an n = 1 column is the quasiparticle
// column of laughlin.hip; here the state has a set D of such dense columns instead of one,
// and the determinant algebra is the rank-|D| form of that kernel's rank-1 one.  With
// W = E^-1, n(a) the electron of coordinate a, rho_a the row derivative over the n = 0
// columns, c_a^L[i] = dE_iL / dx_a, Y_a^L = W c_a^L, z_L = row L of W, r_a = rho_a^T W and
// G_a[L'][L] = Y_a^L[L'] (L, L' in D):
//   tr(W dE_a)          = r_a[n(a)] + tr G_a
//   tr(W dE_a W dE_b)   = r_a[n(b)] r_b[n(a)] + sum_L (rho_a . Y_b^L) z_L[n(a)]
//                         + sum_L z_L[n(b)] (rho_b . Y_a^L) + tr(G_a G_b)
//   tr(W d2E_ab)        = [n(a) = n(b)] sum_{j not in D} W[j][n] d2E_nj
//                         + sum_{L in D} sum_i z_L[i] d2E_iL / dx_a dx_b
// The full complex Hessian of log psi goes to the kinetic / angular-momentum formulas of
// hamiltonian.py:115-169 exactly as in laughlin.hip.  One 64-thread workgroup per walker,
// complex double in LDS.  The value-only instantiation (dh_logpsi, dh_mcmc_step) keeps only
// u, v and E: it eliminates E in place (the pivots are those of the energy instantiation's
// [E | I]) and needs none of the derivative storage, so many walkers share a CU.
//
// Column table (device ints): tab[3 j + (0 level, 1 A, 2 B)] for the N columns, then |D|, p,
// then the column of each member of D.
#include "trial_common.h"

namespace dh {
namespace {

// LDS layout in zd units.  Value only: u, v per electron, E [N][N], the pivot column.
struct CSm {
  int uv, E, misc, dE, d2E, Einv, R, g, H, P, c, Y, S, total;
};
__host__ __device__ inline CSm csm_layout(int N, int nD, bool energy) {
  CSm L{};
  int o = 0;
  L.uv = o;  // energy: u, v, du[2], dv[2], d2u[3], d2v[3] = 12 per electron
  o += (energy ? 12 : 2) * N;
  L.E = o;  // energy: augmented [E | I] -> [I | E^-1]
  o += (energy ? 2 : 1) * N * N;
  L.misc = o;  // pivot factors [N], log det, pivot row
  o += N + 4;
  if (energy) {
    L.dE = o;
    o += 2 * N * N;  // [coord theta/phi][i][j] (row i only: own electron; zero in D)
    L.d2E = o;
    o += 3 * N * N;  // [tt, tp, pp][i][j]
    L.Einv = o;
    o += N * N;
    L.R = o;
    o += 2 * N * N;  // R[a][i] = sum_q dE[a][e_a][q] Einv[q][i]
    L.g = o;
    o += 2 * N;
    L.H = o;
    o += 4 * N * N;
    L.P = o;
    o += 12 * N * nD;  // [i][d]: P1, P2 (value, d1[2], d2[3])
    L.c = o;
    o += 2 * N * nD * N;  // c[a][d][i] = dE_{i L_d} / dx_a
    L.Y = o;
    o += 2 * N * nD * N;  // Y[a][d][j] = (E^-1 c_a^{L_d})[j]
    L.S = o;
    o += nD ? 3 * N * N : 0;  // S[i][k][tt, tp, pp]: the pair (i, k)'s share of the diagonal block (i, i)
  }
  L.total = o;
  return L;
}

template <bool ENERGY>
__global__ __launch_bounds__(64) void cf_kernel(const float* __restrict__ x, const int* __restrict__ tab,
                                                float* __restrict__ out_lp, float* __restrict__ e_l,
                                                float* __restrict__ obs, int N, double Q, double radius, double lambda,
                                                int interaction) {
  extern __shared__ double smd[];
  zd* sm = reinterpret_cast<zd*>(smd);
  const int nD = tab[3 * N], pj = tab[3 * N + 1];
  const int* dcol = tab + 3 * N + 2;
  const CSm L = csm_layout(N, nD, ENERGY);
  constexpr int SU = ENERGY ? 12 : 2;
  zd *UV = sm + L.uv, *E = sm + L.E, *fac = sm + L.misc;
  zd* logdet = fac + N;           // one entry
  double* pivd = &fac[N + 1].re;  // the pivot row of the current step
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int NN = N * N, T = 2 * N, ld = ENERGY ? 2 * N : N;
  const double p2 = 2.0 * pj;
  for (int i = tid; i < N; i += nt)
    uv_derivs<ENERGY>((double)x[2 * (b * N + i)], (double)x[2 * (b * N + i) + 1], UV + SU * i);
  if (tid == 0) *logdet = zd{0.0, 0.0};
  __syncthreads();
  if (ENERGY) {
    zd *dE = sm + L.dE, *d2E = sm + L.d2E, *PP = sm + L.P, *cX = sm + L.c;
    // P1, P2 of every (electron, dense column)
    for (int idx = tid; idx < N * nD; idx += nt) {
      const int i = idx / nD, j = dcol[idx % nD], A = tab[3 * j + 1], B = tab[3 * j + 2];
      zd* P = PP + 12 * idx;
      for (int t = 0; t < 12; ++t) P[t] = zd{0.0, 0.0};
      if (A + 1 != 0) monomial(UV + 12 * i, A, B + 1, P, P + 1, P + 3);
      if (B + 1 != 0) monomial(UV + 12 * i, A + 1, B, P + 6, P + 7, P + 9);
    }
    // E (augmented with I) and the derivatives of its n = 0 columns (row i: electron i only)
    for (int idx = tid; idx < NN; idx += nt) {
      const int i = idx / N, j = idx % N;
      zd val{0.0, 0.0}, d1[2] = {{0.0, 0.0}, {0.0, 0.0}}, d2[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
      if (tab[3 * j] == 0) monomial(UV + 12 * i, tab[3 * j + 1], tab[3 * j + 2], &val, d1, d2);
      E[i * ld + j] = val;
      E[i * ld + N + j] = zd{i == j ? 1.0 : 0.0, 0.0};
      dE[idx] = d1[0];
      dE[NN + idx] = d1[1];
      for (int k = 0; k < 3; ++k) d2E[k * NN + idx] = d2[k];
    }
    __syncthreads();
    // dense columns: E_{i L_d} and c[a][d][i] (thread per (i, d); first derivatives only, so
    // the denominator is recomputed per column here and shared in the second-derivative pass)
    for (int idx = tid; idx < N * nD; idx += nt) {
      const int i = idx / nD, d = idx % nD, j = dcol[d];
      const double al = pj * (tab[3 * j + 1] + 1.0), be = pj * (tab[3 * j + 2] + 1.0);
      zd X{0.0, 0.0}, own0{0.0, 0.0}, own1{0.0, 0.0};
      for (int k = 0; k < N; ++k) {
        if (k == i) continue;
        PairDen den;
        PairD pd;
        pair_den<false>(UV + 12 * i, UV + 12 * k, den);
        pair_col<false>(UV + 12 * i, UV + 12 * k, PP + 12 * idx, al, be, den, pd);
        X = X - pd.h;
        own0 = own0 - pd.d[0];
        own1 = own1 - pd.d[1];
        cX[((2 * k) * nD + d) * N + i] = zd{0.0, 0.0} - pd.d[2];
        cX[((2 * k + 1) * nD + d) * N + i] = zd{0.0, 0.0} - pd.d[3];
      }
      cX[((2 * i) * nD + d) * N + i] = own0;
      cX[((2 * i + 1) * nD + d) * N + i] = own1;
      E[i * ld + j] = X;
    }
  } else {
    for (int idx = tid; idx < NN; idx += nt) {
      const int i = idx / N, j = idx % N, A = tab[3 * j + 1], B = tab[3 * j + 2];
      const zd u = UV[2 * i], v = UV[2 * i + 1];
      zd val;
      if (tab[3 * j] == 0) {
        val = zpow(u, A) * zpow(v, B);
      } else {
        const double al = pj * (A + 1.0), be = pj * (B + 1.0);
        const zd P1 = A + 1 != 0 ? zpow(u, A) * zpow(v, B + 1) : zd{0.0, 0.0};
        const zd P2 = B + 1 != 0 ? zpow(u, A + 1) * zpow(v, B) : zd{0.0, 0.0};
        val = zd{0.0, 0.0};
        for (int k = 0; k < N; ++k) {
          if (k == i) continue;
          const zd uk = UV[2 * k], vk = UV[2 * k + 1];
          val = val - (al * (P1 * uk) + be * (P2 * vk)) * zdiv(zd{1.0, 0.0}, u * vk - uk * v);
        }
      }
      E[i * ld + j] = val;
    }
  }
  __syncthreads();
  // [E | I] -> [I | E^-1], or E alone for the value
  gauss_jordan(E, N, ld, fac, logdet, pivd, tid, nt);
  // pair part of log psi (value): 2 p sum_{i<j} log w_ij
  const zd lpair = pair_logpsi(UV, SU, N, p2, false, tid, nt);
  if (!ENERGY) {
    if (tid == 0) {
      out_lp[2 * b] = (float)(logdet->re + lpair.re);
      out_lp[2 * b + 1] = (float)remainder(logdet->im + lpair.im, 2.0 * M_PI);
    }
    return;
  }
  zd *dE = sm + L.dE, *d2E = sm + L.d2E, *Einv = sm + L.Einv, *R = sm + L.R, *g = sm + L.g, *H = sm + L.H;
  zd *PP = sm + L.P, *cX = sm + L.c, *Y = sm + L.Y, *S = sm + L.S;
  for (int idx = tid; idx < NN; idx += nt) Einv[idx] = E[(idx / N) * ld + N + idx % N];
  __syncthreads();
  // R[a][i] = sum_q dE[a][e_a][q] Einv[q][i],  a = 2 e + (0 theta | 1 phi)
  for (int idx = tid; idx < T * N; idx += nt) {
    const int a = idx / N, i = idx % N, e = a >> 1, c = a & 1;
    zd s{0.0, 0.0};
    for (int q = 0; q < N; ++q) s = s + dE[c * NN + e * N + q] * Einv[q * N + i];
    R[idx] = s;
  }
  // Y[a][d][j] = (E^-1 c_a^{L_d})[j]
  for (int idx = tid; idx < T * nD * N; idx += nt) {
    const int ad = idx / N, j = idx % N;
    zd s{0.0, 0.0};
    for (int i = 0; i < N; ++i) s = s + Einv[j * N + i] * cX[ad * N + i];
    Y[idx] = s;
  }
  // H <- T2[a][b] = sum_d sum_i z_d[i] d2E_{i L_d} / dx_a dx_b, z_d = row L_d of E^-1.  One
  // unordered pair i < k per thread: E_{i L} = -sum h_ik has i as its own electron and k as
  // the other one, E_{k L} the reverse; the denominator's derivatives are formed once per
  // ordered pair and the columns loop inside.  The cross blocks (i, k), (k, i) are complete
  // here; the diagonal blocks collect a share S[i][k] (tt, tp, pp) from every pair.
  for (int idx = tid; idx < (nD ? 0 : T * T); idx += nt) H[idx] = zd{0.0, 0.0};  // no dense column
  for (int pr = tid; pr < (nD ? N * (N - 1) / 2 : 0); pr += nt) {
    int i = 0, k = pr;
    while (k >= N - 1 - i) k -= N - 1 - i++;
    k += i + 1;
    zd di[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}}, dk[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    zd cr[2][2] = {{{0.0, 0.0}, {0.0, 0.0}}, {{0.0, 0.0}, {0.0, 0.0}}};  // [x of i][y of k]
    PairDen den;
    PairD pd;
    pair_den<true>(UV + 12 * i, UV + 12 * k, den);
    for (int d = 0; d < nD; ++d) {
      const int j = dcol[d];
      const double al = pj * (tab[3 * j + 1] + 1.0), be = pj * (tab[3 * j + 2] + 1.0);
      pair_col<true>(UV + 12 * i, UV + 12 * k, PP + 12 * (i * nD + d), al, be, den, pd);
      const zd z = Einv[j * N + i];
      di[0] = di[0] - z * pd.dd[0][0];
      di[1] = di[1] - z * pd.dd[0][1];
      di[2] = di[2] - z * pd.dd[1][1];
      dk[0] = dk[0] - z * pd.dd[2][2];
      dk[1] = dk[1] - z * pd.dd[2][3];
      dk[2] = dk[2] - z * pd.dd[3][3];
      for (int x2 = 0; x2 < 2; ++x2)
        for (int y2 = 0; y2 < 2; ++y2) cr[x2][y2] = cr[x2][y2] - z * pd.dd[x2][2 + y2];
    }
    pair_den<true>(UV + 12 * k, UV + 12 * i, den);
    for (int d = 0; d < nD; ++d) {
      const int j = dcol[d];
      const double al = pj * (tab[3 * j + 1] + 1.0), be = pj * (tab[3 * j + 2] + 1.0);
      pair_col<true>(UV + 12 * k, UV + 12 * i, PP + 12 * (k * nD + d), al, be, den, pd);
      const zd z = Einv[j * N + k];
      dk[0] = dk[0] - z * pd.dd[0][0];
      dk[1] = dk[1] - z * pd.dd[0][1];
      dk[2] = dk[2] - z * pd.dd[1][1];
      di[0] = di[0] - z * pd.dd[2][2];
      di[1] = di[1] - z * pd.dd[2][3];
      di[2] = di[2] - z * pd.dd[3][3];
      for (int x2 = 0; x2 < 2; ++x2)
        for (int y2 = 0; y2 < 2; ++y2) cr[x2][y2] = cr[x2][y2] - z * pd.dd[2 + x2][y2];
    }
    for (int t = 0; t < 3; ++t) {
      S[3 * (i * N + k) + t] = di[t];
      S[3 * (k * N + i) + t] = dk[t];
    }
    for (int x2 = 0; x2 < 2; ++x2)
      for (int y2 = 0; y2 < 2; ++y2) {
        H[(2 * i + x2) * T + 2 * k + y2] = cr[x2][y2];
        H[(2 * k + y2) * T + 2 * i + x2] = cr[x2][y2];
      }
  }
  __syncthreads();
  for (int n = tid; n < (nD ? N : 0); n += nt) {
    zd t[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int k = 0; k < N; ++k) {
      if (k == n) continue;
      for (int q = 0; q < 3; ++q) t[q] = t[q] + S[3 * (n * N + k) + q];
    }
    H[(2 * n) * T + 2 * n] = t[0];
    H[(2 * n) * T + 2 * n + 1] = t[1];
    H[(2 * n + 1) * T + 2 * n] = t[1];
    H[(2 * n + 1) * T + 2 * n + 1] = t[2];
  }
  __syncthreads();
  // gradient: determinant + pairs
  for (int a = tid; a < T; a += nt) {
    const int e = a >> 1, c = a & 1;
    zd s = R[a * N + e];
    for (int d = 0; d < nD; ++d) s = s + Y[(a * nD + d) * N + dcol[d]];
    g[a] = pair_grad(s, UV, N, e, c, p2);
  }
  // Hessian
  for (int idx = tid; idx < T * T; idx += nt) {
    const int a = idx / T, bb = idx % T, ea = a >> 1, ca = a & 1, eb = bb >> 1, cb = bb & 1;
    // T2 (left in H by the pass above) - tr(W dE_a W dE_b)
    zd h = H[idx] - R[bb * N + ea] * R[a * N + eb];
    for (int d = 0; d < nD; ++d) {
      const int Ld = dcol[d];
      const zd *Ya = Y + (a * nD + d) * N, *Yb = Y + (bb * nD + d) * N;
      zd sab{0.0, 0.0}, sba{0.0, 0.0};
      for (int j = 0; j < N; ++j) {
        sab = sab + dE[ca * NN + ea * N + j] * Yb[j];
        sba = sba + dE[cb * NN + eb * N + j] * Ya[j];
      }
      h = h - sab * Einv[Ld * N + ea] - Einv[Ld * N + eb] * sba;
      for (int d2 = 0; d2 < nD; ++d2) h = h - Ya[dcol[d2]] * Y[(bb * nD + d2) * N + Ld];
    }
    if (ea == eb) {
      const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
      zd s{0.0, 0.0};
      for (int j = 0; j < N; ++j) s = s + Einv[j * N + ea] * d2E[k * NN + ea * N + j];
      h = pair_hess_same(h + s, UV, N, ea, ca, cb, p2);
    } else {
      h = pair_hess_cross(h, UV + 12 * ea, UV + 12 * eb, ca, cb, p2);
    }
    H[idx] = h;
  }
  __syncthreads();
  hamiltonian_tail(x, b, N, g, H, Q, radius, lambda, interaction, logdet, lpair, e_l, obs, tid, nt);
}

}  // namespace

size_t cf_smem_bytes(int N, int n_dense, bool energy) {
  return (size_t)csm_layout(N, n_dense, energy).total * 2 * sizeof(double);
}

void launch_cf(const Dims& d, const float* x, const int* tab, int n_dense, float* logpsi, float* e_l, float* obs,
               int nw, hipStream_t s) {
  if (e_l) {
    const size_t bytes = cf_smem_bytes(d.N, n_dense, true);
    ensure_smem(cf_kernel<true>, bytes);
    hipLaunchKernelGGL(cf_kernel<true>, dim3(nw), dim3(64), bytes, s, x, tab, logpsi, e_l, obs, d.N, (double)d.Q,
                       (double)d.r, (double)d.lambda, d.interaction);
  } else {
    const size_t bytes = cf_smem_bytes(d.N, n_dense, false);
    hipLaunchKernelGGL(cf_kernel<false>, dim3(nw), dim3(64), bytes, s, x, tab, logpsi, e_l, obs, d.N, (double)d.Q,
                       (double)d.r, (double)d.lambda, d.interaction);
  }
}

}  // namespace dh
