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
__device__ __forceinline__ zd zdiv(zd a, zd b) {
  const double d = b.re * b.re + b.im * b.im;
  return zd{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
__device__ __forceinline__ zd zpow(zd b, int e) {  // e >= 0
  zd r{1.0, 0.0};
  for (int k = 0; k < e; ++k) r = r * b;
  return r;
}

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
  q[2] = -0.5 * sh * eu;              // du/dth
  q[3] = 0.5 * (I * u);               // du/dph
  q[4] = 0.5 * ch * ev;               // dv/dth
  q[5] = -0.5 * (I * v);              // dv/dph
  q[6] = -0.25 * u;                   // d2u/dth2
  q[7] = 0.5 * (I * q[2]);            // d2u/dth dph
  q[8] = -0.25 * u;                   // d2u/dph2
  q[9] = -0.25 * v;                   // d2v/dth2
  q[10] = -0.5 * (I * q[4]);          // d2v/dth dph
  q[11] = -0.25 * v;                  // d2v/dph2
}

// d/dx and d2/dxdy of u^a v^b (x, y in {th, ph}; xy index 0 tt, 1 tp, 2 pp)
__device__ void monomial(const zd* q, int a, int b, zd* val, zd* d1, zd* d2) {
  const zd u = q[0], v = q[1];
  const zd ua = zpow(u, a), vb = zpow(v, b);
  const zd ua1 = a >= 1 ? zpow(u, a - 1) : zd{0, 0}, vb1 = b >= 1 ? zpow(v, b - 1) : zd{0, 0};
  const zd ua2 = a >= 2 ? zpow(u, a - 2) : zd{0, 0}, vb2 = b >= 2 ? zpow(v, b - 2) : zd{0, 0};
  *val = ua * vb;
  const zd du[2] = {q[2], q[3]}, dv[2] = {q[4], q[5]};
  for (int x = 0; x < 2; ++x) d1[x] = (double)a * (ua1 * vb * du[x]) + (double)b * (ua * vb1 * dv[x]);
  const int xs[3] = {0, 0, 1}, ys[3] = {0, 1, 1};
  for (int k = 0; k < 3; ++k) {
    const int x = xs[k], y = ys[k];
    const zd d2u = q[6 + k], d2v = q[9 + k];
    d2[k] = (double)(a * (a - 1)) * (ua2 * vb * du[x] * du[y]) + (double)a * (ua1 * vb * d2u) +
            (double)(a * b) * (ua1 * vb1 * (du[x] * dv[y] + du[y] * dv[x])) + (double)(b * (b - 1)) * (ua * vb2 * dv[x] * dv[y]) +
            (double)b * (ua * vb1 * d2v);
  }
}

// The denominator e = u_i v_k - u_k v_i of a pair and its derivatives in the coordinates
// (0 th_i, 1 ph_i, 2 th_k, 3 ph_k): the same for every column, so once per pair.
struct PairDen {
  zd einv, ea[4], eab[4][4];
};
__device__ __forceinline__ zd pair_du(const zd* qi, const zd* qk, int a) { return a < 2 ? qi[2 + a] : qk[a]; }
__device__ __forceinline__ zd pair_dv(const zd* qi, const zd* qk, int a) { return a < 2 ? qi[4 + a] : qk[2 + a]; }
template <bool SECOND>
__device__ void pair_den(const zd* qi, const zd* qk, PairDen& D) {
  const zd ui = qi[0], vi = qi[1], uk = qk[0], vk = qk[1];
  D.einv = zdiv(zd{1.0, 0.0}, ui * vk - uk * vi);
  for (int a = 0; a < 4; ++a)
    D.ea[a] = a < 2 ? pair_du(qi, qk, a) * vk - uk * pair_dv(qi, qk, a) : ui * pair_dv(qi, qk, a) - pair_du(qi, qk, a) * vi;
  if (!SECOND) return;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b) {
      zd eab;
      if (b < 2) {  // both on electron i
        const int k = a + b;  // 0 tt, 1 tp, 2 pp
        eab = qi[6 + k] * vk - uk * qi[9 + k];
      } else if (a >= 2) {  // both on electron k
        const int k = (a - 2) + (b - 2);
        eab = ui * qk[9 + k] - qk[6 + k] * vi;
      } else {  // a on i, b on k
        eab = pair_du(qi, qk, a) * pair_dv(qi, qk, b) - pair_du(qi, qk, b) * pair_dv(qi, qk, a);
      }
      D.eab[a][b] = eab;
      D.eab[b][a] = eab;
    }
}

// h = (al P1_i u_k + be P2_i v_k) / e of one column and its first / second derivatives.
// Pi: P1 (0..5) and P2 (6..11) of electron i as value, d/dth, d/dph, d2 tt, tp, pp.  The
// numerator is bilinear in (P1, P2) of i and (u, v) of k; h_a = (n_a - h e_a) / e and
// h_ab = (n_ab - h_a e_b - h_b e_a - h e_ab) / e (the quotient rule twice).
struct PairD {
  zd h, d[4], dd[4][4];
};
template <bool SECOND>
__device__ void pair_col(const zd* qi, const zd* qk, const zd* Pi, double al, double be, const PairDen& D, PairD& o) {
  const zd uk = qk[0], vk = qk[1];
  const zd P1 = Pi[0], P2 = Pi[6];
  o.h = (al * (P1 * uk) + be * (P2 * vk)) * D.einv;
  for (int a = 0; a < 4; ++a) {
    const zd na = a < 2 ? al * (Pi[1 + a] * uk) + be * (Pi[7 + a] * vk)
                        : al * (P1 * pair_du(qi, qk, a)) + be * (P2 * pair_dv(qi, qk, a));
    o.d[a] = (na - o.h * D.ea[a]) * D.einv;
  }
  if (!SECOND) return;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b) {
      zd nab;
      if (b < 2) {
        const int k = a + b;
        nab = al * (Pi[3 + k] * uk) + be * (Pi[9 + k] * vk);
      } else if (a >= 2) {
        const int k = (a - 2) + (b - 2);
        nab = al * (P1 * qk[6 + k]) + be * (P2 * qk[9 + k]);
      } else {
        nab = al * (Pi[1 + a] * pair_du(qi, qk, b)) + be * (Pi[7 + a] * pair_dv(qi, qk, b));
      }
      const zd hab = (nab - o.d[a] * D.ea[b] - o.d[b] * D.ea[a] - o.h * D.eab[a][b]) * D.einv;
      o.dd[a][b] = hab;
      o.dd[b][a] = hab;
    }
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
  zd* logdet = fac + N;       // one entry
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
  // Gauss-Jordan with partial pivoting (|re| + |im| pivot, as det.hip) on [E | I], or on E
  // alone for the value: the left block and so the pivots are the same
  for (int p = 0; p < N; ++p) {
    if (tid == 0) {
      double best = -1.0;
      int bi = p;
      for (int r = p; r < N; ++r) {
        const double v = fabs(E[r * ld + p].re) + fabs(E[r * ld + p].im);
        if (v > best) {
          best = v;
          bi = r;
        }
      }
      *pivd = (double)bi;
    }
    __syncthreads();
    const int pr = (int)*pivd;
    if (pr != p)
      for (int c = tid; c < ld; c += nt) {
        const zd t = E[p * ld + c];
        E[p * ld + c] = E[pr * ld + c];
        E[pr * ld + c] = t;
      }
    __syncthreads();
    const zd P = E[p * ld + p];
    if (tid == 0) {
      logdet->re += 0.5 * log(P.re * P.re + P.im * P.im);
      logdet->im += atan2(P.im, P.re) + (pr != p ? M_PI : 0.0);
    }
    const zd Pinv = zdiv(zd{1.0, 0.0}, P);
    __syncthreads();
    for (int r = tid; r < N; r += nt) fac[r] = (r == p) ? zd{0.0, 0.0} : E[r * ld + p];
    for (int c = tid; c < ld; c += nt) E[p * ld + c] = E[p * ld + c] * Pinv;
    __syncthreads();
    for (int idx = tid; idx < N * ld; idx += nt) {
      const int r = idx / ld, c = idx % ld;
      if (r == p) continue;
      E[r * ld + c] = E[r * ld + c] - fac[r] * E[p * ld + c];
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
      out_lp[2 * b] = (float)(logdet->re + lre);
      out_lp[2 * b + 1] = (float)remainder(logdet->im + lim, 2.0 * M_PI);
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
    const zd* qe = UV + 12 * e;
    for (int j = 0; j < N; ++j) {
      if (j == e) continue;
      const zd* qj = UV + 12 * j;
      const zd w = qe[0] * qj[1] - qj[0] * qe[1];
      const zd dw = qe[2 + c] * qj[1] - qj[0] * qe[4 + c];
      s = s + p2 * zdiv(dw, w);
    }
    g[a] = s;
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
    const zd* qa = UV + 12 * ea;
    if (ea == eb) {
      const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
      zd s{0.0, 0.0};
      for (int j = 0; j < N; ++j) s = s + Einv[j * N + ea] * d2E[k * NN + ea * N + j];
      h = h + s;
      for (int j = 0; j < N; ++j) {
        if (j == ea) continue;
        const zd* qj = UV + 12 * j;
        const zd w = qa[0] * qj[1] - qj[0] * qa[1];
        const zd dx = qa[2 + ca] * qj[1] - qj[0] * qa[4 + ca];
        const zd dy = qa[2 + cb] * qj[1] - qj[0] * qa[4 + cb];
        const zd dxy = qa[6 + k] * qj[1] - qj[0] * qa[9 + k];
        const zd fw = zdiv(dx, w), gw = zdiv(dy, w);
        h = h + p2 * (zdiv(dxy, w) - fw * gw);
      }
    } else {
      const zd* qb = UV + 12 * eb;
      const zd w = qa[0] * qb[1] - qb[0] * qa[1];
      const zd dx = qa[2 + ca] * qb[1] - qb[0] * qa[4 + ca];  // d/dx_a
      const zd dy = qa[0] * qb[4 + cb] - qb[2 + cb] * qa[1];  // d/dy_b
      const zd dxy = qa[2 + ca] * qb[4 + cb] - qb[2 + cb] * qa[4 + ca];
      h = h + p2 * (zdiv(dxy, w) - zdiv(dx, w) * zdiv(dy, w));
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
    ob[6] = (float)(logdet->re + lre);
    ob[7] = (float)remainder(logdet->im + lim, 2.0 * M_PI);
  }
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
