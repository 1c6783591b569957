// Device code shared by the parameter-free trial states (laughlin.hip, cf.hip, pfaffian.hip,
// halperin.hip, quasihole.hip): complex double, the spinor coordinates u, v and their
// derivatives, the monomial u^a v^b, the pair quotient of the LLL-projected second-level
// orbitals, the Gauss-Jordan elimination, the skew (Pfaffian) elimination and the inverse it
// gives, the species weights of a two-component state, the pair (Jastrow) part of log psi with
// its gradient and Hessian, and the kinetic / angular momentum / potential assembly from the
// gradient g and the full Hessian H of log psi.
//
// Each kernel is one 64-thread workgroup per walker with everything in LDS (halperin.hip's value
// kernel apart: several walkers per workgroup); (tid, nt) are its thread index and count.  A
// helper is compiled with the flags of the file that includes it: quasihole.hip's copy is
// uncontracted, pfaffian.hip's is not.  The helpers that replace what used to be inline kernel code are
// __forceinline__ and take their accumulator by value, so that every kernel keeps the
// expression tree (summation order, fused multiply-adds) it had with the code written out.
#pragma once
#include "dh_internal.h"
#include "device_common.h"

namespace dh {

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
__device__ __forceinline__ zd zinv(zd b) {
  const double d = b.re * b.re + b.im * b.im;
  return zd{b.re / d, -b.im / d};
}
__device__ __forceinline__ zd zpow(zd b, int e) {  // e >= 0
  zd r{1.0, 0.0};
  for (int k = 0; k < e; ++k) r = r * b;
  return r;
}

// u, v and their derivatives of electron (th, ph); the first two entries alone if !FULL
template <bool FULL>
static __device__ void uv_derivs(double th, double ph, zd* q) {
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
static __device__ void monomial(const zd* q, int a, int b, zd* val, zd* d1, zd* d2) {
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
static __device__ void pair_den(const zd* qi, const zd* qk, PairDen& D) {
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
static __device__ void pair_col(const zd* qi, const zd* qk, const zd* Pi, double al, double be, const PairDen& D, PairD& o) {
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

// Gauss-Jordan with partial pivoting (|re| + |im| pivot, as det.hip) on the N rows of E
// (leading dimension ld: 2 N for [E | I] -> [I | E^-1], N for E alone; the left block and so
// the pivots are the same).  In LDS, the caller's: fac, the pivot factors [N]; logdet (zeroed
// by the caller before its last barrier, complete after the call); piv, the pivot row of the
// current step, an int or (an int in a double is exact) a double slot beside logdet.
template <typename Piv>
__device__ __forceinline__ void gauss_jordan(zd* E, int N, int ld, zd* fac, zd* logdet, Piv* piv, int tid, int nt) {
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
      *piv = (Piv)bi;
    }
    __syncthreads();
    const int pr = (int)*piv;
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
}

// Pf(A) of a skew-symmetric A by elimination with pivoting (Parlett-Reid in 2x2 blocks): at step
// k = 0, 2, ... the largest |A[k][j]|, j > k (|re| + |im|, as det.hip), is brought to column k + 1
// by swapping row and column j with k + 1 (a factor -1), the pivot P = A[k][k+1] is multiplied
// into Pf, and the trailing block takes the rank-2 skew update
//   A[i][j] += (A[i][k] A[k+1][j] - A[i][k+1] A[k][j]) / P,   i, j >= k + 2,
// which is the row operation row_i += (A[i][k] / P) row_{k+1} - (A[i][k+1] / P) row_k alone: the
// matching column operation only clears rows k, k + 1, which are not read again.
//
// On the N rows of G (leading dimension ld: N for A alone, in place; 2 N for [A | I], to which
// the same row operations and swaps are applied: the right half becomes M with M A M^T = D, D the
// block diagonal of the pivots; the left block and so the pivots are the same).  In LDS, the
// caller's: f0, f1, the factor columns [N]; pinv (ENERGY only), 1 / pivot of step k at [k / 2];
// logpf (zeroed by the caller and G complete before its last barrier; log Pf after the call);
// pivd, the pivot column of the current step (an int in a double is exact).
template <bool ENERGY>
__device__ __forceinline__ void skew_eliminate(zd* G, int N, int ld, zd* f0, zd* f1, zd* pinv, zd* logpf, double* pivd,
                                               int tid, int nt) {
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
}

// The inverse behind the derivatives of log Pf, from [A | I] as skew_eliminate<true> leaves it
// (G, leading dimension 2 N, and pinv, complete before the call):
//   W = A^-1 = M^T D^-1 M,   W[i][j] = sum_k (M[k+1][i] M[k][j] - M[k][i] M[k+1][j]) / P_k,
// then Y[a][j] = (W d_a)[j] for the 2 N rows d_a [N] of d, a = 2 e + (0 theta | 1 phi), also
// complete before the call.  W [N][N] and Y [2 N][N] are the caller's LDS, complete after it.
__device__ __forceinline__ void pfaffian_inverse(const zd* G, int N, const zd* pinv, const zd* d, zd* W, zd* Y, int tid,
                                                 int nt) {
  const int ld = 2 * N;
  for (int idx = tid; idx < N * N; idx += nt) {
    const int i = idx / N, j = idx % N;
    zd s{0.0, 0.0};
    for (int k = 0; k < N; k += 2) {
      const zd *m0 = G + k * ld + N, *m1 = m0 + ld;
      s = s + (m1[i] * m0[j] - m0[i] * m1[j]) * pinv[k >> 1];
    }
    W[idx] = s;
  }
  __syncthreads();
  for (int idx = tid; idx < 2 * N * N; idx += nt) {
    const int a = idx / N, j = idx % N;
    zd s{0.0, 0.0};
    for (int k = 0; k < N; ++k) s = s + W[j * N + k] * d[a * N + k];
    Y[idx] = s;
  }
  __syncthreads();
}

// Weight c_ik of the pair (i, k) of a two-species state, the slots below n_up up and the rest
// down: m_up (both up), m_dn (both down), n_int (one of each)
__device__ __forceinline__ double species_weight(int i, int k, int n_up, int m_up, int m_dn, int n_int) {
  const bool iu = i < n_up, ku = k < n_up;
  return (double)(iu != ku ? n_int : iu ? m_up : m_dn);
}

// Pair part of log psi, weight sum_{i<j} log w_ij with w_ij = u_i v_j - u_j v_i, summed over
// the wave (every lane gets it).  UV: SU entries per electron, u and v first.  pi_per_pair adds
// i pi per pair: the product over ORDERED pairs of laughlin.hip has w_ji = -w_ij in it.
__device__ __forceinline__ zd pair_logpsi(const zd* UV, int SU, int N, double weight, bool pi_per_pair, int tid, int nt) {
  double lre = 0.0, lim = 0.0;
  for (int q = tid; q < N * N; q += nt) {
    const int i = q / N, j = q % N;
    if (j <= i) continue;
    const zd w = UV[SU * i] * UV[SU * j + 1] - UV[SU * j] * UV[SU * i + 1];
    lre += 0.5 * weight * log(w.re * w.re + w.im * w.im);
    lim += pi_per_pair ? weight * atan2(w.im, w.re) + M_PI : weight * atan2(w.im, w.re);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lre += __shfl_xor(lre, o, 64);
    lim += __shfl_xor(lim, o, 64);
  }
  return zd{lre, lim};
}

// The derivatives of the pair part (UV: the 12 uv_derivs entries per electron), each added to
// what the caller has so far.  Gradient entry of coordinate c (0 theta, 1 phi) of electron e:
__device__ __forceinline__ zd pair_grad(zd s, const zd* UV, int N, int e, int c, double weight) {
  const zd* qe = UV + 12 * e;
  for (int j = 0; j < N; ++j) {
    if (j == e) continue;
    const zd* qj = UV + 12 * j;
    const zd w = qe[0] * qj[1] - qj[0] * qe[1];
    const zd dw = qe[2 + c] * qj[1] - qj[0] * qe[4 + c];
    s = s + weight * zdiv(dw, w);
  }
  return s;
}
// Hessian entry of coordinates (ca, cb) of the same electron e ...
__device__ __forceinline__ zd pair_hess_same(zd h, const zd* UV, int N, int e, int ca, int cb, double weight) {
  const zd* qa = UV + 12 * e;
  const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
  for (int j = 0; j < N; ++j) {
    if (j == e) continue;
    const zd* qj = UV + 12 * j;
    const zd w = qa[0] * qj[1] - qj[0] * qa[1];
    const zd dx = qa[2 + ca] * qj[1] - qj[0] * qa[4 + ca];
    const zd dy = qa[2 + cb] * qj[1] - qj[0] * qa[4 + cb];
    const zd dxy = qa[6 + k] * qj[1] - qj[0] * qa[9 + k];
    const zd fw = zdiv(dx, w), gw = zdiv(dy, w);
    h = h + weight * (zdiv(dxy, w) - fw * gw);
  }
  return h;
}
// ... and of coordinate ca of one electron (qa) with cb of another (qb)
__device__ __forceinline__ zd pair_hess_cross(zd h, const zd* qa, const zd* qb, int ca, int cb, double weight) {
  const zd w = qa[0] * qb[1] - qb[0] * qa[1];
  const zd dx = qa[2 + ca] * qb[1] - qb[0] * qa[4 + ca];  // d/dx_a
  const zd dy = qa[0] * qb[4 + cb] - qb[2 + cb] * qa[1];  // d/dy_b
  const zd dxy = qa[2 + ca] * qb[4 + cb] - qb[2 + cb] * qa[4 + ca];
  return h + weight * (zdiv(dxy, w) - zdiv(dx, w) * zdiv(dy, w));
}

// hamiltonian.py:115-169 with g [2 N] and the full Hessian H [2 N][2 N] of log psi of walker b
// (both in LDS, complete before the call); potential (double geometry).  Writes e_l [b][2]
// and obs [b][8] = KE re, KE im, PE, Lz, Lz^2, L^2, log|psi|, arg psi, the last two from the
// two parts of log psi: ldet (determinant or Pfaffian part, in LDS) and lpair (pair part).
__device__ __forceinline__ void hamiltonian_tail(const float* x, int b, int N, const zd* g, const zd* H, double Q,
                                                 double radius, double lambda, int interaction, const zd* ldet, zd lpair,
                                                 float* e_l, float* obs, int tid, int nt) {
  const int NN = N * N, T = 2 * N;
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
    ob[6] = (float)(ldet->re + lpair.re);
    ob[7] = (float)remainder(ldet->im + lpair.im, 2.0 * M_PI);
  }
}

}  // namespace dh
