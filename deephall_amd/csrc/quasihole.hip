// Quasiholes pinned at chosen points of the sphere, on a Halperin (Laughlin) or a Moore-Read base,
// and their local energy.
//
// Hole a at (theta_a, phi_a) has the spinor (U_a, V_a) of an electron there, and
//   s_a(i) = u_i V_a - v_i U_a
// is w of electron i and the hole: zero with the electron on the hole.
//
//   Halperin base: log psi = sum_{i<k} c_ik log w_ik + sum_a sum_{i in S_a} log s_a(i)
//     c_ik = species_weight; S_a all electrons, the up slots or the down slots by the hole's kind.
//   Pfaffian base: the 2 k holes of the groups A and B, and Abelian holes acting on every electron,
//     F_i = prod_{a in A} s_a(i),  G_i = prod_{b in B} s_b(i),
//     A_ik = (F_i G_k + F_k G_i) / w_ik (i != k),  A_ii = 0,
//     log psi = log Pf(A) + 2 p sum_{i<k} log w_ik + sum_{a Abelian} sum_i log s_a(i)
//     (k = 0, Abelian holes only: A_ik = 1 / w_ik, Moore-Read's own entries).
//
// No normalisation; Im log psi is the principal phase.  Both bases are the pair part of
// halperin.hip (the Pfaffian base with all three weights 2 p), a one-body part, and for the
// Pfaffian base the skew elimination pfaffian.hip uses (skew_eliminate) on the new A.
//
// One-body part: with s_x = du_x V - dv_x U and s_xy = d2u_xy V - d2v_xy U it adds log s to
// log psi, s_x / s to g[2 i + c] and s_xy / s - s_x s_y / s^2 to the same-electron Hessian block,
// nothing to the cross blocks.
//
// Pfaffian part: the identities of pfaffian.hip's header (W = M^T D^-1 M, y_a = W d_a, the three
// Hessian terms) hold for any antisymmetric A whose entry (i, k) depends on electrons i and k
// only.  With n_ik = F_i G_k + F_k G_i the quotient rule twice, as pair_col does:
//   A_x = (n_x - A w_x) / w,   A_xy = (n_xy - A_x w_y - A_y w_x - A w_xy) / w,
//   n_xy = F_x G_y' + G_x F_y' between two electrons.
// F and G with their first and second derivatives (12 numbers per electron) are formed once, by
// the product rule over the group's holes: no division by s, an electron on a hole of a group is
// no singularity of A.
//
// One 64-lane workgroup per walker, complex double in LDS, for the value (dh_logpsi,
// dh_mcmc_step) and for the energy (dh_local_energy).  The file is compiled without contraction
// and log psi is formed by the same functions (pair_log, hole_log, the elimination on the left
// block) in both instantiations: they give the same bits.
// LDS in complex doubles: energy, Halperin base 4 N^2 + 14 N + 20; energy, Pfaffian base
// 11 N^2 + 29 N + 20 (N <= 28 in 160 KiB); value 2 N + 20 and N^2 + 6 N + 20.
//
// hole_logs_kernel (dh_hole_logs) is the value kernel over a table of hole configurations on the
// same walkers, its result kept in double: the input of the overlap matrix of holes.hip.
#include "trial_common.h"

namespace dh {
namespace {

constexpr int kMaxHoles = DH_QUASIHOLE_MAX_HOLES;

// LDS layout in zd units
struct QSm {
  int uv, hole, kind, lp, fg, G, misc, W, d, y, g, H, total;
};
__host__ __device__ inline QSm qsm_layout(int N, bool pf, bool energy) {
  QSm L{};
  int o = 0;
  L.uv = o;  // energy: u, v, du[2], dv[2], d2u[3], d2v[3] = 12 per electron
  o += (energy ? 12 : 2) * N;
  L.hole = o;  // U, V per hole
  o += 2 * kMaxHoles;
  L.kind = o;  // the holes' kinds: kMaxHoles ints
  o += (kMaxHoles * (int)sizeof(int) + (int)sizeof(zd) - 1) / (int)sizeof(zd);
  L.lp = o;  // log Pf (zero on the Halperin base), the pivot column of the current step
  o += 2;
  if (pf) {
    L.fg = o;  // F and G of each electron; energy: value, d/dth, d/dph, d2 tt, tp, pp of each
    o += (energy ? 12 : 2) * N;
    L.G = o;  // A; energy: augmented [A | I] -> [. | M]
    o += (energy ? 2 : 1) * N * N;
    L.misc = o;  // factor columns f0 [N], f1 [N], (energy) 1 / pivot [N]
    o += (energy ? 3 : 2) * N;
    if (energy) {
      L.W = o;
      o += N * N;
      L.d = o;  // d[a][k] = dA_{n(a) k} / dx_a
      o += 2 * N * N;
      L.y = o;  // y[a][j] = (W d_a)[j]
      o += 2 * N * N;
    }
  }
  if (energy) {
    L.g = o;
    o += 2 * N;
    L.H = o;
    o += 4 * N * N;
  }
  L.total = o;
  return L;
}

// does a hole of this kind act on electron i through the one-body part?
__device__ __forceinline__ bool hole_acts(int kind, int i, int n_up) {
  return kind == DH_HOLE_BOTH || (kind == DH_HOLE_UP && i < n_up) || (kind == DH_HOLE_DOWN && i >= n_up);
}

// sum_{i<k} c_ik log w_ik over the wave (every lane gets it).  UV: SU entries per electron.
__device__ __forceinline__ zd pair_log(const zd* UV, int SU, int N, int n_up, int m_up, int m_dn, int n_int, int tid) {
  double lre = 0.0, lim = 0.0;
  for (int q = tid; q < N * N; q += 64) {
    const int i = q / N, k = q % N;
    if (k <= i) continue;
    const double c = species_weight(i, k, n_up, m_up, m_dn, n_int);
    if (c == 0.0) continue;  // an up and a down electron may coincide at n = 0
    const zd w = UV[SU * i] * UV[SU * k + 1] - UV[SU * k] * UV[SU * i + 1];
    lre += (0.5 * c) * log(w.re * w.re + w.im * w.im);
    lim += c * atan2(w.im, w.re);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lre += __shfl_xor(lre, o, 64);
    lim += __shfl_xor(lim, o, 64);
  }
  return zd{lre, lim};
}

// sum_a sum_{i in S_a} log s_a(i) over the wave (every lane gets it)
__device__ __forceinline__ zd hole_log(const zd* UV, int SU, int N, int n_up, const zd* HU, const int* kind, int nh,
                                       int tid) {
  double lre = 0.0, lim = 0.0;
  for (int q = tid; q < N * nh; q += 64) {
    const int i = q / nh, a = q % nh;
    if (!hole_acts(kind[a], i, n_up)) continue;
    const zd s = UV[SU * i] * HU[2 * a + 1] - UV[SU * i + 1] * HU[2 * a];
    lre += 0.5 * log(s.re * s.re + s.im * s.im);
    lim += atan2(s.im, s.re);
  }
  for (int o = 32; o > 0; o >>= 1) {
    lre += __shfl_xor(lre, o, 64);
    lim += __shfl_xor(lim, o, 64);
  }
  return zd{lre, lim};
}

// The one-body part's derivatives of electron qe (its 12 uv_derivs entries), each added to what
// the caller has so far: gradient entry of coordinate c ...
__device__ __forceinline__ zd hole_grad(zd s, const zd* qe, int e, int c, int n_up, const zd* HU, const int* kind,
                                        int nh) {
  for (int a = 0; a < nh; ++a) {
    if (!hole_acts(kind[a], e, n_up)) continue;
    const zd U = HU[2 * a], V = HU[2 * a + 1];
    s = s + zdiv(qe[2 + c] * V - qe[4 + c] * U, qe[0] * V - qe[1] * U);
  }
  return s;
}
// ... and Hessian entry of coordinates (ca, cb)
__device__ __forceinline__ zd hole_hess(zd h, const zd* qe, int e, int ca, int cb, int n_up, const zd* HU,
                                        const int* kind, int nh) {
  const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
  for (int a = 0; a < nh; ++a) {
    if (!hole_acts(kind[a], e, n_up)) continue;
    const zd U = HU[2 * a], V = HU[2 * a + 1];
    const zd sv = qe[0] * V - qe[1] * U;
    const zd fx = zdiv(qe[2 + ca] * V - qe[4 + ca] * U, sv), fy = zdiv(qe[2 + cb] * V - qe[4 + cb] * U, sv);
    h = h + (zdiv(qe[6 + k] * V - qe[9 + k] * U, sv) - fx * fy);
  }
  return h;
}

// P = prod s_a(i) over the holes of one group with (FULL) its first and second derivatives, by
// the product rule: out = value (, d/dth, d/dph, d2 tt, tp, pp).  The value is formed by the
// same products in both instantiations.  init: the empty product, 1 (G of a state without groups
// starts at 1/2: its numerator F_i G_k + F_k G_i is then 1, the entries are Moore-Read's 1 / w).
template <bool FULL>
__device__ __forceinline__ void group_product(const zd* q, const zd* HU, const int* kind, int nh, int group,
                                              double init, zd* out) {
  zd P{init, 0.0}, Px[2] = {zd{0.0, 0.0}, zd{0.0, 0.0}}, Pxy[3] = {zd{0.0, 0.0}, zd{0.0, 0.0}, zd{0.0, 0.0}};
  for (int a = 0; a < nh; ++a) {
    if (kind[a] != group) continue;
    const zd U = HU[2 * a], V = HU[2 * a + 1];
    const zd s = q[0] * V - q[1] * U;
    if (FULL) {
      const zd sx[2] = {q[2] * V - q[4] * U, q[3] * V - q[5] * U};
      const zd sxy[3] = {q[6] * V - q[9] * U, q[7] * V - q[10] * U, q[8] * V - q[11] * U};
      Pxy[0] = Pxy[0] * s + 2.0 * (Px[0] * sx[0]) + P * sxy[0];
      Pxy[1] = Pxy[1] * s + Px[0] * sx[1] + Px[1] * sx[0] + P * sxy[1];
      Pxy[2] = Pxy[2] * s + 2.0 * (Px[1] * sx[1]) + P * sxy[2];
      Px[0] = Px[0] * s + P * sx[0];
      Px[1] = Px[1] * s + P * sx[1];
    }
    P = P * s;
  }
  out[0] = P;
  if (!FULL) return;
  out[1] = Px[0];
  out[2] = Px[1];
  out[3] = Pxy[0];
  out[4] = Pxy[1];
  out[5] = Pxy[2];
}

template <bool PF, bool ENERGY>
__global__ __launch_bounds__(64) void quasihole_kernel(const float* __restrict__ x, float* __restrict__ out_lp,
                                                       float* __restrict__ e_l, float* __restrict__ obs, int N,
                                                       int n_up, QuasiholeState qs, double Q, double radius,
                                                       double lambda, int interaction) {
  extern __shared__ double smd[];
  zd* sm = reinterpret_cast<zd*>(smd);
  const QSm L = qsm_layout(N, PF, ENERGY);
  constexpr int SU = ENERGY ? 12 : 2;  // entries per electron of UV, and of FG
  zd *UV = sm + L.uv, *HU = sm + L.hole, *logpf = sm + L.lp;
  int* kind = reinterpret_cast<int*>(sm + L.kind);
  double* pivd = &logpf[1].re;  // the pivot column of the current step
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int NN = N * N, T = 2 * N, n_dn = N - n_up, nh = qs.n_holes;
  const int m_up = qs.m_up, m_dn = qs.m_dn, n_int = qs.n_int;
  for (int i = tid; i < N; i += nt)
    uv_derivs<ENERGY>((double)x[2 * ((size_t)b * N + i)], (double)x[2 * ((size_t)b * N + i) + 1], UV + SU * i);
  // the holes into LDS, lane a hole a (unrolled: constant indices into the by-value argument)
#pragma unroll
  for (int a = 0; a < kMaxHoles; ++a)
    if (tid == a) {
      const bool on = a < nh;
      HU[2 * a] = on ? zd{qs.uv[a][0], qs.uv[a][1]} : zd{0.0, 0.0};
      HU[2 * a + 1] = on ? zd{qs.uv[a][2], qs.uv[a][3]} : zd{0.0, 0.0};
      kind[a] = on ? qs.kind[a] : -1;
    }
  if (tid == 0) *logpf = zd{0.0, 0.0};
  __syncthreads();
  if (PF) {
    zd *FG = sm + L.fg, *G = sm + L.G, *f0 = sm + L.misc, *f1 = f0 + N, *pinv = f1 + N;  // pinv: energy only
    const int ld = ENERGY ? 2 * N : N;
    bool grouped = false;
    for (int a = 0; a < nh; ++a) grouped = grouped || kind[a] == DH_HOLE_GROUP_A;
    for (int idx = tid; idx < 2 * N; idx += nt) {
      const int i = idx >> 1, grp = idx & 1;
      group_product<ENERGY>(UV + SU * i, HU, kind, nh, grp ? DH_HOLE_GROUP_B : DH_HOLE_GROUP_A,
                            grp && !grouped ? 0.5 : 1.0, FG + SU * i + (ENERGY ? 6 : 1) * grp);
    }
    __syncthreads();
    constexpr int GO = ENERGY ? 6 : 1;  // G's offset in an electron's FG entries
    // A (augmented with I) and, for the energy, d[a][k] = A_x of the pair (n(a), k)
    for (int idx = tid; idx < NN; idx += nt) {
      const int i = idx / N, k = idx % N;
      const zd *qi = UV + SU * i, *qk = UV + SU * k, *Fi = FG + SU * i, *Fk = FG + SU * k;
      zd a{0.0, 0.0}, wi{0.0, 0.0};
      if (i != k) {
        wi = zinv(qi[0] * qk[1] - qk[0] * qi[1]);
        a = (Fi[0] * Fk[GO] + Fk[0] * Fi[GO]) * wi;
      }
      G[i * ld + k] = a;
      if (ENERGY) {
        G[i * ld + N + k] = zd{i == k ? 1.0 : 0.0, 0.0};
        zd* d = sm + L.d;
        for (int c = 0; c < 2; ++c) {
          const zd wx = qi[2 + c] * qk[1] - qk[0] * qi[4 + c];
          const zd nx = Fi[1 + c] * Fk[GO] + Fk[0] * Fi[GO + 1 + c];
          d[(2 * i + c) * N + k] = i == k ? zd{0.0, 0.0} : (nx - a * wx) * wi;
        }
      }
    }
    __syncthreads();
    // on [A | I], or on A alone for the value, as pfaffian.hip: the left block and so the pivots
    // are the same
    skew_eliminate<ENERGY>(G, N, ld, f0, f1, pinv, logpf, pivd, tid, nt);
  }
  // pair and one-body parts of log psi
  const zd lrest = pair_log(UV, SU, N, n_up, m_up, m_dn, n_int, tid) + hole_log(UV, SU, N, n_up, HU, kind, nh, tid);
  if (!ENERGY) {
    if (tid == 0) {
      out_lp[2 * (size_t)b] = (float)(logpf->re + lrest.re);
      out_lp[2 * (size_t)b + 1] = (float)remainder(logpf->im + lrest.im, 2.0 * M_PI);
    }
    return;
  }
  zd *g = sm + L.g, *H = sm + L.H;
  zd *FG = sm + L.fg, *W = sm + L.W, *d = sm + L.d, *Y = sm + L.y;  // Pfaffian base only
  // W = M^T D^-1 M and y[a][j] = (W d_a)[j],  a = 2 e + (0 theta | 1 phi)
  if (PF) pfaffian_inverse(sm + L.G, N, sm + L.misc + 2 * N /* 1 / pivot */, d, W, Y, tid, nt);
  // gradient: Pfaffian, then pairs (the up partners, the down partners), then holes
  for (int a = tid; a < T; a += nt) {
    const int e = a >> 1, c = a & 1;
    const double wu = species_weight(e, 0, n_up, m_up, m_dn, n_int), wd = species_weight(e, N - 1, n_up, m_up, m_dn, n_int);
    zd s{0.0, 0.0};
    if (PF) s = s - Y[a * N + e];
    if (n_up > 0 && wu != 0.0) s = pair_grad(s, UV, n_up, e, c, wu);
    if (n_dn > 0 && wd != 0.0) s = pair_grad(s, UV + 12 * n_up, n_dn, e - n_up, c, wd);
    g[a] = hole_grad(s, UV + 12 * e, e, c, n_up, HU, kind, nh);
  }
  // Hessian
  for (int idx = tid; idx < T * T; idx += nt) {
    const int a = idx / T, bb = idx % T, ea = a >> 1, ca = a & 1, eb = bb >> 1, cb = bb & 1;
    const zd *qa = UV + 12 * ea, *qb = UV + 12 * eb;
    zd h{0.0, 0.0};
    if (PF) h = h - Y[a * N + eb] * Y[bb * N + ea];
    if (ea == eb) {
      const double wu = species_weight(ea, 0, n_up, m_up, m_dn, n_int), wd = species_weight(ea, N - 1, n_up, m_up, m_dn, n_int);
      if (n_up > 0 && wu != 0.0) h = pair_hess_same(h, UV, n_up, ea, ca, cb, wu);
      if (n_dn > 0 && wd != 0.0) h = pair_hess_same(h, UV + 12 * n_up, n_dn, ea - n_up, ca, cb, wd);
      h = hole_hess(h, qa, ea, ca, cb, n_up, HU, kind, nh);
      if (PF) {  // 1/2 tr(W d2A) = sum_j W[j][n] A_xy of the pair (n, j)
        const int k = ca + cb;  // 0 tt, 1 tp, 2 pp
        const zd* Fa = FG + 12 * ea;
        for (int j = 0; j < N; ++j) {
          if (j == ea) continue;
          const zd *qj = UV + 12 * j, *Fj = FG + 12 * j;
          const zd wi = zinv(qa[0] * qj[1] - qj[0] * qa[1]);
          const zd wx = qa[2 + ca] * qj[1] - qj[0] * qa[4 + ca], wy = qa[2 + cb] * qj[1] - qj[0] * qa[4 + cb];
          const zd wxy = qa[6 + k] * qj[1] - qj[0] * qa[9 + k];
          const zd A = (Fa[0] * Fj[6] + Fj[0] * Fa[6]) * wi;
          const zd Ax = (Fa[1 + ca] * Fj[6] + Fj[0] * Fa[7 + ca] - A * wx) * wi;
          const zd Ay = (Fa[1 + cb] * Fj[6] + Fj[0] * Fa[7 + cb] - A * wy) * wi;
          const zd nxy = Fa[3 + k] * Fj[6] + Fj[0] * Fa[9 + k];
          h = h + W[j * N + ea] * ((nxy - Ax * wy - Ay * wx - A * wxy) * wi);
        }
      }
    } else {
      const double w = species_weight(ea, eb, n_up, m_up, m_dn, n_int);
      if (w != 0.0) h = pair_hess_cross(h, qa, qb, ca, cb, w);
      if (PF) {  // x = coordinate ca of electron ea, y = coordinate cb of electron eb
        const zd *Fa = FG + 12 * ea, *Fb = FG + 12 * eb;
        const zd wi = zinv(qa[0] * qb[1] - qb[0] * qa[1]);
        const zd wx = qa[2 + ca] * qb[1] - qb[0] * qa[4 + ca], wy = qa[0] * qb[4 + cb] - qb[2 + cb] * qa[1];
        const zd wxy = qa[2 + ca] * qb[4 + cb] - qb[2 + cb] * qa[4 + ca];
        const zd A = (Fa[0] * Fb[6] + Fb[0] * Fa[6]) * wi;
        const zd Ax = (Fa[1 + ca] * Fb[6] + Fb[0] * Fa[7 + ca] - A * wx) * wi;
        const zd Ay = (Fa[0] * Fb[7 + cb] + Fb[1 + cb] * Fa[6] - A * wy) * wi;
        const zd nxy = Fa[1 + ca] * Fb[7 + cb] + Fb[1 + cb] * Fa[7 + ca];
        zd dy{0.0, 0.0};
        for (int j = 0; j < N; ++j) dy = dy + d[a * N + j] * Y[bb * N + j];
        h = h + W[eb * N + ea] * (dy + (nxy - Ax * wy - Ay * wx - A * wxy) * wi);
      }
    }
    H[idx] = h;
  }
  __syncthreads();
  hamiltonian_tail(x, b, N, g, H, Q, radius, lambda, interaction, logpf, lrest, e_l, obs, tid, nt);
}

// log psi_c of one walker for the K hole configurations of a table (dh_hole_logs), complex double.
// The value layout of quasihole_kernel<PF, false> and its functions, so that out[b][c] rounded to
// float32 is dh_logpsi of a handle with configuration c, bit for bit: the electrons' spinors and
// the pair part are formed once per walker, the holes of configuration c then take the place of
// the by-value argument in HU and kind, and on the Pfaffian base A is rebuilt in the same LDS and
// eliminated once per configuration.  uv [K][kMaxHoles][4] and knd [K][kMaxHoles] are the device
// table; every bound (N, nh, K) is a host-checked argument, none is read from the table.
template <bool PF>
__global__ __launch_bounds__(64) void hole_logs_kernel(const float* __restrict__ x, const double* __restrict__ uv,
                                                       const int* __restrict__ knd, double* __restrict__ out, int N,
                                                       int n_up, int m_up, int m_dn, int n_int, int nh, int K) {
  extern __shared__ double smd[];
  zd* sm = reinterpret_cast<zd*>(smd);
  const QSm L = qsm_layout(N, PF, false);
  constexpr int SU = 2;
  zd *UV = sm + L.uv, *HU = sm + L.hole, *logpf = sm + L.lp;
  int* kind = reinterpret_cast<int*>(sm + L.kind);
  double* pivd = &logpf[1].re;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < N; i += nt)
    uv_derivs<false>((double)x[2 * ((size_t)b * N + i)], (double)x[2 * ((size_t)b * N + i) + 1], UV + SU * i);
  __syncthreads();
  const zd lpair = pair_log(UV, SU, N, n_up, m_up, m_dn, n_int, tid);
  for (int c = 0; c < K; ++c) {
    __syncthreads();  // configuration c - 1 has been read
    if (tid < kMaxHoles) {
      const bool on = tid < nh;
      const double* h = uv + 4 * ((size_t)c * kMaxHoles + tid);
      HU[2 * tid] = on ? zd{h[0], h[1]} : zd{0.0, 0.0};
      HU[2 * tid + 1] = on ? zd{h[2], h[3]} : zd{0.0, 0.0};
      kind[tid] = on ? knd[c * kMaxHoles + tid] : -1;
    }
    if (tid == 0) *logpf = zd{0.0, 0.0};
    __syncthreads();
    if (PF) {
      zd *FG = sm + L.fg, *G = sm + L.G, *f0 = sm + L.misc, *f1 = f0 + N;
      bool grouped = false;
      for (int a = 0; a < nh; ++a) grouped = grouped || kind[a] == DH_HOLE_GROUP_A;
      for (int idx = tid; idx < 2 * N; idx += nt) {
        const int i = idx >> 1, grp = idx & 1;
        group_product<false>(UV + SU * i, HU, kind, nh, grp ? DH_HOLE_GROUP_B : DH_HOLE_GROUP_A,
                             grp && !grouped ? 0.5 : 1.0, FG + SU * i + grp);
      }
      __syncthreads();
      for (int idx = tid; idx < N * N; idx += nt) {
        const int i = idx / N, k = idx % N;
        const zd *qi = UV + SU * i, *qk = UV + SU * k, *Fi = FG + SU * i, *Fk = FG + SU * k;
        zd a{0.0, 0.0};
        if (i != k) a = (Fi[0] * Fk[1] + Fk[0] * Fi[1]) * zinv(qi[0] * qk[1] - qk[0] * qi[1]);
        G[i * N + k] = a;
      }
      __syncthreads();
      skew_eliminate<false>(G, N, N, f0, f1, nullptr, logpf, pivd, tid, nt);
    }
    const zd lrest = lpair + hole_log(UV, SU, N, n_up, HU, kind, nh, tid);
    if (tid == 0) {
      double* o = out + 2 * ((size_t)b * K + c);
      o[0] = logpf->re + lrest.re;
      o[1] = remainder(logpf->im + lrest.im, 2.0 * M_PI);
    }
  }
}

template <bool PF>
void launch_quasihole_b(const Dims& d, const float* x, const QuasiholeState& q, float* logpsi, float* e_l, float* obs,
                        int nw, hipStream_t s) {
  if (e_l) {
    const size_t bytes = quasihole_smem_bytes(d.N, PF, true);
    ensure_smem(quasihole_kernel<PF, true>, bytes);
    hipLaunchKernelGGL((quasihole_kernel<PF, true>), dim3(nw), dim3(64), bytes, s, x, logpsi, e_l, obs, d.N, d.n_up, q,
                       (double)d.Q, (double)d.r, (double)d.lambda, d.interaction);
  } else {
    const size_t bytes = quasihole_smem_bytes(d.N, PF, false);
    hipLaunchKernelGGL((quasihole_kernel<PF, false>), dim3(nw), dim3(64), bytes, s, x, logpsi, e_l, obs, d.N, d.n_up, q,
                       (double)d.Q, (double)d.r, (double)d.lambda, d.interaction);
  }
}

}  // namespace

size_t quasihole_smem_bytes(int N, bool pfaffian, bool energy) {
  return (size_t)qsm_layout(N, pfaffian, energy).total * 2 * sizeof(double);
}

void launch_quasihole(const Dims& d, const float* x, const QuasiholeState& q, float* logpsi, float* e_l, float* obs,
                      int nw, hipStream_t s) {
  if (q.pfaffian)
    launch_quasihole_b<true>(d, x, q, logpsi, e_l, obs, nw, s);
  else
    launch_quasihole_b<false>(d, x, q, logpsi, e_l, obs, nw, s);
}

void launch_hole_logs(const float* x, int B, int N, int n_up, const QuasiholeState& base, int K, const void* table,
                      double* out, hipStream_t s) {
  const double* uv = static_cast<const double*>(table);
  const int* knd = reinterpret_cast<const int*>(uv + (size_t)DH_HOLE_MAX_CONFIGS * kMaxHoles * 4);
  const size_t bytes = quasihole_smem_bytes(N, base.pfaffian, false);  // at most 20 KiB (N = 32)
  if (base.pfaffian)
    hipLaunchKernelGGL(hole_logs_kernel<true>, dim3(B), dim3(64), bytes, s, x, uv, knd, out, N, n_up, base.m_up,
                       base.m_dn, base.n_int, base.n_holes, K);
  else
    hipLaunchKernelGGL(hole_logs_kernel<false>, dim3(B), dim3(64), bytes, s, x, uv, knd, out, N, n_up, base.m_up,
                       base.m_dn, base.n_int, base.n_holes, K);
}

}  // namespace dh
