// Halperin (m_up, m_dn, n) two-component states, and their local energy.
//
//   log psi = sum_{i<k} c_ik log w_ik,   w_ik = u_i v_k - u_k v_i,
//   c_ik = m_up (both up), m_dn (both down), n (one of each),
//   u = cos(theta/2) e^(i phi/2),  v = sin(theta/2) e^(-i phi/2)
//
// with the slots below n_up up and the rest down: (3,3,2) the singlet at 2/5, (1,1,0) two filled
// lowest Landau levels, (1,1,1) the quantum Hall ferromagnet.  An up electron has degree
// m_up (n_up - 1) + n n_dn in (u, v), a down electron m_dn (n_dn - 1) + n n_up: both are the
// flux.  No determinant and no normalisation; the sum runs over i < k as in cf.hip and
// pfaffian.hip, and Im log psi is the principal phase.
//
// The whole state is a pair part, so its derivatives are those of trial_common.h's pair helpers
// with one weight per species block: pair_grad and pair_hess_same are called once per species
// range (a range whose weight is 0 is skipped: at n = 0 an up and a down electron may coincide,
// and 0 x (1 / w) must not reach the sum), pair_hess_cross with the weight of its pair.  The full
// complex Hessian of log psi goes to hamiltonian_tail exactly as in the other three kernels.
//
// log psi itself is formed by halperin_logpsi in both instantiations: a group of G lanes
// (16, 32 or 64 by N: halperin_group) walks the pairs with stride G and adds its partials by xor
// shuffles inside the group, compiled without contraction, so that the value-only instantiation
// and the energy instantiation give the same bits whatever surrounds the call.
//
//   value (dh_logpsi, dh_mcmc_step): 256-thread workgroups, one walker per group of G lanes
//     (16, 8 or 4 walkers per workgroup), u and v in LDS: 32 N bytes per walker.  There is no
//     elimination to spread over a wave, only N (N - 1) / 2 pair terms: 15 at N = 6.
//   energy (dh_local_energy): one 64-lane workgroup per walker as laughlin.hip, cf.hip and
//     pfaffian.hip, which hamiltonian_tail's wave-wide reductions need; the 4 N^2 Hessian entries
//     fill the wave from N = 4 on.  LDS: 16 (4 N^2 + 14 N + 1) bytes (u, v and their derivatives,
//     g, H, one zero for the absent determinant part); group 0 of the wave forms log psi.
#include "trial_common.h"

namespace dh {
namespace {

constexpr int kValueNT = 256;  // threads of a value workgroup

// sum_{i<k} c_ik log w_ik of one walker by the G lanes of its group (lane = index in the group;
// a lane with live == false adds nothing but takes part in the shuffles); every lane of the
// group gets the sum.  UV: SU entries per electron, u and v first.  Every product and sum is
// rounded on its own (no contraction): the result does not depend on the caller's other code.
template <int G>
__device__ __forceinline__ zd halperin_logpsi(const zd* UV, int SU, int N, int n_up, int m_up, int m_dn, int n_int,
                                              int lane, bool live) {
#pragma clang fp contract(off)
  double lre = 0.0, lim = 0.0;
  for (int q = live ? lane : N * N; q < N * N; q += G) {
    const int i = q / N, k = q % N;
    if (k <= i) continue;
    const double c = species_weight(i, k, n_up, m_up, m_dn, n_int);
    if (c == 0.0) continue;
    const zd ui = UV[SU * i], vi = UV[SU * i + 1], uk = UV[SU * k], vk = UV[SU * k + 1];
    const double a_re = ui.re * vk.re, a_re2 = ui.im * vk.im, b_re = uk.re * vi.re, b_re2 = uk.im * vi.im;
    const double a_im = ui.re * vk.im, a_im2 = ui.im * vk.re, b_im = uk.re * vi.im, b_im2 = uk.im * vi.re;
    const double wre = (a_re - a_re2) - (b_re - b_re2), wim = (a_im + a_im2) - (b_im + b_im2);
    const double r2 = wre * wre, i2 = wim * wim;
    const double tr = (0.5 * c) * log(r2 + i2), ti = c * atan2(wim, wre);
    lre = lre + tr;
    lim = lim + ti;
  }
  for (int o = G / 2; o > 0; o >>= 1) {
    const double pr = __shfl_xor(lre, o, G), pi = __shfl_xor(lim, o, G);
    lre = lre + pr;
    lim = lim + pi;
  }
  return zd{lre, lim};
}

// log psi as both instantiations store it: (float) Re, (float) principal phase
__device__ __forceinline__ void halperin_store(zd lp, float* re, float* im) {
  *re = (float)lp.re;
  *im = (float)remainder(lp.im, 2.0 * M_PI);
}

template <int G>
__global__ __launch_bounds__(kValueNT) void halperin_value_kernel(const float* __restrict__ x,
                                                                  float* __restrict__ out_lp, int nw, int N,
                                                                  int n_up, int m_up, int m_dn, int n_int) {
  extern __shared__ double smd[];
  constexpr int WPB = kValueNT / G;  // walkers per workgroup
  const int tid = threadIdx.x, grp = tid / G, lane = tid % G;
  const int b = blockIdx.x * WPB + grp;
  const bool live = b < nw;  // the last workgroup may hold fewer walkers; its idle groups read nothing
  zd* UV = reinterpret_cast<zd*>(smd) + (size_t)grp * 2 * N;
  if (live)
    for (int i = lane; i < N; i += G)
      uv_derivs<false>((double)x[2 * ((size_t)b * N + i)], (double)x[2 * ((size_t)b * N + i) + 1], UV + 2 * i);
  __syncthreads();
  const zd lp = halperin_logpsi<G>(UV, 2, N, n_up, m_up, m_dn, n_int, lane, live);
  if (live && lane == 0) halperin_store(lp, out_lp + 2 * (size_t)b, out_lp + 2 * (size_t)b + 1);
}

// LDS of the energy instantiation in zd units
struct HSm {
  int uv, g, H, zero, total;
};
__host__ __device__ inline HSm hsm_layout(int N) {
  HSm L{};
  int o = 0;
  L.uv = o;  // u, v, du[2], dv[2], d2u[3], d2v[3] = 12 per electron
  o += 12 * N;
  L.g = o;
  o += 2 * N;
  L.H = o;
  o += 4 * N * N;
  L.zero = o;  // the determinant part hamiltonian_tail adds to the pair part: none
  o += 1;
  L.total = o;
  return L;
}

template <int G>
__global__ __launch_bounds__(64) void halperin_energy_kernel(const float* __restrict__ x, float* __restrict__ e_l,
                                                             float* __restrict__ obs, int N, int n_up, int m_up,
                                                             int m_dn, int n_int, double Q, double radius,
                                                             double lambda, int interaction) {
  extern __shared__ double smd[];
  zd* sm = reinterpret_cast<zd*>(smd);
  const HSm L = hsm_layout(N);
  zd *UV = sm + L.uv, *g = sm + L.g, *H = sm + L.H, *zero = sm + L.zero;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int T = 2 * N, n_dn = N - n_up;
  for (int i = tid; i < N; i += nt)
    uv_derivs<true>((double)x[2 * ((size_t)b * N + i)], (double)x[2 * ((size_t)b * N + i) + 1], UV + 12 * i);
  if (tid == 0) *zero = zd{0.0, 0.0};
  __syncthreads();
  // group 0 of the wave, as a group of the value kernel (tid 0, which writes, is in it)
  const zd lpair = halperin_logpsi<G>(UV, 12, N, n_up, m_up, m_dn, n_int, tid % G, tid < G);
  // gradient: g_a = sum_k c d log w, the up partners then the down partners
  for (int a = tid; a < T; a += nt) {
    const int e = a >> 1, c = a & 1;
    const double wu = species_weight(e, 0, n_up, m_up, m_dn, n_int), wd = species_weight(e, N - 1, n_up, m_up, m_dn, n_int);
    zd s{0.0, 0.0};
    if (n_up > 0 && wu != 0.0) s = pair_grad(s, UV, n_up, e, c, wu);
    if (n_dn > 0 && wd != 0.0) s = pair_grad(s, UV + 12 * n_up, n_dn, e - n_up, c, wd);
    g[a] = s;
  }
  // Hessian: the same-electron blocks sum over the partners, a cross block is its pair's alone
  for (int idx = tid; idx < T * T; idx += nt) {
    const int a = idx / T, bb = idx % T, ea = a >> 1, ca = a & 1, eb = bb >> 1, cb = bb & 1;
    zd h{0.0, 0.0};
    if (ea == eb) {
      const double wu = species_weight(ea, 0, n_up, m_up, m_dn, n_int), wd = species_weight(ea, N - 1, n_up, m_up, m_dn, n_int);
      if (n_up > 0 && wu != 0.0) h = pair_hess_same(h, UV, n_up, ea, ca, cb, wu);
      if (n_dn > 0 && wd != 0.0) h = pair_hess_same(h, UV + 12 * n_up, n_dn, ea - n_up, ca, cb, wd);
    } else {
      const double w = species_weight(ea, eb, n_up, m_up, m_dn, n_int);
      if (w != 0.0) h = pair_hess_cross(h, UV + 12 * ea, UV + 12 * eb, ca, cb, w);
    }
    H[idx] = h;
  }
  __syncthreads();
  hamiltonian_tail(x, b, N, g, H, Q, radius, lambda, interaction, zero, lpair, e_l, obs, tid, nt);
}

}  // namespace

int halperin_group(int N) { return N <= 8 ? 16 : N <= 16 ? 32 : 64; }

size_t halperin_smem_bytes(int N, bool energy) {
  if (energy) return (size_t)hsm_layout(N).total * 2 * sizeof(double);
  return (size_t)(kValueNT / halperin_group(N)) * 2 * N * 2 * sizeof(double);
}

template <int G>
static void launch_halperin_g(const Dims& d, const float* x, int m_up, int m_dn, int n_int, float* logpsi, float* e_l,
                              float* obs, int nw, hipStream_t s) {
  if (e_l) {
    const size_t bytes = halperin_smem_bytes(d.N, true);
    ensure_smem(halperin_energy_kernel<G>, bytes);
    hipLaunchKernelGGL(halperin_energy_kernel<G>, dim3(nw), dim3(64), bytes, s, x, e_l, obs, d.N, d.n_up, m_up, m_dn,
                       n_int, (double)d.Q, (double)d.r, (double)d.lambda, d.interaction);
  } else {
    constexpr int WPB = kValueNT / G;
    hipLaunchKernelGGL(halperin_value_kernel<G>, dim3((nw + WPB - 1) / WPB), dim3(kValueNT),
                       halperin_smem_bytes(d.N, false), s, x, logpsi, nw, d.N, d.n_up, m_up, m_dn, n_int);
  }
}

void launch_halperin(const Dims& d, const float* x, int m_up, int m_dn, int n_int, float* logpsi, float* e_l,
                     float* obs, int nw, hipStream_t s) {
  const int G = halperin_group(d.N);
  if (G == 16)
    launch_halperin_g<16>(d, x, m_up, m_dn, n_int, logpsi, e_l, obs, nw, s);
  else if (G == 32)
    launch_halperin_g<32>(d, x, m_up, m_dn, n_int, logpsi, e_l, obs, nw, s);
  else
    launch_halperin_g<64>(d, x, m_up, m_dn, n_int, logpsi, e_l, obs, nw, s);
}

}  // namespace dh
