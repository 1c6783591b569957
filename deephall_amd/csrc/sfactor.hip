// Static structure factor in angular-momentum space (netobs/observables/structure_factor.py; not in
// the reference).  Walkers x[B][N][2] float32 (theta, phi), the slots below n_up up and the rest
// down; everything below is double arithmetic on the upcast coordinates.
//
//   pair sums    T_s(L) = sum over the pairs i < j of species s (uu, ud, dd) of P_L(cos gamma_ij),
//                cos gamma = cos th_i cos th_j + sin th_i sin th_j cos(ph_i - ph_j).  Lane l takes
//                the pairs l, l + 64, ... (up to 8 at N = 32), walks each upward by
//                P_{L+1} = x P_L + (L / (L + 1)) (x P_L - P_{L-1}), a form that stays at 1 and (-1)^L
//                exactly at x = 1, -1, and adds its own pairs by species; nothing is clamped: at |x|
//                marginally above 1 the recurrence is as good as inside.  Each per-L sum is then a
//                wave reduction by xor shuffles; lane L keeps T_s(L) (lane 0 also L = 64).
//   multipoles   rho^a_LM = sum over the electrons of species a of Y_LM, 0 <= M <= L <= lmax, at
//                lm = L (L + 1) / 2 + M.  Y_LM = Pn_LM(cos th) e^{i M ph} with the fully normalised
//                Pn: the sectoral seed Pn_MM = S_M (-sin th)^M, S_M = S_{M-1} sqrt((2M+1)/(2M)),
//                S_0 = 1 / sqrt(4 pi) (the Condon-Shortley phase is the minus sign; the power by
//                repeated squaring, so sin^M th underflows to 0 near a pole as it should), then
//                upward in L: Pn_LM = a_LM (cos th Pn_{L-1,M} - Pn_{L-2,M} / a_{L-1,M}),
//                a_LM = sqrt((4 L^2 - 1) / (L^2 - M^2)).  No factorial is ever formed.  sin th keeps
//                its sign (theta past pi is the point (2 pi - theta, phi + pi), as in cos gamma).
//                The phase is one sincos(M ph) per electron and M.  Lane M owns the column M of
//                both species (lane 0 also M = 64), so the accumulator rows in LDS have one writer;
//                it walks four electrons of a species side by side (independent recurrences hide
//                each other's latency) and adds them in slot order into one update of the row.
//
// One wave is one workgroup.  Its dynamic LDS holds L / (L + 1), S_M, the walker's cos th, sin th
// and ph, and, for the multipoles, a_LM, 1 / a_{L-1,M} and the accumulator [2][nlm] complex: 48 nlm
// + 1824 bytes, 104800 at lmax = 64 (one workgroup per CU there, several at the usual lmax).
//
//   sf_pairs_kernel       T[B][3][lmax+1], sf_multipoles_kernel  rho[B][2][nlm] complex: per walker,
//                         NaN rows for a walker with a non-finite coordinate.
//   sf_accumulate_kernel  the same walker functions fused with the sum over walkers: workgroup g
//                         takes the walkers [g W, (g + 1) W) in ascending order, the pair sums in
//                         registers and the multipoles in its LDS accumulator, and writes one partial
//                         (pair sums, multipole sums, valid count) to the workspace;
//   sf_finish_kernel      adds the partials in workgroup order.
// W = max(8, ceil(B / 512)) depends on B alone.  A fixed order, no float atomics, and the file is
// built with -ffp-contract=off (_build.py; the fused operations are written out as fma), so every
// instantiation rounds alike: two calls give identical bits, and the pair sums are the same bits
// with and without the multipoles.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kHead = 228;  // doubles in front of the tables: c[66], seed[66], ct[32], st[32], ph[32]
constexpr double kInvSqrt4Pi = 0.28209479177387814347403972578039;

struct Smem {
  double *c, *seed, *ct, *st, *ph, *a, *ainv;
  double2* acc;
};

__device__ __forceinline__ Smem carve(double* base, int nlm) {
  const int n2 = (nlm + 1) & ~1;  // keeps acc 16-byte aligned
  Smem m;
  m.c = base;
  m.seed = base + 66;
  m.ct = base + 132;
  m.st = base + 164;
  m.ph = base + 196;
  m.a = base + kHead;
  m.ainv = m.a + n2;
  m.acc = reinterpret_cast<double2*>(m.ainv + n2);
  return m;
}

template <bool WANT>
__device__ void fill_tables(const Smem& m, int lmax, int lane) {
  for (int L = lane; L <= lmax; L += 64) m.c[L] = (double)L / (double)(L + 1);
  if (lane == 0) {
    double s = kInvSqrt4Pi;
    m.seed[0] = s;
    for (int M = 1; M <= lmax; ++M) {
      s *= sqrt((double)(2 * M + 1) / (double)(2 * M));
      m.seed[M] = s;
    }
  }
  if (WANT) {
    for (int L = 0; L <= lmax; ++L)
      for (int M = lane; M <= L; M += 64) {
        const int lm = L * (L + 1) / 2 + M;
        const double l1 = L - 1;
        m.a[lm] = L > M ? sqrt((4.0 * L * L - 1.0) / ((double)L * L - (double)M * M)) : 0.0;
        m.ainv[lm] = L > M + 1 ? sqrt((l1 * l1 - (double)M * M) / (4.0 * l1 * l1 - 1.0)) : 0.0;
      }
  }
  __syncthreads();
}

// The walker's trigonometry into LDS; false (nothing written) when a coordinate is not finite.
__device__ bool load_walker(const float* __restrict__ x, size_t b, int N, int lane, const Smem& m) {
  const float* xb = x + b * 2 * N;
  const float v = lane < 2 * N ? xb[lane] : 0.0f;
  if (__any(!isfinite(v))) return false;
  __syncthreads();  // the previous walker's readers are done
  if (lane < N) {
    double s, c;
    sincos((double)xb[2 * lane], &s, &c);
    m.ct[lane] = c;
    m.st[lane] = s;
    m.ph[lane] = (double)xb[2 * lane + 1];
  }
  __syncthreads();
  return true;
}

// lo[s] += T_s(lane) (lanes 0 .. min(lmax, 63)), hi[s] += T_s(64), s = uu, ud, dd.  Lane l holds the
// pairs l, l + 64, ... (C of them at most, np <= 64 C), walks their recurrences side by side and adds
// them by species in that order before the three wave reductions of each L.
template <int C>
__device__ __forceinline__ void walker_pairs_c(int N, int n_up, int lmax, int lane, const Smem& m, double lo[3],
                                               double hi[3]) {
  const int np = N * (N - 1) / 2;
  double xx[C], pm[C], pc[C];
  int type[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int p = k * 64 + lane;
    type[k] = -1;
    xx[k] = 0.0;
    pm[k] = pc[k] = 1.0;  // P_{L-1}, P_L
    if (p < np) {
      int i = 0, r = p;
      while (r >= N - 1 - i) {
        r -= N - 1 - i;
        ++i;
      }
      const int j = i + 1 + r;
      type[k] = j < n_up ? 0 : i < n_up ? 1 : 2;
      xx[k] = fma(m.ct[i], m.ct[j], m.st[i] * m.st[j] * cos(m.ph[i] - m.ph[j]));
    }
  }
  for (int L = 0; L <= lmax; ++L) {
    const double c = m.c[L];
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      t0 += type[k] == 0 ? pc[k] : 0.0;
      t1 += type[k] == 1 ? pc[k] : 0.0;
      t2 += type[k] == 2 ? pc[k] : 0.0;
      const double xp = xx[k] * pc[k];
      const double pn = fma(c, xp - pm[k], xp);
      pm[k] = pc[k];
      pc[k] = pn;
    }
    t0 = wave_sum(t0);
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
    if (L < 64) {
      if (lane == L) {
        lo[0] += t0;
        lo[1] += t1;
        lo[2] += t2;
      }
    } else {
      hi[0] += t0;
      hi[1] += t1;
      hi[2] += t2;
    }
  }
}

__device__ __forceinline__ void walker_pairs(int N, int n_up, int lmax, int lane, const Smem& m, double lo[3], double hi[3]) {
  const int np = N * (N - 1) / 2;  // <= 496 = 7.75 x 64
  if (np <= 64)
    walker_pairs_c<1>(N, n_up, lmax, lane, m, lo, hi);
  else if (np <= 128)
    walker_pairs_c<2>(N, n_up, lmax, lane, m, lo, hi);
  else if (np <= 256)
    walker_pairs_c<4>(N, n_up, lmax, lane, m, lo, hi);
  else
    walker_pairs_c<8>(N, n_up, lmax, lane, m, lo, hi);
}

// acc[a][lm] += Y_lm of the walker's electrons of species a: kGrp electrons at a time walk their
// recurrences side by side (a short last group is padded with zero seeds) and are added in slot
// order before they reach the accumulator, whose next row is fetched before this one is stored.
constexpr int kGrp = 4;

__device__ __forceinline__ void walker_multipoles(int N, int n_up, int lmax, int nlm, int lane, const double* __restrict__ ctv,
                                  const double* __restrict__ stv, const double* __restrict__ phv,
                                  const double* __restrict__ seed, const double* __restrict__ a,
                                  const double* __restrict__ ainv, double2* __restrict__ acc) {
  for (int M = lane; M <= lmax; M += 64) {
    const double sd = seed[M];
    for (int sp = 0; sp < 2; ++sp) {
      const int e0 = sp ? n_up : 0, e1 = sp ? N : n_up;
      double2* ac = acc + sp * nlm;
      for (int g = e0; g < e1; g += kGrp) {
        double ct[kGrp], p1[kGrp], p2[kGrp], cs[kGrp], sn[kGrp];
#pragma unroll
        for (int k = 0; k < kGrp; ++k) {
          const bool on = g + k < e1;
          const int e = on ? g + k : e0;
          ct[k] = ctv[e];
          double r = 1.0, base = -stv[e];
          for (int q = M; q; q >>= 1) {
            if (q & 1) r *= base;
            base *= base;
          }
          double s1, c1;
          sincos((double)M * phv[e], &s1, &c1);
          sn[k] = s1;
          cs[k] = c1;
          p1[k] = on ? sd * r : 0.0;
          p2[k] = 0.0;
        }
        int lm = M * (M + 1) / 2 + M;
        double2 v = ac[lm];
        for (int L = M; L <= lmax; ++L) {
          double sx = 0.0, sy = 0.0;
          if (L > M) {
            const double al = a[lm], bl = ainv[lm];
#pragma unroll
            for (int k = 0; k < kGrp; ++k) {
              const double p = al * fma(ct[k], p1[k], -(bl * p2[k]));
              p2[k] = p1[k];
              p1[k] = p;
            }
          }
#pragma unroll
          for (int k = 0; k < kGrp; ++k) {
            sx = fma(p1[k], cs[k], sx);
            sy = fma(p1[k], sn[k], sy);
          }
          const int next = lm + L + 1;
          const double2 vn = L < lmax ? ac[next] : make_double2(0.0, 0.0);
          ac[lm] = make_double2(v.x + sx, v.y + sy);
          v = vn;
          lm = next;
        }
      }
    }
  }
}

__device__ __forceinline__ void zero_acc(const Smem& m, int nlm, int lane) {
  __syncthreads();
  for (int k = lane; k < 2 * nlm; k += 64) m.acc[k] = make_double2(0.0, 0.0);
  __syncthreads();
}

__global__ __launch_bounds__(64) void sf_pairs_kernel(const float* __restrict__ x, int B, int N, int n_up, int lmax,
                                                      double* __restrict__ T) {
  extern __shared__ __attribute__((aligned(16))) double sf_smem[];
  const int lane = threadIdx.x, nl = lmax + 1;
  const Smem m = carve(sf_smem, 0);
  fill_tables<false>(m, lmax, lane);
  const double nan = quiet_nan();
  for (size_t b = blockIdx.x; b < (size_t)B; b += gridDim.x) {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    const bool ok = load_walker(x, b, N, lane, m);
    if (ok) walker_pairs(N, n_up, lmax, lane, m, lo, hi);
    double* Tb = T + b * 3 * nl;
    for (int s = 0; s < 3; ++s) {
      if (lane < nl) Tb[s * nl + lane] = ok ? lo[s] : nan;
      if (lane == 0 && lmax == 64) Tb[s * nl + 64] = ok ? hi[s] : nan;
    }
  }
}

__global__ __launch_bounds__(64) void sf_multipoles_kernel(const float* __restrict__ x, int B, int N, int n_up,
                                                           int lmax, int nlm, double2* __restrict__ rho) {
  extern __shared__ __attribute__((aligned(16))) double sf_smem[];
  const int lane = threadIdx.x;
  const Smem m = carve(sf_smem, nlm);
  fill_tables<true>(m, lmax, lane);
  const double nan = quiet_nan();
  for (size_t b = blockIdx.x; b < (size_t)B; b += gridDim.x) {
    zero_acc(m, nlm, lane);
    const bool ok = load_walker(x, b, N, lane, m);
    if (ok) walker_multipoles(N, n_up, lmax, nlm, lane, m.ct, m.st, m.ph, m.seed, m.a, m.ainv, m.acc);
    __syncthreads();
    double2* rb = rho + b * 2 * nlm;
    for (int k = lane; k < 2 * nlm; k += 64) rb[k] = ok ? m.acc[k] : make_double2(nan, nan);
  }
}

// part[g][stride]: [3][lmax+1] pair sums, then (WANT) [2][nlm] complex; cnt[g]
template <bool WANT>
__global__ __launch_bounds__(64) void sf_accumulate_kernel(const float* __restrict__ x, int B, int N, int n_up,
                                                           int lmax, int nlm, int W, int stride,
                                                           double* __restrict__ part, int32_t* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) double sf_smem[];
  const int lane = threadIdx.x, nl = lmax + 1, g = blockIdx.x;
  const Smem m = carve(sf_smem, WANT ? nlm : 0);
  fill_tables<WANT>(m, lmax, lane);
  if (WANT) zero_acc(m, nlm, lane);
  double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
  int n = 0;
  const int b0 = g * W, b1 = min(B, b0 + W);  // b0 < B: the grid is ceil(B / W)
  for (int b = b0; b < b1; ++b) {
    if (!load_walker(x, (size_t)b, N, lane, m)) continue;
    walker_pairs(N, n_up, lmax, lane, m, lo, hi);
    if (WANT) walker_multipoles(N, n_up, lmax, nlm, lane, m.ct, m.st, m.ph, m.seed, m.a, m.ainv, m.acc);
    ++n;
  }
  double* pg = part + (size_t)g * stride;
  for (int s = 0; s < 3; ++s) {
    if (lane < nl) pg[s * nl + lane] = lo[s];
    if (lane == 0 && lmax == 64) pg[s * nl + 64] = hi[s];
  }
  if (WANT) {
    __syncthreads();
    double2* pr = reinterpret_cast<double2*>(pg + 3 * nl);
    for (int k = lane; k < 2 * nlm; k += 64) pr[k] = m.acc[k];
  }
  if (lane == 0) cnt[g] = n;
}

__global__ __launch_bounds__(256) void sf_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ cnt,
                                                        int G, int stride, int npair, double* __restrict__ pair_sums,
                                                        double* __restrict__ rho_sums, int32_t* __restrict__ nvalid) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < stride) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * stride + t];
    if (t < npair)
      pair_sums[t] = s;
    else
      rho_sums[t - npair] = s;
  }
  if (t == 0) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += cnt[g];
    *nvalid = n;
  }
}

size_t lds_bytes(int nlm) { return (size_t)(kHead + 2 * ((nlm + 1) & ~1) + 4 * nlm) * sizeof(double); }

int walkers_per_group(int B) { return std::max(8, (B + 511) / 512); }
int groups(int B) {
  const int W = walkers_per_group(B);
  return (B + W - 1) / W;
}
size_t partial_doubles(int lmax) { return (size_t)3 * (lmax + 1) + 4 * (size_t)sf_nlm(lmax); }

}  // namespace

int sf_nlm(int lmax) { return (lmax + 1) * (lmax + 2) / 2; }

// part [G][3 (lmax + 1) + 4 nlm] double, then cnt [G] int32
size_t sf_workspace_bytes(int B, int lmax) {
  const size_t G = groups(B);
  return G * partial_doubles(lmax) * sizeof(double) + G * sizeof(int32_t);
}

void launch_sf_pairs(const float* x, int B, int N, int n_up, int lmax, double* T, hipStream_t s) {
  hipLaunchKernelGGL(sf_pairs_kernel, dim3(std::min(B, 1024)), dim3(64), lds_bytes(0), s, x, B, N, n_up, lmax, T);
}

void launch_sf_multipoles(const float* x, int B, int N, int n_up, int lmax, double* rho, hipStream_t s) {
  const int nlm = sf_nlm(lmax);
  ensure_smem(sf_multipoles_kernel, lds_bytes(nlm));
  hipLaunchKernelGGL(sf_multipoles_kernel, dim3(std::min(B, 1024)), dim3(64), lds_bytes(nlm), s, x, B, N, n_up, lmax,
                     nlm, reinterpret_cast<double2*>(rho));
}

void launch_sf_accumulate(const float* x, int B, int N, int n_up, int lmax, bool want, double* pair_sums,
                          double* rho_sums, int32_t* nvalid, void* workspace, hipStream_t s) {
  const int nlm = sf_nlm(lmax), W = walkers_per_group(B), G = groups(B), npair = 3 * (lmax + 1);
  const int stride = want ? (int)partial_doubles(lmax) : npair;
  double* part = static_cast<double*>(workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(part + (size_t)G * partial_doubles(lmax));
  if (want) {
    ensure_smem(sf_accumulate_kernel<true>, lds_bytes(nlm));
    hipLaunchKernelGGL(sf_accumulate_kernel<true>, dim3(G), dim3(64), lds_bytes(nlm), s, x, B, N, n_up, lmax, nlm, W,
                       stride, part, cnt);
  } else {
    hipLaunchKernelGGL(sf_accumulate_kernel<false>, dim3(G), dim3(64), lds_bytes(0), s, x, B, N, n_up, lmax, nlm, W,
                       stride, part, cnt);
  }
  hipLaunchKernelGGL(sf_finish_kernel, dim3((stride + 255) / 256), dim3(256), 0, s, part, cnt, G, stride, npair,
                     pair_sums, rho_sums, nvalid);
}

}  // namespace dh
