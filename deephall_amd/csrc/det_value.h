// Device code of the log-psi value kernel (det.hip det_value_kernel) shared with the layer-2
// chain launch (gemm_x6.hip chain_x6s_kernel<-1>), which runs the same body as its tail on
// orbital rows that never leave the CU: the envelope values, the Jastrow term, the contraction
// Phi_k = sum_m F env, the pivoted LU, the log-sum-exp over determinants and the MCMC accept /
// next proposal (McmcEpi).  One body for both launches, so that they agree bit for bit; it is
// parameterised on where a row of F lives (global with ldF, or an LDS tile) and on the barrier
// (the stand-alone kernel's workgroup is one wave and keeps __syncthreads; inside the chain's
// 512-thread workgroup every wave works on its own walkers in its own LDS regions and uses a
// wave barrier).
#pragma once
#include "dh_internal.h"
#include "device_common.h"
#include "mcmc_common.h"

#ifndef DET_LU_REG  // A/B knob: det_value's LU with one column per lane in registers (1) or eliminate (0):
#define DET_LU_REG 0  // bitwise equal, measured 0.3-0.7 us per call slower at C2 (profiles/r05_v17_det_ab.txt)
#endif
#ifndef DET_T  // phase stamps: det.hip's diagnostic builds only
#define DET_T(slot, i)
#endif

namespace dh {

// The barrier between the phases of a walker's threads.  BlockSync: the threads are a whole
// workgroup.  WaveSync: they are (half of) one wave of a larger workgroup whose other waves
// work elsewhere: the wave's LDS traffic drained, then a wave barrier (no s_barrier: the other
// waves of the workgroup never arrive)
struct BlockSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
struct WaveSync {
  __device__ __forceinline__ void operator()() const {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
};

// Rows of F in global memory: row (walker b, electron i) at F + (b N + i) ld
struct FRowsGlobal {
  const float* __restrict__ F;
  int ld, N;
  __device__ __forceinline__ const float* operator()(int b, int i) const { return F + ((size_t)b * N + i) * ld; }
};
// Rows of F in an LDS tile that starts at walker b0: row (b, i) at F + ((b - b0) N + i) ld
struct FRowsTile {
  const float* F;
  int ld, N, b0;
  __device__ __forceinline__ const float* operator()(int b, int i) const { return F + ((b - b0) * N + i) * ld; }
};

__device__ inline float ipow(float b, int e) { return e < 0 ? 0.f : (e == 0 ? 1.f : powf(b, (float)e)); }
// integer power by squaring (the envelope values and leaves: a few multiplies per power instead
// of powf's log / exp).  Not powf's 1-ulp result: squaring doubles the relative error it
// carries, so b^e is within about (e + popcount(e)) * 2^-24 relative (< 4e-6 at e = 57, C5's
// largest exponent) against powf's ~6e-8; tests/test_gpu_kernels.py::test_env_leaf_powers
// bounds both forms against float64 at M = 58 near the poles (dh_debug_env_leaf)
__device__ inline float ipow_sq(float b, int e) {
  float r = 1.f;
  for (; e > 0; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// envelope value (and optionally leaves) for electron angle (th, ph), harmonic index p
struct EnvLeaf {
  cf e0, dth, dph, lb, d2th;
};
// `gauge` = kappa removes the per-electron phase exp(i kappa phi) from the envelope (0 =
// reference gauge); the removed term i sum_i kappa_i phi_i is added back analytically (in
// double) by the energy assembly.  kappa_i = env_gauge(cos theta_i): the envelope's dominant
// harmonic m* = Q cos theta (|u|^2 = cos^2 theta/2 weights Q + m binomially), so the phi
// derivatives i (m - kappa) of the contracted orbitals stay small for every electron.  At the
// poles this is the north / south patch (kappa = +-Q: regular channels where the reference's
// 1 / sin theta terms blow up); near the equator it stays ~0 where the patch choice put up to
// 2Q into every phi channel and the f32 contractions below lost the digits.
// Quantised to 1/64 of Q so that m - kappa is exact in f32.
__device__ __forceinline__ float env_gauge(float ct, int M) {
  return (float)(M - 1) * __builtin_rintf(64.f * ct) * (1.f / 128.f);
}
__device__ inline EnvLeaf env_leaf(float th, float ph, int p, int M, float norm, bool leaves, float gauge = 0.f,
                                   bool sq = false) {
  const int a = p, b = M - 1 - p;
  const float m = 0.5f * (float)(a - b) - gauge;
  float c, s;
  sincosf(0.5f * th, &s, &c);
  float sph, cph;
  sincosf(m * ph, &sph, &cph);
  const float R = sq ? ipow_sq(c, a) * ipow_sq(s, b) : ipow(c, a) * ipow(s, b);
  EnvLeaf L;
  L.e0 = cf{norm * R * cph, norm * R * sph};
  if (leaves) {
    const float fa = (float)a, fb = (float)b;
    // sq: the powers by squaring here too (negative exponents 0, as ipow)
    auto pw = [sq](float x, int e) { return sq ? (e < 0 ? 0.f : ipow_sq(x, e)) : ipow(x, e); };
    const float R1 = 0.5f * (fb * pw(c, a + 1) * pw(s, b - 1) - fa * pw(c, a - 1) * pw(s, b + 1));
    const float R2 = 0.25f * (fb * (fb - 1.f) * pw(c, a + 2) * pw(s, b - 2) - fb * (fa + 1.f) * R -
                              fa * (fb + 1.f) * R + fa * (fa - 1.f) * pw(c, a - 2) * pw(s, b + 2));
    float st, ct;
    sincosf(th, &st, &ct);
    L.dth = cf{norm * R1 * cph, norm * R1 * sph};
    L.d2th = cf{norm * R2 * cph, norm * R2 * sph};
    // d/dphi / sin th = i m e0 / st
    L.dph = cf{-m * L.e0.im / st, m * L.e0.re / st};
    // LB = d2th - m^2 e0 / st^2 + cot th * dth
    const float cot = ct / st;
    const float k2 = m * m / (st * st);
    L.lb = cf{L.d2th.re - k2 * L.e0.re + cot * L.dth.re, L.d2th.im - k2 * L.e0.im + cot * L.dth.im};
  }
  return L;
}

// the first `width` threads (a wave, or a half-wave per walker) find the pivot row (first
// max of |re|+|im| in column p, rows >= p)
__device__ inline void find_pivot(const cf* A, int lda, int N, int p, int* piv, int tid, int width) {
  if (tid < width) {
    const int lane = tid;
    float best = -1.f;
    int bi = N;
    for (int r = p + lane; r < N; r += width) {
      const float v = cabs1(A[r * lda + p]);
      if (v > best) {
        best = v;
        bi = r;
      }
    }
    for (int o = width >> 1; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, width);
      const int oi = __shfl_xor(bi, o, width);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    if (lane == 0) *piv = (bi < N) ? bi : p;
  }
}

// In-place elimination on A [N][ncol] (lda) with partial pivoting.
//   gj = true : Gauss-Jordan on an augmented [A | I] (ncol = 2N): right block -> A^-1
//   gj = false: LU (rows below the pivot only) — determinant only
// Accumulates log det into logdet (complex, phase unwrapped).  Barriers: sync (BlockSync:
// __syncthreads).
// tid / nt: this walker's threads (default the whole block; det_value's half-wave form
// passes its 32 lanes and width 32 for the pivot search).
// PIN (det_value's half-wave form, LU only): the pivot's magnitude, the factors and the update
// are written out with the roundings det_value_kernel<0, true> has always had (its products
// come in (re, im) pairs that the compiler packs, which decides what it fuses: |P|^2 = re re +
// im im with no fused product, one product fused in the factor's imaginary part and in each
// part of the update), so that the chain launch's tail (gemm_x6.hip, compiled without that
// packing) rounds the same way; left to the compiler there, it fused |P|^2 and the real part
// of the factor, and log psi differed in the last bits.
struct PinnedLu {
  static __device__ __forceinline__ float mag2(cf P) {
#pragma clang fp contract(off)
    const float rr = P.re * P.re, ii = P.im * P.im;
    return rr + ii;
  }
  static __device__ __forceinline__ cf factor(cf c, cf Pinv) {
#pragma clang fp contract(off)
    const float rr = c.re * Pinv.re, ii = c.im * Pinv.im, ri = c.re * Pinv.im;
    return cf{rr - ii, __builtin_fmaf(c.im, Pinv.re, ri)};
  }
  static __device__ __forceinline__ cf update(cf v, cf f, cf a) {
#pragma clang fp contract(off)
    const float ii = f.im * a.im, ri = f.re * a.im;
    const float tre = __builtin_fmaf(f.re, a.re, -ii);
    const float tim = __builtin_fmaf(f.im, a.re, ri);
    return cf{v.re - tre, v.im - tim};
  }
};
template <class Sync = BlockSync, bool PIN = false>
__device__ __forceinline__ void eliminate(cf* A, int lda, int N, int ncol, bool gj, cf* fac, int* piv, cf* logdet,
                          int tid = threadIdx.x, int nt = blockDim.x, int width = 64, Sync sync = Sync{}) {
  if (tid == 0) *logdet = cf{0.f, 0.f};
  sync();
  for (int p = 0; p < N; ++p) {
    find_pivot(A, lda, N, p, piv, tid, width);
    sync();
    const int pr = *piv;
    if (pr != p) {
      for (int c = tid; c < ncol; c += nt) {
        const cf t = A[p * lda + c];
        A[p * lda + c] = A[pr * lda + c];
        A[pr * lda + c] = t;
      }
    }
    sync();
    const cf P = A[p * lda + p];
    if (tid == 0) {
      const float mag = PIN ? sqrtf(PinnedLu::mag2(P)) : sqrtf(P.re * P.re + P.im * P.im);
      logdet->re += logf(mag);
      logdet->im += atan2f(P.im, P.re) + (pr != p ? kPi : 0.f);
    }
    const cf Pinv = cdiv(cf{1.f, 0.f}, P);
    sync();
    if (gj) {
      for (int r = tid; r < N; r += nt) fac[r] = (r == p) ? cf{0.f, 0.f} : A[r * lda + p];
      for (int c = tid; c < ncol; c += nt) A[p * lda + c] = A[p * lda + c] * Pinv;
    } else {
      for (int r = tid; r < N; r += nt)
        fac[r] = (r > p) ? (PIN ? PinnedLu::factor(A[r * lda + p], Pinv) : A[r * lda + p] * Pinv) : cf{0.f, 0.f};
    }
    sync();
    const int r0 = gj ? 0 : p + 1;
    const int c0 = gj ? 0 : p;
    const int nr = N - r0, nc = ncol - c0;
    for (int idx = tid; idx < nr * nc; idx += nt) {
      const int r = r0 + idx / nc, c = c0 + idx % nc;
      if (r == p) continue;
      const cf f = fac[r];
      cf v = A[r * lda + c];
      const cf a = A[p * lda + c];
      if constexpr (PIN) {
        v = PinnedLu::update(v, f, a);
      } else {
        v.re -= f.re * a.re - f.im * a.im;
        v.im -= f.re * a.im + f.im * a.re;
      }
      A[r * lda + c] = v;
    }
    sync();
  }
}

// eliminate(A, N, N, N, gj = false) for N <= NMAX with column c of A in registers of lane c
// of the (half-)wave (round 5): the same pivots (first maximum of cabs1 at or below the
// diagonal), the same factors f = A[r][p] / P and updates of columns c >= p, the same log det
// terms — without LDS round trips or barriers (the pivot search is lane p's own column, the
// pivot and factors reach the other lanes by shuffles).  Register arrays are indexed only by
// compile-time constants (selects), or they would go to scratch.
template <int NMAX>
__device__ __forceinline__ cf lu_logdet_cols(cf (&col)[NMAX], int N, int lane, int width) {
  // r == q through an opaque value: left visible, the compiler turns the select chain into a
  // run-time index of col (and col into scratch)
  auto is = [](int r, int q) __attribute__((always_inline)) {
    int m = r == q;
    asm volatile("" : "+v"(m));
    return m != 0;
  };
  auto pick = [&](int q) __attribute__((always_inline)) {
    cf v = col[0];
#pragma unroll
    for (int r = 1; r < NMAX; ++r)
      if (is(r, q)) v = col[r];
    return v;
  };
  float lre = 0.f, lim = 0.f;
  for (int p = 0; p < N; ++p) {
    float best = -1.f;
    int bi = N;
#pragma unroll
    for (int r = 0; r < NMAX; ++r) {
      if (r >= p && r < N) {
        const float v = cabs1(col[r]);
        if (v > best) {
          best = v;
          bi = r;
        }
      }
    }
    int pr = __shfl(bi, p, width);
    pr = pr < N ? pr : p;
    if (pr != p) {  // swap rows p and pr (every column)
      const cf a = pick(p), b = pick(pr);
#pragma unroll
      for (int r = 0; r < NMAX; ++r) {
        if (is(r, p)) col[r] = b;
        if (is(r, pr)) col[r] = a;
      }
    }
    const cf mine = pick(p);  // A[p][lane]
    const cf P{__shfl(mine.re, p, width), __shfl(mine.im, p, width)};
    const float mag = sqrtf(P.re * P.re + P.im * P.im);
    lre += logf(mag);
    lim += atan2f(P.im, P.re) + (pr != p ? kPi : 0.f);
    const cf Pinv = cdiv(cf{1.f, 0.f}, P);
#pragma unroll
    for (int r = 0; r < NMAX; ++r) {
      if (r > p && r < N) {
        // the roundings of eliminate's code (its factor and update as the compiler emits them:
        // one product of each pair fused), so that equal rows cancel exactly as there and a
        // singular matrix keeps its zero pivot (psi = 0, tests/test_gpu_grad.py)
#pragma clang fp contract(off)
        const cf c = col[r];
        const cf fl{c.re * Pinv.re - c.im * Pinv.im, __builtin_fmaf(c.im, Pinv.re, c.re * Pinv.im)};
        const cf f{__shfl(fl.re, p, width), __shfl(fl.im, p, width)};  // lane p's: row r's factor
        if (lane >= p) {
          const float tre = __builtin_fmaf(f.re, mine.re, -(f.im * mine.im));
          const float tim = __builtin_fmaf(f.im, mine.re, f.re * mine.im);
          col[r] = cf{c.re - tre, c.im - tim};
        }
      }
    }
  }
  return cf{lre, lim};
}

__device__ inline double jastrow_pair(double r, double al, double cst, double* f1, double* f2) {
  const double ar = al + r;
  *f1 = (cst * al * al) / (ar * ar);
  *f2 = -2.0 * (cst * al * al) / (ar * ar * ar);
  return -(cst * al * al) / ar;
}

// ------------------------------------------------------------------ value body
// log psi of walker bw (and, with epi.on, its MCMC accept and next proposal) by the nt threads
// tid < nt of one (half-)wave, in the walker's LDS region sm_raw (det_value_per floats).
// The orbital matrix is contracted row by row: lane (j, g) sums harmonics m = g + G u
// (G = 64 / N lane groups, u < MGV, all loads of a row in flight at once, one wave load
// instruction covering G consecutive harmonics = 4 G N contiguous bytes), groups combined
// with shuffles.
// HW (MGV = 0 only): the walker has one 32-lane half of the wave (the other half works on the
// next walker in its own region): the serial parts (pivot search, log det, Jastrow reduction)
// then serve two walkers per instruction.
// live = false: a dead half (no walker left): it repeats walker nw - 1 and writes nothing.
// x is not __restrict__: with the MCMC epilogue it is the same buffer as epi.x2, which the
// epilogue writes (each thread reads its own walker's angles before that, behind a barrier)
template <int MGV, bool HW, class Sync, class FRows>
__device__ __forceinline__ void det_value_body(float* sm_raw, FRows frow, const float* x,
                                               const float* __restrict__ jas, const float* __restrict__ norm,
                                               float* __restrict__ logpsi, int N, int n_up, int M, int K, int bw,
                                               int nw, int tid, const McmcEpi& epi, Sync sync) {
  static_assert(!HW || MGV == 0, "half-wave form: serial contraction only");
  cf* E0 = reinterpret_cast<cf*>(sm_raw);  // [N][M]
  cf* A = E0 + N * M;                      // [N][N]
  cf* fac = A + N * N;                     // [N]
  cf* ld = fac + N;                        // [K] log dets
  cf* logdet = ld + K;
  int* piv = reinterpret_cast<int*>(logdet + 1);
  const bool live = bw < nw;
  const int b = live ? bw : nw - 1;  // a dead half repeats the last walker, writes nothing
  const int nt = HW ? 32 : 64, width = HW ? 32 : 64;
  double* cart = reinterpret_cast<double*>(piv + 2);  // [N][3] unit vectors (double: close pairs)
  DET_T(0, 0);
  for (int idx = tid; idx < N * M; idx += nt) {
    const int i = idx / M, p = idx % M;
    E0[idx] = env_leaf(x[2 * (b * N + i)], x[2 * (b * N + i) + 1], p, M, norm[p], false, 0.f, true).e0;
  }
  for (int i = tid; i < N; i += nt) {
    double st, ct, sp, cp;
    sincos((double)x[2 * (b * N + i)], &st, &ct);
    sincos((double)x[2 * (b * N + i) + 1], &sp, &cp);
    cart[3 * i] = st * cp;
    cart[3 * i + 1] = st * sp;
    cart[3 * i + 2] = ct;
  }
  sync();
  DET_T(0, 1);
  // Jastrow (blocks.py:76-121): chord distances on the unit sphere, pairs spread over the
  // wave, accumulated in double and reduced with shuffles (one 64-lane wave per walker)
  double Jw = 0.0;
  {
    const double ap = jas[0], aa = jas[1];
    for (int q = tid; q < N * N; q += nt) {
      const int i = q / N, j = q - (q / N) * N;
      if (j <= i) continue;
      const double dx = cart[3 * j] - cart[3 * i], dy = cart[3 * j + 1] - cart[3 * i + 1],
                   dz = cart[3 * j + 2] - cart[3 * i + 2];
      const double r = sqrt(dx * dx + dy * dy + dz * dz);
      const bool same = (i < n_up) == (j < n_up);
      double f1, f2;
      Jw += jastrow_pair(r, same ? ap : aa, same ? 0.25 : 0.5, &f1, &f2);
    }
    for (int o = width >> 1; o > 0; o >>= 1) Jw += __shfl_xor(Jw, o, width);
  }
  DET_T(0, 2);
  const int G = 64 / N, gj = tid % N, gg = tid / N, NK = N * K, MNK = M * NK;
  for (int k = 0; k < K; ++k) {
    if constexpr (MGV == 0) {  // small rows: one thread per entry, serial over m
      for (int idx = tid; idx < N * N; idx += nt) {
        const int i = idx / N, j = idx % N;
        const int blk = (i >= n_up && n_up > 0) ? 1 : 0;
        const float* rp = frow(b, i) + (size_t)blk * 2 * MNK + (size_t)j * K + k;
        cf acc{0.f, 0.f};
        // 16 harmonics' loads in flight at once (a loop with the trip count M at run time
        // waited for every pair before its FMA: 16 L2 round trips in a row at C2); the same
        // products summed in the same order
        for (int p0 = 0; p0 < M; p0 += 16) {
          float fr[16], fi[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const size_t p = (size_t)min(p0 + q, M - 1);
            fr[q] = rp[p * NK];
            fi[q] = rp[(size_t)MNK + p * NK];
          }
#pragma unroll
          for (int q = 0; q < 16; ++q)
            if (p0 + q < M) cfma(acc, cf{fr[q], fi[q]}, E0[i * M + p0 + q]);
        }
        A[idx] = acc;
      }
    }
    if constexpr (MGV > 0) {
      // row i's F loads in flight while row i - 1 is contracted (two register sets, rows in
      // pairs; round 5): one row at a time waited for every row's L2 / HBM round trip (C5: 20
      // rows, 63 % of the kernel, profiles/r05_v17_det_stamps_c5.txt).  The loads are
      // unconditional (clamped harmonic and row; out-of-range terms zeroed after the load), so
      // the compiler's counted waits leave the other set in flight.
      constexpr int NF = 2 * (MGV > 0 ? MGV : 1);
      auto ldrow = [&](int i, float (&f)[NF]) __attribute__((always_inline)) {
        const int blk = (i >= n_up && n_up > 0) ? 1 : 0;
        const float* rp = frow(b, i) + (size_t)blk * 2 * MNK + (size_t)gj * K + k;
#pragma unroll
        for (int u = 0; u < MGV; ++u) {
          const size_t m = (size_t)min(gg + G * u, M - 1);
          f[2 * u] = rp[m * NK];
          f[2 * u + 1] = rp[(size_t)MNK + m * NK];
        }
      };
      auto contract = [&](int i, const float (&f)[NF]) __attribute__((always_inline)) {
        cf acc{0.f, 0.f};
#pragma unroll
        for (int u = 0; u < MGV; ++u) {
          const int m = gg + G * u;
          const bool ok = gg < G && m < M;
          cfma(acc, cf{ok ? f[2 * u] : 0.f, ok ? f[2 * u + 1] : 0.f}, E0[i * M + min(m, M - 1)]);
        }
        float re = acc.re, im = acc.im;
        for (int q = 1; q < G; ++q) {
          re += __shfl(acc.re, gj + N * q, 64);
          im += __shfl(acc.im, gj + N * q, 64);
        }
        if (gg == 0) A[i * N + gj] = cf{re, im};
      };
      float fa[NF], fb[NF];
      if constexpr (MGV <= 24) {
        ldrow(0, fa);
        for (int i = 0; i < N; i += 2) {
          ldrow(min(i + 1, N - 1), fb);
          contract(i, fa);
          ldrow(min(i + 2, N - 1), fa);
          if (i + 1 < N) contract(i + 1, fb);
        }
      } else {  // (the widest forms: a second set would cost the second wave per SIMD)
        for (int i = 0; i < N; ++i) {
          ldrow(i, fa);
          contract(i, fa);
        }
      }
    }
    sync();
    DET_T(0, 3);
    if (N <= 8 && DET_LU_REG) {  // register LU, one column per lane
      cf col[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) col[r] = (r < N && tid < N) ? A[r * N + tid] : cf{0.f, 0.f};
      const cf l = lu_logdet_cols<8>(col, N, tid, width);
      if (tid == 0) ld[k] = l;
    } else {  // (a 32-row register LU for N = 10, 20 took the C5 form to 256 VGPRs, one wave per SIMD)
      eliminate<Sync, HW>(A, N, N, N, false, fac, piv, logdet, tid, nt, width, sync);
      if (tid == 0) ld[k] = *logdet;
    }
    sync();
    DET_T(0, 4);
  }
  float* lpv = reinterpret_cast<float*>(cart + 3 * N);  // this walker's Re log psi for the epilogue
  if (tid == 0 && live) {
    // log-sum-exp over determinants (psiformer.py:74-76)
    float lmax = -INFINITY;
    for (int k = 0; k < K; ++k) lmax = fmaxf(lmax, ld[k].re);
    float zr = 0.f, zi = 0.f;
    for (int k = 0; k < K; ++k) {
      const float mag = expf(ld[k].re - lmax);
      zr += mag * cosf(ld[k].im);
      zi += mag * sinf(ld[k].im);
    }
    float val_re = 0.5f * logf(zr * zr + zi * zi) + lmax;
    float val_im = atan2f(zi, zr);
    logpsi[2 * b] = val_re + (float)Jw;
    logpsi[2 * b + 1] = val_im;
    *lpv = val_re + (float)Jw;
  }
  DET_T(0, 5);
  if (!epi.on) return;
  // ---- MCMC epilogue (McmcEpi): the accept of epi.step for this walker and its next proposal,
  // lane i < N moving electron i — accept_propose_kernel's arithmetic on the same values
  sync();
  if (!live || tid >= N) return;
  const float lp2 = 2.f * *lpv;
  const bool cond = accept_one(lp2, epi.lp[b], b, N, epi.seed, epi.step, epi.woff, epi.noise);
  const int e = b * N + tid;
  float th = epi.x[2 * e], ph = epi.x[2 * e + 1];
  if (cond) {
    th = x[2 * e];  // x is the proposal this kernel evaluated (epi.x2)
    ph = x[2 * e + 1];
    epi.x[2 * e] = th;
    epi.x[2 * e + 1] = ph;
    if (tid == 0) {
      epi.lp[b] = lp2;
      epi.nacc[b] += 1;
    }
  }
  if (epi.propose)
    propose_one(th, ph, epi.x2, epi.geo, e, b, tid, N, epi.width, epi.seed, epi.step + 1, epi.woff, epi.noise2);
  DET_T(0, 6);
}

}  // namespace dh
