// The per-walker gradient Gram matrix (the neural tangent kernel of log psi) that MinSR solves
// in sample space (api_grad.cpp dh_ntk):
//
//   T[b][b'] = <g_b, g_b'>,  g_b = ct_b.re d Re log psi_b / dp + ct_b.im d Im log psi_b / dp
//
// For a dense map y = [x, 1] [W; bias] the per-walker weight gradient is dW_b = sum_{t in b}
// x~_t dy_t^T over the walker's electron rows t, so
//
//   <dW_b, dW_b'> = sum_{t in b, t' in b'} (x_t . x_t' + 1) (dy_t . dy_t')
//
// — two row-Gram products multiplied element by element and summed over n x n blocks; the
// B x P Jacobian is never formed.  ntk_gram_kernel does that for one map on the layout the
// reverse pass already has (rows = walker x electron, features contiguous), exact f32 MFMA
// (v_mfma_f32_32x32x2_f32, as tn_partial_kernel of grad.hip):
//
//   a workgroup owns the pair (I, J), I <= J, of walker tiles: tw walkers = tw n <= 128 rows
//   each, walker-aligned, rows past the tile / the batch zero-padded, so no walker straddles
//   two workgroups; it forms X_I X_J^T and dY_I dY_J^T in accumulators of the same layout
//   (K streamed through LDS 32 columns at a time), multiplies them, sums each n x n block from
//   LDS in a fixed order and ADDS it into its own entries of T.  Launches of successive maps
//   are ordered by the stream: no atomics, and two calls give bit-identical T.
//
// Precision: the saved activations are LayerNorm outputs whose rows share a large common part
// (x_t . x_t' is about D for every pair) while the tangents of a walker nearly cancel over its
// rows, so the block sum would lose to the f32 rounding of X_I X_J^T what the VJP's X^T dY
// loses to its own.  ntk_centre_kernel therefore takes the batch-mean row m out first:
//   x_t . x_t' + bias = u_t . u_t' + a_t + a_t',  u = x - m,  a_t = m . u_t + (m . m + bias) / 2
// and the kernel contracts the small u rows, adding a_t + a_t' in its epilogue.
//
// Parameters that belong to no dense map (LayerNorm scale / bias, the Jastrow alphas) come as
// explicit per-walker Jacobian rows (n = 1, no dY): T += J J^T by the same kernel.
// ntk_mirror_kernel copies the upper triangle onto the lower one: T is exactly symmetric.
//
// Sharding over ranks (dh_ntk_part): an entry T[wi][wj], wi <= wj, belongs to part
//   owner(wi) = (wi / tw_dense) % nparts,  tw_dense = ntk_tile_walkers(N)
// whatever the launch's own tile size, so that all of an entry's additions happen on one rank
// in the stream's order and the sum of the parts is, bit for bit, the whole.  A dense map's
// workgroup (tile = tw_dense walkers) leaves at once unless its tile row is the part's; a
// per-walker-row launch (tile = 128 walkers) computes its tile and masks the final add.
//
// The Jacobian-vector product (dh_ntk_jvp; SPRING's O phi_prev): jv[b] = <g_b, v> for a parameter
// direction v, by the same identity on the same rows.  With V, v_b the direction's slices for
// the map,
//   <dW_b, V> + <db_b, v_b> = sum_{t in b} (x_t V + v_b) . dy_t
// — one rows x K_in x K_out product, multiplied element by element with dY and summed over
// each walker's rows (ntk_jvp_kernel; a workgroup owns one walker tile and one block of 128
// output columns, and the blocks' sums are added to jv in block order).  It contracts the
// centred rows u = x - m that the Gram launch of the map has just made; the common part goes
// into the per-column constant cvec = m V + v_b (ntk_jvp_cvec_kernel).  The explicit per-walker rows are short dot products
// (ntk_rowdot_kernel).  Linear in v, every sum in a fixed order: jvp(2 v) = 2 jvp(v) bit for bit.
//
// minsr_rowsum / minsr_gsum / minsr_matrix kernels (dh_minsr_matrix): the float64 matrix MinSR
// solves, A = C T C / n + damping I with C the centring over the valid walkers, from the float32
// T in two passes over it and one write of A.
#include "dh_internal.h"
#include "device_common.h"

namespace dh {

typedef float f32x16_n __attribute__((ext_vector_type(16)));

namespace {

constexpr int kNtkKB = 32;       // K columns staged per step
constexpr int kNtkLd = 36;       // LDS row stride of a staged tile (16-B aligned float4 reads)

// Four columns k .. k + 3 of row `row` (zeros where !ok or past K).  VEC: K % 4 == 0, ld % 4 == 0,
// Z 16-byte aligned, so the four are in or out of range together and load as one float4.
template <bool VEC>
__device__ __forceinline__ float4 ntk_load4(const float* __restrict__ Z, int ld, int K, int row, int k, bool ok) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!ok) return v;
  const float* p = Z + (size_t)row * ld + k;
  if (VEC) {
    if (k < K) v = *reinterpret_cast<const float4*>(p);
  } else {
    if (k < K) v.x = p[0];
    if (k + 1 < K) v.y = p[1];
    if (k + 2 < K) v.z = p[2];
    if (k + 3 < K) v.w = p[3];
  }
  return v;
}

// T[wi][wj] += sum_{i, j < n} (X_I X_J^T + a_i + a_j)[bi n + i][bj n + j] (Y_I Y_J^T)[bi n + i][bj n + j]
// for the walker pairs of tile pair (I, J) = (blockIdx.y, blockIdx.x), I <= J; a [rows] per-row
// offsets (null: 0); Y == null: the second factor is 1 (explicit Jacobian rows).  Only entries
// wi <= wj of the rows with (wi / tw_own) % nparts == part are added to (header, "Sharding").
// rows = nwalk * n; tw * n <= kNtkTileRows.  The next 32 columns of both tiles are fetched into
// registers (8 float4 per thread) while the MFMAs of the current ones run.
template <bool VEC>
__global__ __launch_bounds__(256) void ntk_gram_kernel(const float* __restrict__ X, int ldx, int Kx,
                                                       const float* __restrict__ Y, int ldy, int Ky,
                                                       const float* __restrict__ arow, int n, int tw, int nwalk,
                                                       int tw_own, int part, int nparts, float* __restrict__ T) {
  // staging: two [128][kNtkLd] tiles; epilogue: the [128][128] product
  __shared__ float sm[kNtkTileRows * kNtkTileRows];
  const int I = blockIdx.y, J = blockIdx.x;
  if (I > J) return;
  // tw_own: the dense maps' tile, which decides the owner of a row of T (header)
  if (tw == tw_own && I % nparts != part) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  const int tr = tw * n, rows = nwalk * n;
  float* sA = sm;
  float* sB = sm + kNtkTileRows * kNtkLd;
  const int fr = tid >> 3, fc = (tid & 7) * 4;  // this thread's staged rows fr + 32 q, columns fc .. fc + 3
  f32x16_n g[2][2][2];  // [product][row half][column half]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) g[p][a][b][e] = 0.f;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float* Z = p == 0 ? X : Y;
    const int ld = p == 0 ? ldx : ldy, K = p == 0 ? Kx : Ky;
    if (!Z) continue;
    float4 fa[4], fb[4];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = fr + 32 * q, ra = I * tr + r, rb = J * tr + r;
        fa[q] = ntk_load4<VEC>(Z, ld, K, ra, k0 + fc, r < tr && ra < rows);
        fb[q] = ntk_load4<VEC>(Z, ld, K, rb, k0 + fc, r < tr && rb < rows);
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kNtkKB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<float4*>(sA + (fr + 32 * q) * kNtkLd + fc) = fa[q];
        *reinterpret_cast<float4*>(sB + (fr + 32 * q) * kNtkLd + fc) = fb[q];
      }
      __syncthreads();
      if (k0 + kNtkKB < K) fetch(k0 + kNtkKB);
#pragma unroll
      for (int kk = 0; kk < kNtkKB; kk += 8) {
        // lane half lh holds columns kk + 4 lh .. + 3 of its row: MFMA u contracts column
        // kk + u (lh = 0) and kk + 4 + u (lh = 1), the same pairing in A and B
        float4 av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          av[a] = *reinterpret_cast<const float4*>(sA + (wr + 32 * a + l32) * kNtkLd + kk + 4 * lh);
          bv[a] = *reinterpret_cast<const float4*>(sB + (wc + 32 * a + l32) * kNtkLd + kk + 4 * lh);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const float x = u == 0 ? av[a].x : u == 1 ? av[a].y : u == 2 ? av[a].z : av[a].w;
              const float y = u == 0 ? bv[b].x : u == 1 ? bv[b].y : u == 2 ? bv[b].z : bv[b].w;
              g[p][a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, g[p][a][b], 0, 0, 0);
            }
      }
    }
  }
  // product into LDS; C/D map: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).
  // Padded rows have dY = 0 (or, without Y, X = 0) and offset 0: their products are 0.
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int c = wc + 32 * b + l32;
      const float ac = (arow && c < tr && J * tr + c < rows) ? arow[J * tr + c] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = wr + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * lh;
        const float ar = (arow && r < tr && I * tr + r < rows) ? arow[I * tr + r] : 0.f;
        const float g1 = g[0][a][b][e] + (ar + ac);
        sm[r * kNtkTileRows + c] = Y ? g1 * g[1][a][b][e] : g1;
      }
    }
  __syncthreads();
  // a dense map's workgroup owns all of its tile row or has left already
  const bool masked = nparts > 1 && tw != tw_own;
  for (int p = tid; p < tw * tw; p += 256) {
    const int bi = p / tw, bj = p - bi * tw;
    const int wi = I * tw + bi, wj = J * tw + bj;
    // (a diagonal tile pair's lower half is the mirror's to fill)
    if (wi >= nwalk || wj >= nwalk || wi > wj || (masked && (wi / tw_own) % nparts != part)) continue;
    float s = 0.f;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) s += sm[(bi * n + i) * kNtkTileRows + bj * n + j];
    T[(size_t)wi * nwalk + wj] += s;
  }
}

constexpr int kJvpCols = 128;    // output columns per block of the JVP kernel
constexpr int kJvpLdV = 136;     // LDS row stride of the staged V panel: rows k and k + 4 lie 32 banks apart
constexpr int kJvpLdR = 65;      // row stride of the final [128][64] reduction image

// part[blockIdx.y][w] = sum_{t in w} sum_c ((X V)[t][c] + cvec[c]) dY[t][c] over the 128 columns
// c of block blockIdx.y, for the tw walkers of tile blockIdx.x (header, "The Jacobian-vector
// product"): X [rows][K], V [K][Ky] (row stride ldv), cvec [Ky] (null: 0), dY [rows][Ky], part
// [ceil(Ky / 128)][nwalk].  The workgroup streams K through LDS 32 columns at a time (the X tile as
// the Gram kernel stages it, the V panel [32][128] as it lies), the next step fetched into
// registers under the current MFMAs, and multiplies the 128 x 128 product by dY in registers,
// one partial sum per accumulator row and lane.  Rows past the tile / the batch and columns past
// Ky contribute 0.  The 64 partials of a row (2 waves x 32 lanes) are summed from LDS in a fixed
// order, then each walker's n rows.  Every column block has its own workgroup whatever the
// batch — a small batch still fills the machine, and the sum over the blocks
// (ntk_jvp_reduce_kernel, block order) does not depend on how they were scheduled: no atomics.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void ntk_jvp_kernel(const float* __restrict__ X, int ldx, int K,
                                                         const float* __restrict__ V, int ldv,
                                                         const float* __restrict__ cvec,
                                                         const float* __restrict__ dY, int ldy, int Ky, int n,
                                                         int tw, int nwalk, float* __restrict__ part) {
  // staging: the X tile [128][kNtkLd] and the V panel [32][kJvpLdV]; at the end the [128][kJvpLdR] image
  __shared__ float sm[kNtkTileRows * kNtkLd + kNtkKB * kJvpLdV];
  __shared__ float srow[kNtkTileRows];
  static_assert(kNtkTileRows * kJvpLdR <= kNtkTileRows * kNtkLd + kNtkKB * kJvpLdV, "reduction image fits");
  const int I = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
  const int tr = tw * n, rows = nwalk * n;
  const int nval = min(tr, rows - I * tr);  // rows of this tile that exist
  float* sA = sm;
  float* sV = sm + kNtkTileRows * kNtkLd;
  const int fr = tid >> 3, fc = (tid & 7) * 4;    // X: rows fr + 32 q, columns fc .. fc + 3 of the step
  const int vr = tid >> 5, vc = (tid & 31) * 4;   // V: rows vr + 8 q of the step, columns vc .. vc + 3 of the block
  float rs[2][16];  // this lane's partial of row wr + 32 a + (e & 3) + 8 (e >> 2) + 4 lh
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) rs[a][e] = 0.f;
  const int c0 = blockIdx.y * kJvpCols;
  {
    f32x16_n g[2][2];  // [row half][column half]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) g[a][b][e] = 0.f;
    float4 fa[4], fv[4];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = fr + 32 * q, ra = I * tr + r, kv = k0 + vr + 8 * q;
        fa[q] = ntk_load4<VEC>(X, ldx, K, ra, k0 + fc, r < tr && ra < rows);
        fv[q] = ntk_load4<VEC>(V, ldv, Ky, kv, c0 + vc, kv < K);
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kNtkKB) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        *reinterpret_cast<float4*>(sA + (fr + 32 * q) * kNtkLd + fc) = fa[q];
        *reinterpret_cast<float4*>(sV + (vr + 8 * q) * kJvpLdV + vc) = fv[q];
      }
      __syncthreads();
      if (k0 + kNtkKB < K) fetch(k0 + kNtkKB);
#pragma unroll
      for (int kk = 0; kk < kNtkKB; kk += 8) {
        // as the Gram kernel: MFMA u contracts column kk + u (lh = 0) and kk + 4 + u (lh = 1) of X
        // with the same rows of V; a lane's B operand is V[k][its column], one float
        float4 av[2];
        float bv[4][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
          av[a] = *reinterpret_cast<const float4*>(sA + (wr + 32 * a + l32) * kNtkLd + kk + 4 * lh);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int b = 0; b < 2; ++b) bv[u][b] = sV[(kk + 4 * lh + u) * kJvpLdV + wc + 32 * b + l32];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const float x = u == 0 ? av[a].x : u == 1 ? av[a].y : u == 2 ? av[a].z : av[a].w;
              g[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, bv[u][b], g[a][b], 0, 0, 0);
            }
      }
    }
    // C/D map: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int c = c0 + wc + 32 * b + l32;
      const bool cok = c < Ky;
      const float cv = (cvec && cok) ? cvec[c] : 0.f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int r0 = wr + 32 * a + 4 * lh;
        const float* py = dY + (size_t)(I * tr + r0) * ldy + c;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int ro = (e & 3) + 8 * (e >> 2);
          const float dy = (cok && r0 + ro < nval) ? py[(size_t)ro * ldy] : 0.f;
          rs[a][e] = fmaf(g[a][b][e] + cv, dy, rs[a][e]);
        }
        // one accumulator's 16 loads in flight at a time: hoisting all 64 spilled
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      sm[(wr + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * lh) * kJvpLdR + (w & 1) * 32 + l32] = rs[a][e];
  __syncthreads();
  if (tid < kNtkTileRows) {
    float s = 0.f;
    for (int j = 0; j < 64; ++j) s += sm[tid * kJvpLdR + j];
    srow[tid] = s;
  }
  __syncthreads();
  const int wi = I * tw + tid;
  if (tid < tw && wi < nwalk) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += srow[tid * n + i];
    part[(size_t)blockIdx.y * nwalk + wi] = s;
  }
}

// jv[w] += sum_{cb < ncb} part[cb][w], cb ascending
__global__ __launch_bounds__(256) void ntk_jvp_reduce_kernel(const float* __restrict__ part, int ncb, int nwalk,
                                                             float* __restrict__ jv) {
  const int wi = blockIdx.x * 256 + threadIdx.x;
  if (wi >= nwalk) return;
  float s = 0.f;
  for (int cb = 0; cb < ncb; ++cb) s += part[(size_t)cb * nwalk + wi];
  jv[wi] += s;
}

// cvec[c] = b[c] (null: 0) + sum_k m[k] V[k][c] (m null: the bias alone).  64 columns per
// workgroup; wave q sums the rows k = q, q + 4, .. in ascending order (loads batched eight at a
// time: one thread per column over all of K waited 100 us on its own load latencies), the four
// partials are added in wave order
__global__ __launch_bounds__(256) void ntk_jvp_cvec_kernel(const float* __restrict__ m, int K,
                                                           const float* __restrict__ V, int ldv,
                                                           const float* __restrict__ b, int Ky,
                                                           float* __restrict__ cvec) {
  __shared__ float red[4][64];
  const int q = threadIdx.x >> 6, cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl;
  float s = 0.f;
  if (m && c < Ky) {
#pragma unroll 8
    for (int k = q; k < K; k += 4) s = fmaf(m[k], V[(size_t)k * ldv + c], s);
  }
  red[q][cl] = s;
  __syncthreads();
  if (q == 0 && c < Ky) cvec[c] = (b ? b[c] : 0.f) + (((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl]);
}

// jv[w] += sum_{k < ka} J[w][k] va[k] + sum_{k < kb} J[w][ka + k] vb[k]: explicit per-walker
// tangent rows against their two slices of the direction; one wave per walker, each lane's
// columns in ascending order, then the butterfly
__global__ __launch_bounds__(256) void ntk_rowdot_kernel(const float* __restrict__ J, int ldj,
                                                         const float* __restrict__ va, int ka,
                                                         const float* __restrict__ vb, int kb, int nwalk,
                                                         float* __restrict__ jv) {
  const int wi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wi >= nwalk) return;
  const float* Jr = J + (size_t)wi * ldj;
  float s = 0.f;
  for (int k = lane; k < ka; k += 64) s = fmaf(Jr[k], va[k], s);
  for (int k = lane; k < kb; k += 64) s = fmaf(Jr[ka + k], vb[k], s);
  s = wave_sum(s);
  if (lane == 0) jv[wi] += s;
}

// U[r][k] = X[r][k] - m[k] (row stride K) and a[r] = m . U[r] + (m . m + bias) / 2; one wave per row
__global__ __launch_bounds__(256) void ntk_centre_kernel(const float* __restrict__ X, int ldx, int K,
                                                         const float* __restrict__ m, float bias, int rows,
                                                         float* __restrict__ U, float* __restrict__ a) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  float mu = 0.f, mm = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float mk = m[k], u = X[(size_t)r * ldx + k] - mk;
    U[(size_t)r * K + k] = u;
    mu = fmaf(mk, u, mu);
    mm = fmaf(mk, mk, mm);
  }
  mu = wave_sum(mu);
  mm = wave_sum(mm);
  if (lane == 0) a[r] = mu + 0.5f * (mm + bias);
}

// T[j][i] = T[i][j], i < j
__global__ __launch_bounds__(256) void ntk_mirror_kernel(float* __restrict__ T, int B) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * B) return;
  const int j = (int)(idx / B), i = (int)(idx % B);
  if (i < j) T[idx] = T[(size_t)i * B + j];
}

// out[b] = ct[b] where log psi_b is finite, else 0 (psi = 0: the walker has no tangent)
__global__ __launch_bounds__(256) void ntk_mask_ct_kernel(const float* __restrict__ logpsi,
                                                          const float* __restrict__ ct, float* __restrict__ out,
                                                          int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const bool ok = isfinite(logpsi[2 * b]) && isfinite(logpsi[2 * b + 1]);
  out[2 * b] = ok ? ct[2 * b] : 0.f;
  out[2 * b + 1] = ok ? ct[2 * b + 1] : 0.f;
}

// the input features [cos th, sin th cos ph, sin th sin ph, s] (psiformer.py:51-60) of every
// row from geo = (sin th, cos th, sin ph, cos ph), as w0_partial_kernel forms them
__global__ __launch_bounds__(256) void ntk_features_kernel(const float* __restrict__ geo, int rows, int N, int n_up,
                                                           float* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float4 g = *reinterpret_cast<const float4*>(geo + 4 * (size_t)r);
  *reinterpret_cast<float4*>(out + 4 * (size_t)r) =
      make_float4(g.y, g.x * g.w, g.x * g.z, ((r % N) < n_up) ? 1.f : -1.f);
}

// ---- dh_minsr_matrix.  Rows (a, i), columns (c, j) of T [M][M], M = 2 Bg; halves a, c; walkers
// i, j; v the valid flags, n = max(1, sum v).  Workspace (doubles): s [M][2], the row sums and
// then r = s / n | g [4] | n.

// sum over 256 threads' doubles in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double minsr_block_sum(double x, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = x;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// pass 1: s[row][c] = sum_j v_j T[row][c Bg + j] (not yet / n); one workgroup per row, each
// thread's columns in a fixed order, then the fixed tree
template <bool VEC>
__global__ __launch_bounds__(256) void minsr_rowsum_kernel(const float* __restrict__ T,
                                                           const unsigned char* __restrict__ valid, int Bg,
                                                           double* __restrict__ s) {
  __shared__ double red[256];
  const int M = 2 * Bg, row = blockIdx.x, tid = threadIdx.x;
  const float* Tr = T + (size_t)row * M;
  double acc[2] = {0.0, 0.0};
  if (VEC) {
    for (int j0 = 4 * tid; j0 < M; j0 += 1024) {
      const float4 t = *reinterpret_cast<const float4*>(Tr + j0);
      const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u, c = j >= Bg;
        const double x = valid[j - c * Bg] ? (double)tv[u] : 0.0;
        acc[0] += c ? 0.0 : x;
        acc[1] += c ? x : 0.0;
      }
    }
  } else {
    for (int j = tid; j < M; j += 256) {
      const int c = j >= Bg;
      const double x = valid[j - c * Bg] ? (double)Tr[j] : 0.0;
      acc[0] += c ? 0.0 : x;
      acc[1] += c ? x : 0.0;
    }
  }
  const double s0 = minsr_block_sum(acc[0], red);
  const double s1 = minsr_block_sum(acc[1], red);
  if (tid == 0) {
    s[2 * (size_t)row] = s0;
    s[2 * (size_t)row + 1] = s1;
  }
}

// n and g[a][c] = sum_i v_i s[(a, i)][c] / n^2, then s /= n in place (one workgroup).  g[0][1] and
// g[1][0] are the same number summed in two orders: g[1][0] is stored as g[0][1], so that A is
// exactly symmetric.
__global__ __launch_bounds__(256) void minsr_gsum_kernel(const unsigned char* __restrict__ valid, int Bg,
                                                         double* __restrict__ s, double* __restrict__ g) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double cnt = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < Bg; i += 256) {
    if (!valid[i]) continue;
    cnt += 1.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[2 * a + c] += s[2 * ((size_t)a * Bg + i) + c];
  }
  double n = minsr_block_sum(cnt, red);
  double tot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tot[k] = minsr_block_sum(acc[k], red);
  n = n < 1.0 ? 1.0 : n;
  for (size_t k = tid; k < 4 * (size_t)Bg; k += 256) s[k] /= n;  // every read of s above is behind a barrier
  if (tid == 0) {
    g[0] = tot[0] / n / n;
    g[1] = g[2] = tot[1] / n / n;
    g[3] = tot[3] / n / n;
    g[4] = n;
  }
}

// pass 2: A[(a,i)][(c,j)] = v_i v_j (T - (r[(a,i)][c] + r[(c,j)][a]) + g[a][c]) / n + damping [row == col];
// one workgroup per row, two columns per thread and step: a wave reads 512 and writes 1024
// contiguous bytes per instruction (float4 in and two double2 out per thread left every store
// instruction with 16-byte holes: 1.40 ms against 1.22 ms at M = 16384).  A is not read again
// before the solve, so its stores are nontemporal and leave T in the Infinity Cache for the rows
// that follow (M = 8192: 0.29 -> 0.17 ms)
template <bool VEC>
__global__ __launch_bounds__(256) void minsr_matrix_kernel(const float* __restrict__ T,
                                                           const unsigned char* __restrict__ valid, int Bg,
                                                           double damping, const double* __restrict__ r,
                                                           const double* __restrict__ g, double* __restrict__ A) {
  const int M = 2 * Bg, row = blockIdx.x, tid = threadIdx.x;
  const int a = row >= Bg;
  const bool vi = valid[row - a * Bg] != 0;
  const double n = g[4];
  const double ri[2] = {r[2 * (size_t)row], r[2 * (size_t)row + 1]};
  const double ga[2] = {g[2 * a], g[2 * a + 1]};
  const float* Tr = T + (size_t)row * M;
  double* Ar = A + (size_t)row * M;
  auto entry = [&](int j, float t, bool vj, double rj) {
    const int c = j >= Bg;
    const double x = vi && vj ? (((double)t - (ri[c] + rj)) + ga[c]) / n : 0.0;
    return j == row ? x + damping : x;
  };
  if (VEC) {
    typedef double d2_t __attribute__((ext_vector_type(2)));
    for (int j0 = 2 * tid; j0 < M; j0 += 512) {
      const float2 t = *reinterpret_cast<const float2*>(Tr + j0);
      bool vj[2];
      double rj[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = j0 + u;
        vj[u] = valid[j >= Bg ? j - Bg : j] != 0;
        rj[u] = r[2 * (size_t)j + a];
      }
      d2_t o;
      o.x = entry(j0, t.x, vj[0], rj[0]);
      o.y = entry(j0 + 1, t.y, vj[1], rj[1]);
      __builtin_nontemporal_store(o, reinterpret_cast<d2_t*>(Ar + j0));
    }
  } else {
    for (int j = tid; j < M; j += 256) Ar[j] = entry(j, Tr[j], valid[j >= Bg ? j - Bg : j] != 0, r[2 * (size_t)j + a]);
  }
}

}  // namespace

int ntk_tile_walkers(int N) { return N >= 1 && N <= kNtkTileRows ? kNtkTileRows / N : 0; }

int ntk_jvp_col_blocks(int Ky) { return (Ky + kJvpCols - 1) / kJvpCols; }

void launch_ntk_gram(const float* X, int ldx, int Kx, const float* Y, int ldy, int Ky, const float* arow, int n,
                     int nwalk, int tw_own, int part, int nparts, float* T, hipStream_t s) {
  const int tw = ntk_tile_walkers(n);
  if (tw < 1 || nwalk < 1) return;
  const int nt = (nwalk + tw - 1) / tw;
  auto vec_ok = [](const float* Z, int ld, int K) {
    return !Z || (K % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(Z) % 16 == 0);
  };
  if (vec_ok(X, ldx, Kx) && vec_ok(Y, ldy, Ky))
    hipLaunchKernelGGL(ntk_gram_kernel<true>, dim3(nt, nt), dim3(256), 0, s, X, ldx, Kx, Y, ldy, Ky, arow, n, tw,
                       nwalk, tw_own, part, nparts, T);
  else
    hipLaunchKernelGGL(ntk_gram_kernel<false>, dim3(nt, nt), dim3(256), 0, s, X, ldx, Kx, Y, ldy, Ky, arow, n, tw,
                       nwalk, tw_own, part, nparts, T);
}

void launch_ntk_centre(const float* X, int ldx, int K, const float* mean, bool bias, int rows, float* U, float* a,
                       hipStream_t s) {
  hipLaunchKernelGGL(ntk_centre_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, X, ldx, K, mean, bias ? 1.f : 0.f,
                     rows, U, a);
}

void launch_ntk_jvp(const float* X, int ldx, int K, const float* V, int ldv, const float* cvec, const float* dY,
                    int ldy, int Ky, int n, int nwalk, float* part, float* jv, hipStream_t s) {
  const int tw = ntk_tile_walkers(n);
  if (tw < 1 || nwalk < 1 || K < 1 || Ky < 1) return;
  const int nt = (nwalk + tw - 1) / tw, ncb = ntk_jvp_col_blocks(Ky);
  auto vec_ok = [](const float* Z, int ld, int Kz) {
    return Kz % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(Z) % 16 == 0;
  };
  if (vec_ok(X, ldx, K) && vec_ok(V, ldv, Ky))
    hipLaunchKernelGGL(ntk_jvp_kernel<true>, dim3(nt, ncb), dim3(256), 0, s, X, ldx, K, V, ldv, cvec, dY, ldy, Ky, n,
                       tw, nwalk, part);
  else
    hipLaunchKernelGGL(ntk_jvp_kernel<false>, dim3(nt, ncb), dim3(256), 0, s, X, ldx, K, V, ldv, cvec, dY, ldy, Ky, n,
                       tw, nwalk, part);
  hipLaunchKernelGGL(ntk_jvp_reduce_kernel, dim3((nwalk + 255) / 256), dim3(256), 0, s, part, ncb, nwalk, jv);
}

void launch_ntk_jvp_cvec(const float* mean, int K, const float* V, int ldv, const float* bias, int Ky, float* cvec,
                         hipStream_t s) {
  hipLaunchKernelGGL(ntk_jvp_cvec_kernel, dim3((Ky + 63) / 64), dim3(256), 0, s, mean, K, V, ldv, bias, Ky, cvec);
}

void launch_ntk_rowdot(const float* J, int ldj, const float* va, int ka, const float* vb, int kb, int nwalk, float* jv,
                       hipStream_t s) {
  if (nwalk < 1) return;
  hipLaunchKernelGGL(ntk_rowdot_kernel, dim3((nwalk + 3) / 4), dim3(256), 0, s, J, ldj, va, ka, vb, kb, nwalk, jv);
}

void launch_ntk_mirror(float* T, int B, hipStream_t s) {
  const size_t n = (size_t)B * B;
  hipLaunchKernelGGL(ntk_mirror_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, T, B);
}

size_t minsr_matrix_ws_doubles(int Bg) { return 4 * (size_t)Bg + 8; }

void launch_minsr_matrix(const float* T, const unsigned char* valid, int Bg, double damping, double* A, double* ws,
                         hipStream_t s) {
  const int M = 2 * Bg;
  double* rs = ws;
  double* g = ws + 2 * (size_t)M;
  const bool vec = Bg % 2 == 0 && reinterpret_cast<uintptr_t>(T) % 16 == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(minsr_rowsum_kernel<true>, dim3(M), dim3(256), 0, s, T, valid, Bg, rs);
  else
    hipLaunchKernelGGL(minsr_rowsum_kernel<false>, dim3(M), dim3(256), 0, s, T, valid, Bg, rs);
  hipLaunchKernelGGL(minsr_gsum_kernel, dim3(1), dim3(256), 0, s, valid, Bg, rs, g);
  if (vec)
    hipLaunchKernelGGL(minsr_matrix_kernel<true>, dim3(M), dim3(256), 0, s, T, valid, Bg, damping, rs, g, A);
  else
    hipLaunchKernelGGL(minsr_matrix_kernel<false>, dim3(M), dim3(256), 0, s, T, valid, Bg, damping, rs, g, A);
}

void launch_ntk_mask_ct(const float* logpsi, const float* ct, float* out, int B, hipStream_t s) {
  hipLaunchKernelGGL(ntk_mask_ct_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logpsi, ct, out, B);
}

void launch_ntk_features(const Dims& d, const float* geo, int rows, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ntk_features_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, geo, rows, d.N, d.n_up, out);
}

}  // namespace dh
