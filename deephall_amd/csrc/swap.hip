// Swap estimator of the Renyi-2 entanglement entropy of a spherical cap (netobs/observables/
// renyi2.py; not in the reference).  Walkers x[B][N][2] (theta, phi), P = B / 2 pairs: pair p is
// (R1, R2) = (walker p, walker p + P), an odd last walker is ignored.  Region A_a is the cap
// theta < theta_a of A angles; the slots below n_up are up electrons.  "In A" is everywhere the
// float32 comparison x[..][0] < theta_a on the stored value, so the kernels agree with each other
// and with a numpy restatement bit for bit (a NaN theta is outside every cap).
//
//   classify  one thread per (a, p): the up / down counts in A of both members; the sector
//             k = nA_up (n_dn + 1) + nA_dn of each member is added to counts[A][K] (integer
//             atomics), sector[a P + p] = k when both counts agree (the pair is matched), else -1.
//   scan      exclusive prefix sum of the matched flags in flattened (a-major, then p) order:
//             row[a P + p] = the output row o of a matched pair, start[a] = the first row of
//             angle a, start[A] = M.  One workgroup walks the flags in tiles of 1024 (ballot +
//             popcount per wave, the 16 wave totals in order): no atomic counter, so the rows
//             are the same on every call.
//   gather    one thread per (a, p, member): xs[2 o + member] = the member with the coordinates
//             of its in-A slots, in ascending slot order within each spin, replaced by the
//             partner's in-A coordinates in ascending slot order; pair[o] = a P + p.
//             Coordinates are copied, never recomputed.
//   reduce    sums[a][k] = sum over the matched pairs of angle a in sector k of
//             exp(log psi(R1') + log psi(R2') - log psi(R1) - log psi(R2)), complex, in double from
//             the float32 logs on (amp_ratio).  One workgroup per (a, k) walks the rows of angle a:
//             each thread its strided rows in order, a wave by xor shuffles, then thread q adds
//             component q of the waves in order (the estimators' convention, estimator_common.h).
//             An (a, k) without a matched pair writes zeros.
//
// Only about 40 % of the pairs match, and every row that reaches dh_logpsi costs a
// full forward pass: hence the compaction between classify and the wavefunction call.
// Every grid below has at least one block whenever B >= 2 and A >= 1, which the C entry points
// check first; M = 0 and an angle without matches need no launch of their own.
#include "dh_internal.h"
#include "estimator_common.h"

namespace dh {
namespace {

constexpr int kScanNT = 1024;
constexpr int kScanNW = kScanNT / 64;
constexpr int kRedNT = 256;
constexpr int kRedNW = kRedNT / 64;

// the number of slots [lo, hi) of walker xb inside the cap theta < th
__device__ __forceinline__ int count_in(const float* __restrict__ xb, int lo, int hi, float th) {
  int n = 0;
  for (int i = lo; i < hi; ++i) n += xb[2 * i] < th ? 1 : 0;
  return n;
}

__global__ __launch_bounds__(256) void swap_classify_kernel(const float* __restrict__ x, int P, int N, int n_up,
                                                            SwapThetas th, int A, int32_t* __restrict__ sector,
                                                            int32_t* __restrict__ counts) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= A * P) return;
  const int a = idx / P, p = idx - a * P;
  const int n_dn = N - n_up, K = (n_up + 1) * (n_dn + 1);
  const float t = th.t[a];
  const float* x1 = x + (size_t)p * N * 2;
  const float* x2 = x + (size_t)(p + P) * N * 2;
  const int k1 = count_in(x1, 0, n_up, t) * (n_dn + 1) + count_in(x1, n_up, N, t);
  const int k2 = count_in(x2, 0, n_up, t) * (n_dn + 1) + count_in(x2, n_up, N, t);
  // k = u (n_dn + 1) + d with d <= n_dn is one-to-one in (u, d): k1 == k2 means both counts agree
  sector[idx] = k1 == k2 ? k1 : -1;
  atomicAdd(counts + (size_t)a * K + k1, 1);
  atomicAdd(counts + (size_t)a * K + k2, 1);
}

// one workgroup; n = A P flags
__global__ __launch_bounds__(kScanNT) void swap_scan_kernel(const int32_t* __restrict__ sector, int n, int P, int A,
                                                            int32_t* __restrict__ row, int32_t* __restrict__ start) {
  __shared__ int wtot[kScanNW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;  // matched pairs before this tile
  for (int t0 = 0; t0 < n; t0 += kScanNT) {
    const int idx = t0 + tid;
    const bool m = idx < n && sector[idx] >= 0;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) wtot[w] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int j = 0; j < kScanNW; ++j) {
      if (j < w) off += wtot[j];
      tot += wtot[j];
    }
    off += __popcll(bal & ((1ull << lane) - 1ull));
    if (idx < n) {
      row[idx] = m ? off : -1;
      if (idx % P == 0) start[idx / P] = off;
    }
    base += tot;
    __syncthreads();  // wtot is rewritten by the next tile
  }
  if (tid == 0) start[A] = base;
}

__global__ __launch_bounds__(256) void swap_gather_kernel(const float* __restrict__ x, int P, int N, int n_up,
                                                          SwapThetas th, int A, const int32_t* __restrict__ row,
                                                          int32_t* __restrict__ pair, float* __restrict__ xs) {
  const int tix = blockIdx.x * 256 + threadIdx.x;
  if (tix >= 2 * A * P) return;
  const int idx = tix >> 1, member = tix & 1;
  const int o = row[idx];
  if (o < 0) return;  // unmatched; o < A P, the rows the caller's xs holds
  const int a = idx / P, p = idx - a * P;
  const float t = th.t[a];
  const float2* self = reinterpret_cast<const float2*>(x) + (size_t)(member ? p + P : p) * N;
  const float2* other = reinterpret_cast<const float2*>(x) + (size_t)(member ? p : p + P) * N;
  float2* out = reinterpret_cast<float2*>(xs) + ((size_t)2 * o + member) * N;
  for (int s = 0; s < 2; ++s) {
    const int lo = s ? n_up : 0, hi = s ? N : n_up;
    int j = lo;  // the partner's next in-A slot of this spin
    for (int i = lo; i < hi; ++i) {
      float2 v = self[i];
      if (v.x < t) {
        while (j < hi && !(other[j].x < t)) ++j;
        if (j < hi) v = other[j++];  // always, for a matched pair
      }
      out[i] = v;
    }
  }
  if (member == 0) pair[o] = idx;
}

// one workgroup per (a, k)
__global__ __launch_bounds__(kRedNT) void swap_reduce_kernel(const float* __restrict__ lp,
                                                             const float* __restrict__ lps, int P, int K, int M,
                                                             const int32_t* __restrict__ pair,
                                                             const int32_t* __restrict__ sector,
                                                             const int32_t* __restrict__ start,
                                                             double* __restrict__ sums) {
  __shared__ double wsum[kRedNW][2];
  const int a = blockIdx.x / K, k = blockIdx.x - a * K;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // start and pair are the caller's memory: nothing they hold takes a read out of the buffers
  // (pair[M], logpsi_s[2 M]; with M = 0 no row is read)
  const int o0 = max(start[a], 0), o1 = min(start[a + 1], M);
  double sr = 0.0, si = 0.0;
  for (int o = o0 + tid; o < o1; o += kRedNT) {
    const int idx = pair[o];
    if (idx < a * P || idx >= (a + 1) * P || sector[idx] != k) continue;
    const int p = idx - a * P;
    const float* l1 = lp + 2 * (size_t)p;
    const float* l2 = lp + 2 * (size_t)(p + P);
    const float* s1 = lps + 4 * (size_t)o;  // rows 2 o and 2 o + 1
    const double dr = ((double)s1[0] + (double)s1[2]) - ((double)l1[0] + (double)l2[0]);
    const double di = ((double)s1[1] + (double)s1[3]) - ((double)l1[1] + (double)l2[1]);
    const double2 r = amp_ratio(dr, di);
    sr += r.x;
    si += r.y;
  }
  for (int off = 32; off > 0; off >>= 1) {
    sr += __shfl_xor(sr, off, 64);
    si += __shfl_xor(si, off, 64);
  }
  if (lane == 0) {
    wsum[w][0] = sr;
    wsum[w][1] = si;
  }
  __syncthreads();
  if (tid < 2) {
    double t = 0.0;
    for (int j = 0; j < kRedNW; ++j) t += wsum[j][tid];
    sums[2 * (size_t)blockIdx.x + tid] = t;
  }
}

}  // namespace

void launch_swap_classify(const float* x, int B, int N, int n_up, const SwapThetas& th, int A, int32_t* sector,
                          int32_t* counts, hipStream_t s) {
  const int P = B / 2, n = A * P;  // n >= 1: B >= 2, A >= 1
  hipLaunchKernelGGL(swap_classify_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, P, N, n_up, th, A, sector,
                     counts);
}

void launch_swap_compact(const float* x, int B, int N, int n_up, const SwapThetas& th, int A, const int32_t* sector,
                         int32_t* row, int32_t* start, int32_t* pair, float* xs, hipStream_t s) {
  const int P = B / 2, n = A * P;
  hipLaunchKernelGGL(swap_scan_kernel, dim3(1), dim3(kScanNT), 0, s, sector, n, P, A, row, start);
  // one thread per (a, p, member), matched or not: the grid does not depend on M
  hipLaunchKernelGGL(swap_gather_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, s, x, P, N, n_up, th, A, row,
                     pair, xs);
}

void launch_swap_reduce(const float* logpsi, const float* logpsi_s, int B, int K, int A, int M, const int32_t* pair,
                        const int32_t* sector, const int32_t* start, double* sums, hipStream_t s) {
  // A K >= 1 blocks whatever M is: every (a, k) writes its sum, zeros where nothing matched
  hipLaunchKernelGGL(swap_reduce_kernel, dim3(A * K), dim3(kRedNT), 0, s, logpsi, logpsi_s, B / 2, K, M, pair,
                     sector, start, sums);
}

}  // namespace dh
