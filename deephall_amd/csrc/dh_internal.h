// Internal declarations shared by the HIP kernel files and the C ABI (api.cpp, api_grad.cpp).
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/deephall_amd.h"

namespace dh {

// Static network geometry derived from dh_config (all sizes in elements).
struct Dims {
  int N, n_up, n_dn;   // electrons
  int T;               // 2N first-order tangent channels
  int C;               // 2N + 5 channels (local energy)
  int M;               // 2Q + 1 monopole harmonics
  float Q, r;          // monopole strength, sphere radius
  int H, dh, D, L, K;  // heads, head dim, model dim, layers, determinants
  int NB;              // spin blocks of the orbital layer (1 or 2)
  int orb_cols;        // NB * 2 * M * N * K
  int ld_orb;          // orb_cols rounded up to 128
  int interaction;     // DH_INTERACTION_*
  float lambda;        // interaction strength
  int sparse;          // orbital type "sparse": F = 8 features per (j, k) (blocks.py:52-62)
};
constexpr int kSparseFeatures = 8;
constexpr int kMqkStride = 32;  // floats per head of layer 1's score forms Mqk (25 used; attn_val.h)

// Device pointers into the packed parameter buffer.
struct LayerParams {
  const float *Wqkv, *bqkv, *Wol, *bol, *ln1, *Wm, *bm, *ln2;
  // backward (x^T-side) copies of the same weights for dX = dY W^T: split-bf16 planes of the
  // untransposed W (x6 path) or W^T [ncols][D] (exact-f32 path)
  const uint16_t *WqkvB, *WolB, *WmB;
  const float *WqkvBT, *WolBT, *WmBT;
  const float *WqkvT, *WolT, *WmT;  // transposed copies [ncols pad 256][D] for the NT GEMM
  const uint16_t *WqkvP, *WolP, *WmP;  // split-bf16 planes [3][x6_plane_rows(ncols)][D] (gemm_x6)
};
struct Params {
  const float* W0;
  LayerParams layer[16];
  const float *Worb, *borb, *jastrow;
  const float* W0qkv;  // [4][3D] = W0 @ Wqkv of layer 0 (folded at packing)
  const float* WorbT;  // [orb_cols pad 256][D]
  const uint16_t* WorbP;  // split-bf16 planes of Worb
  const uint16_t* WorbB;  // backward planes (untransposed Worb [D][ld_orb])
  const float* WorbBT;    // backward exact-f32 copy Worb^T [ld_orb][D]
  const float* Mqk;       // layer 1's score forms Wq~ Wk~^T / 8, [H][kMqkStride] (attn_val.h)
  // layer 1's output map in feature space (round 6): U^T [n < D, pad 256][k < ofeat_k] with
  // U[8 h + a][n] = sum_d Wv~[a][h dh + d] Wol[h dh + d][n] (a < 5; a = 5..7 zero), and its planes
  const float* UT;
  const uint16_t* UP;
  // layer 1 in coefficient space (gemm_lnch MODE 2, H = 4): planes of V^T and B^T [3][ldp][32],
  // and V^T [256][32] itself (layer1_ch_kernel, N = 10, 20)
  const uint16_t *L1VP, *L1BP;
  const float* L1VT;
  const float* W2T;     // envelope first (env_first): W2T [256 2N][KE] and its planes
  const uint16_t* W2P;
};
// Layer 1's attention output in feature space (attention.hip feat2, the chain prologue): per
// row o~ [ofeat_k] = per head h the five sums o~_h[a] = sum_j A_ij f~_j[a] (f~ = (z, x, y,
// spin, 1)) at columns 8 h + a, zeros elsewhere, so o = o~_h Wv~ and o Wol = o~ U (K = ofeat_k)
inline int ofeat_k(const Dims& d) { return (8 * d.H + 31) / 32 * 32; }

// Channel bookkeeping for one pass: C = 1 (log psi only) or 2N+5 (local energy).
struct Pass {
  int nw;      // walkers in this pass
  int C;       // channels
  int rows;    // nw * N * C
  int rows_pad;
};

// Which launches make up one Psiformer pass (DESIGN.md §1 "Routes"): decided once per pass by
// trunk_route (trunk_route.cpp; host only: no device call, no allocation), then walked by
// run_trunk, carve, dh_local_energy and the debug hooks (api.cpp).  dh_debug_route writes the
// fields as ints in the order they stand here.
enum GemmFamily : int { GEMM_F32_NN = 0, GEMM_F32_NT = 1, GEMM_X6 = 2 };  // exact f32 (W / W^T) or split-bf16
enum LayerForm : int {
  LF_SEPARATE = 0,  // GEMM, LayerNorm, GEMM, LayerNorm: four launches
  LF_LN_EPILOGUE,   // log psi: two GEMMs with the LayerNorm in their epilogue (gemm_x6_ln / gemm_ln by family)
  LF_CHAIN,         // log psi: launch_chain_x6, the two LayerNorm GEMMs and the next linear map in one launch
  LF_CHAIN_ATTN,    // the same with layer 1's attention in its prologue
  LF_LNCH_PAIR,     // channel rows: gemm_lnch, GEMM + channel LayerNorm per map (two launches)
  LF_LNCH_WHOLE,    // channel rows: gemm_lnch MODE 2, layer 1 whole in one launch
  LF_L1CH,          // channel rows, N = 10, 20: layer1_ch_kernel, layer 1 whole in one launch
};
enum OrbitalMap : int { ORB_NONE = 0, ORB_GEMM = 1, ORB_IN_CHAIN = 2 };  // none: envelope first maps no F
// (C = 1: the value kernel) / the channel determinants straight from F / from PhiC contracted out
// of F into w.o (det_precontract) / from PhiC formed from h without F (env_first)
enum DetStage : int { DET_VALUE = 0, DET_DIRECT = 1, DET_PRECONTRACT = 2, DET_ENV_FIRST = 3 };
struct TrunkRoute {
  int family;        // GemmFamily of every dense GEMM of the pass
  int input_h;       // the input kernel writes h0 = f W0 (else layer 1 forms it: h0_epilogue)
  int input_qkv;     // ... and layer 1's q|k|v = f (W0 Wqkv)
  int input_skip;    // geo is all it writes: skipped when the caller's geometry is in place
  int form0, form1;  // LayerForm of layer 1 and of every later layer
  int attn_feat;     // layer 1's attention forms q|k|v from the features (else reads the input kernel's)
  int h0_epilogue;   // layer 1's residual h0 = f W0 is formed from geo in the first map's epilogue / LayerNorm
  int ofeat;         // layer 1's first map contracts the o~ rows with U at K = ofeat_k (else o with Wol at K = D)
  int qkv_gemm;      // layers >= 2: a q|k|v GEMM precedes attention (a chained layer's last pass wrote it already)
  int orbital;       // OrbitalMap
  int det;           // DetStage
  // Not among the fields dh_debug_route reports (kTrunkRouteFields): the value kernel's work can
  // run as the tail of the last layer's chain launch (gemm_x6.hip chain_x6s_kernel<-1>;
  // value_pass takes it up, every other caller of run_trunk keeps F in HBM and the value kernel)
  int det_in_chain;
};
constexpr int kTrunkRouteFields = 12;
static_assert(sizeof(TrunkRoute) == (kTrunkRouteFields + 1) * sizeof(int) &&
                  offsetof(TrunkRoute, det_in_chain) == kTrunkRouteFields * sizeof(int),
              "dh_debug_route copies the first kTrunkRouteFields fields as ints");
// The family a dense GEMM of this network takes: split-bf16 if wanted and D allows it, else exact f32
int gemm_family(const Dims& d, bool want_x6);
// gemm_mode: DH_GEMM_*; C = 1 or 2N + 5; rows = walkers * N * C
TrunkRoute trunk_route(const Dims& d, int gemm_mode, int C, int rows);
// Process-global switch of TrunkRoute::det_in_chain (1 = on where the route allows it, the
// default; 0 = the separate value kernel everywhere); returns the previous value
int set_det_in_chain(int on);

// The chain kernel's tile (gemm_x6.hip): 96 rows, and the bytes of its three activation planes
// in LDS, which are dead after the last GEMM pass (the determinant tail's F tile and walker
// regions live there)
constexpr int kChainTileRows = 96;
constexpr size_t kChainPlaneBytes = 3 * (size_t)kChainTileRows * 264 * 2;
// det_value_kernel's LDS floats per walker (+1: the epilogue's log psi slot after the f64 unit vectors)
inline int det_value_per(const Dims& d) {
  return (2 * d.N * d.M + 2 * d.N * d.N + 2 * d.N + 2 * d.K + 2 + 4 + 6 * d.N + 2 + 3 + 1) & ~3;
}
// launch_det_value takes the form with two walkers per wave (one per 32-lane half)
inline bool det_value_half_wave(const Dims& d) {
  const int mgv = (d.M + 64 / d.N - 1) / (64 / d.N);  // harmonics per lane
  return mgv <= 2 && d.N * d.N <= 64;
}
// Row stride (floats) of the F tile the chain's determinant tail keeps in LDS.  The contraction
// reads, per 32-lane half, entry (i, j) of the matrix in lane i N + j at float i ld + j K + k
// (+ m N K for harmonic m, the same for every lane), and ds_read_b32 banks are float % 32 per
// half: with ld = orb_cols (192 at N = 6) every row i starts on bank 0 and the read is N-way
// conflicted.  The smallest ld >= orb_cols with ld % 32 == N K % 32 puts lane i N + j on bank
// (i N + j) K + k: conflict-free at K = 1, K-way at K determinants.
inline int det_chain_ldf(const Dims& d) {
  return d.orb_cols + (((d.N * d.K - d.orb_cols) % 32) + 32) % 32;
}

constexpr int kRowPad = 256;
// walker-row buffers (h, qkv, o, t) are padded to 768 = lcm(96, 256) rows, so the log-psi
// LayerNorm GEMM may take 64-, 96- or 128-row tiles without reading past the buffer
constexpr int kWalkerRowPad = 768;
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// Opt a kernel into more than 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU).
template <typename Kern>
inline void ensure_smem(Kern kernel, size_t bytes) {
  if (bytes > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

// ---- kernel launchers (each .hip file) ----------------------------------------
// gemm.hip: Y[r][n] = sum_k X[r][k] W[k][n] + (r % C == 0 ? bias[n] : 0) + (R ? R[r][n] : 0)
void launch_gemm(const float* X, int ldx, const float* W, int ldw, const float* bias, const float* R, int ldr,
                 float* Y, int ldy, int rows, int ncols, int K, int C, hipStream_t s);
// One tile form by its code (0 .. 11 but 3; launch_gemm picks 9, 10); false, nothing launched,
// for any other code.
bool launch_gemm_variant(int v, const float* X, int ldx, const float* W, int ldw, const float* bias, const float* R,
                         int ldr, float* Y, int ldy, int rows, int ncols, int K, int C, hipStream_t s);
// NT form: Y = X Wt^T, Wt[n][k] (row stride ldw), K % 32 == 0, Wt rows padded to 256.
// Codes 0 .. 7, three-stage 10, 11, 14 .. 17, persistent 20 .. 26 (launch_gemm_nt picks 4, 6, 7,
// 20, 25); false, nothing launched, for any other code.
bool launch_gemm_nt_variant(int v, const float* X, int ldx, const float* Wt, int ldw, const float* bias,
                            const float* R, int ldr, float* Y, int ldy, int rows, int ncols, int K, int C,
                            hipStream_t s);
// NT GEMM with the tile shape chosen from (rows, ncols, residual): Wt[n][k], row stride ldw.
void launch_gemm_nt(const float* X, int ldx, const float* Wt, int ldw, const float* bias, const float* R, int ldr,
                    float* Y, int ldy, int rows, int ncols, int K, int C, hipStream_t s);
// Log-psi rows (C = 1), D = 256: GEMM + bias, then (mode 0) + h or (mode 1) h + tanh(.),
// then LayerNorm (ln = gamma|beta), written in place over h [rows][256].
bool gemm_ln_supported(int D, int K);
void launch_gemm_ln(const float* X, int ldx, const float* Wt, int ldw, const float* bias, const float* ln, float* h,
                    int rows, int K, int mode, int bm, hipStream_t s);
// gemm_x6.hip: split-bf16 GEMM (f32-accurate, 6 bf16 MFMAs per product block).
// Wp = three bf16 planes [3][ldp][K] of the transposed weight (launch_split_planes),
// ldp = x6_plane_rows(ncols); K % 32 == 0; X holds round_up(rows, 256) readable rows.
int x6_plane_rows(int ncols);
void launch_split_planes(const float* Wt, int ldw, int ncols, int K, uint16_t* Wp, hipStream_t s);
bool gemm_x6_supported(int K);
// The forms launch_gemm_x6 picks from, named kernel_tile (rows x columns); the values are the
// variant codes of DESIGN.md and profiles/.
enum X6Form : int {
  X6D_128x192 = 44,  // gemm_x6d: two workgroups per CU, short (log-psi) row counts
  X6D_256x128 = 46,
  X6Q_256x128 = 52,  // gemm_x6q: persistent, channel rows
  X6Q_256x256 = 56,
  X6Q_256x192 = 57,
  X6Q_256x160 = 58,
  X6M_256x256 = 76,  // gemm_x6m: persistent 16x16x32 form, the wide channel-row maps
  X6M_256x192 = 77,
};
// The form launch_gemm_x6 takes for a shape (host only: no device call).
int gemm_x6_choose(int rows, int ncols);
// One form by its code: an X6Form, or one of the tiles kept beside them for comparison (gemm_x6.hip
// kX6Forms); false, nothing launched, for any other code.
bool launch_gemm_x6_variant(int v, const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias,
                            const float* R, int ldr, float* Y, int ldy, int rows, int ncols, int K, int C,
                            hipStream_t s);
void launch_gemm_x6(const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias, const float* R, int ldr,
                    float* Y, int ldy, int rows, int ncols, int K, int C, hipStream_t s);
// h = LN(h + X W + b) (mode 0) or LN(h + tanh(X W + b)) (mode 1), in place, split-bf16
// arithmetic; h [rows][256], ln = [gamma(256), beta(256)]; nw = tile form (0: pick, or 1, 2, 3, 4, 8;
// gemm_x6.hip); false, nothing launched, for any other nw.
// feat (layer 1 of log psi, mode 0): the residual h = features W0 is formed in the epilogue
// from geo [rows][4] = (sin th, cos th, sin ph, cos ph) and W0 [4][256] instead of read.
struct X6Feat {
  const float* W0 = nullptr;
  const float* geo = nullptr;
  int N = 1, n_up = 0;
  // launch_chain_x6 only: layer 1's attention formed in the chain prologue from the features
  // (folded W0 Wqkv [4][3D], bqkv [3D]) instead of read from X1 (chain_attn_supported)
  const float* W0qkv = nullptr;
  const float* bqkv = nullptr;
  const float* Mqk = nullptr;  // [H][kMqkStride] (attn_val.h attn_feat_core)
  // with W0qkv: layer 1's coefficient-space maps (planes of V^T, B^T; launch_l1_basis)
  const uint16_t* L1V = nullptr;
  const uint16_t* L1B = nullptr;
};
bool launch_gemm_x6_ln(const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias, const float* ln,
                       float* h, int rows, int K, int mode, int nw, hipStream_t s, X6Feat feat = X6Feat{});
// gemm_lnch.hip: channel rows (C = 2N + 5 per electron, ne electrons), D = K = 256, N <= 8:
// h = LN_ch(h + X W + b) (mode 0) or LN_ch(h + tanh_ch(h W + b)) (mode 1) in ONE launch,
// in place over h [ne * C][256]; X [ne * C][256] (mode 1: X = h); split-bf16 arithmetic.
// DH_LNCH=0 selects the GEMM + layernorm_ch pair instead.
bool gemm_lnch_supported(int N, int D);
int set_lnch_form(int f);  // 0 off, 1 gemm_lnch_kernel; returns the previous form
// K: X's row length and the contraction (mode 0 / 2; 256, or layer 1's ofeat_k o~ rows with
// Wp = the planes of U^T); mode 1 contracts over h's 256 features.  Mode 2 (layer 1 whole, H = 4:
// LN1, Wm, tanh_ch, LN2 from the o~ rows; ln = LN2's scale | shift, bias = bol, W0f = W0): Wv /
// Wb = the planes of layer 1's coefficient-space maps V^T / B^T (launch_l1_basis, K = 32).
void launch_gemm_lnch(int N, const float* X, const uint16_t* Wp, int ldp, const float* bias, const float* ln,
                      const float* geo, float* h, int ne, int mode, hipStream_t s,
                      const float* W0f = nullptr, int n_up = 0, int K = 256, const uint16_t* Wv = nullptr,
                      const uint16_t* Wb = nullptr);
// Layer 1 in coefficient space (gemm_lnch.hip MODE 2): with E = [W0 (4); U's 5 H nonzero rows;
// bol; ones] and row 26 = beta, BT[n][j] = gamma_n E[j][n] (j < 26), beta_n (j = 26), and
// VT[n][j] = sum_k B[j][k] Wm[k][n] (+ bm_n for j = 26); 32 columns, f64 sums; H = 4.
void launch_l1_basis(const Dims& d, const float* W0, const float* UT, const float* bol, const float* ln1,
                     const float* Wm, const float* bm, float* BT, float* VT, hipStream_t s);
bool chain_attn_supported(int N, int H, int dh);
struct ChainDet;
// Log-psi layer tail in one launch (D = K = 256): h1 = LN1(h + X1 Wol + b1) (feature
// residual when feat.W0), h = LN2(h1 + tanh(h1 Wm + b2)), then Y3 = h W3 + b3 if Wp3.
// det (TrunkRoute::det_in_chain, Y3 = the orbitals F): the value kernel's work runs as the
// launch's tail on the tile's F rows in LDS; store_F then says whether F is written to Y3 too.
void launch_chain_x6(const float* X1, const uint16_t* Wp1, int ldp1, const float* b1, const float* ln1,
                     const uint16_t* Wp2, int ldp2, const float* b2, const float* ln2, const uint16_t* Wp3, int ldp3,
                     const float* b3, int n3, float* Y3, int ldy3, float* h, int rows, X6Feat feat, hipStream_t s,
                     bool store_h = true, const ChainDet* det = nullptr, bool store_F = true);
// dst[c][r] = src[r][c] for r < rows, c < cols (row strides ld_src / ld_dst).
void launch_transpose(const float* src, int ld_src, int rows, int cols, float* dst, int ld_dst, hipStream_t s);

// input.hip
// Features (psiformer.py:51-60) of every channel times W0 -> h [rows][D]; also
// writes geo[nw][N][4] = (sin th, cos th, sin ph, cos ph).
// With W0qkv != nullptr it also writes layer 1's q|k|v = f (W0 Wqkv) (+ bqkv on value
// rows): the first attention projection is folded into the K=4 input map.
void launch_input(const Dims& d, const float* x, const float* W0, const float* W0qkv, const float* bqkv, float* h,
                  float* qkv, float* geo, int nw, int C, hipStream_t s);
// Proposal (mcmc.py:67-102): x2 = sph_sampling(x, noise).
// geo (optional): the proposal's geometry (sin/cos of the f32 angles, as input_kernel).
void launch_propose(const Dims& d, const float* x, float* x2, int nw, float width, uint64_t seed, uint64_t step,
                    int64_t walker_offset, const float* noise, int noise_stride, hipStream_t s, float* geo = nullptr);
// accept of `step` + proposal of `step + 1` (and its geometry) in one launch.
void launch_accept_propose(const Dims& d, float* x, float* x2, float* geo, float* lp, const float* logpsi2,
                           int32_t* n_acc, int nw, float width, uint64_t seed, uint64_t step, int64_t walker_offset,
                           const float* noise, const float* noise2, hipStream_t s);
void launch_init_walkers(const Dims& d, float* x, int nw, uint64_t seed, int64_t walker_offset, hipStream_t s);

// attention.hip: channel self-attention for all heads.
// W0qkv/bqkv non-null: layer-1 q|k|v formed in-kernel from the input features (only when
// attention_takes_features(d)); otherwise read from qkv [rows][3D].
bool attention_takes_features(const Dims& d, int C);
// channel attention on the matrix cores (attention_mfma.hip): C > 1, dh = 64, N = 10, 20
bool attention_mfma_supported(const Dims& d);
void launch_attention_mfma(const Dims& d, const float* qkv, const float* geo, float* o, int nw, hipStream_t s,
                           const float* W0qkv, const float* bqkv);
void launch_attention(const Dims& d, const float* qkv, const float* geo, float* o, int nw, int C, hipStream_t s,
                      const float* W0qkv = nullptr, const float* bqkv = nullptr, const float* Mqk = nullptr);
// layer 1's 5 x 5 score forms per head, Mqk[h][a][b] = sum_d Wq~[a][h dh + d] Wk~[b][h dh + d] / 8
// (Wq~ / Wk~ = the folded W0 Wqkv rows with the bias as row 4; dh = 64; f64 sums)
void launch_lowrank_qk(const Dims& d, const float* W0qkv, const float* bqkv, float* Mqk, hipStream_t s);
// U^T [n][ofeat_k] (row stride ofeat_k, rows n < D; f64 sums) from the folded W0 Wqkv, bqkv and Wol
void launch_ofeat_weight(const Dims& d, const float* W0qkv, const float* bqkv, const float* Wol, float* UT,
                         hipStream_t s);

// layernorm.hip
//   mode 0: h = LN_ch(X)           (X may alias h)
//   mode 1: h = LN_ch(h + tanh_ch(Z))
void launch_layernorm(const Dims& d, const float* X, const float* Z, const float* ln, const float* geo, float* h,
                      int nw, int C, int mode, hipStream_t s,
                      const float* W0f = nullptr);
// layer 1 of the local energy at N = 10, 20 in one launch from the o~ rows O [ne C][KO]
// (layernorm.hip layer1_ch_kernel): UT = U^T [256][KO], VT = V^T [256][32] (launch_l1_basis)
bool layer1_ch_supported(const Dims& d);
void launch_layer1_ch(const Dims& d, const float* O, const float* UT, const float* VT, const float* W0f,
                      const float* bol, const float* ln1, const float* ln2, const float* geo, float* h, int nw,
                      hipStream_t s);

// det.hip
//   value mode (C == 1): logpsi[nw][2]
//   energy mode (C == 2N+5): e_l[nw][2], obs[nw][8]
// MCMC epilogue of the value kernel (round 5): after log psi of the proposal x2 (= the x the
// kernel evaluates), the accept of `step` (mcmc.py:55-62: x, lp, nacc updated) and, when
// `propose`, the next proposal of step + 1 into x2 / geo (mcmc.py:67-102) — what
// launch_accept_propose / launch_accept do, per walker, bit for bit, without their launch.
struct McmcEpi {
  int on = 0, propose = 0;
  float* x = nullptr;
  float* x2 = nullptr;
  float* geo = nullptr;
  float* lp = nullptr;
  int32_t* nacc = nullptr;
  float width = 0.f;
  uint64_t seed = 0, step = 0;
  int64_t woff = 0;
  const float* noise = nullptr;   // this step's injected noise (accept uniform)
  const float* noise2 = nullptr;  // the next step's (its proposal)
};
void launch_det_value(const Dims& d, const float* F, const float* x, const float* jastrow, const float* norm,
                      float* logpsi, int nw, hipStream_t s, const McmcEpi& epi = McmcEpi{});
// launch_det_value's arguments for the chain launch that runs the value kernel's body as its
// tail (launch_chain_x6's det; det_value_half_wave(d) and the route's conditions hold)
struct ChainDet {
  const float* x = nullptr;
  const float* jastrow = nullptr;
  const float* norm = nullptr;
  float* logpsi = nullptr;
  int N = 0, n_up = 0, M = 0, K = 0, nw = 0;
  int per = 0;  // det_value_per
  int ldf = 0;  // det_chain_ldf
  McmcEpi epi;
};
// phic != nullptr (det_precontract(d)): the channel matrices are first contracted from F by
// env_contract_kernel into phic [nw][K][C][N][N] complex, then assembled from there
// NetObs estimators (netobs.hip): theta / pair-angle histograms, LLL monopole harmonics
void launch_histograms(const float* x, int B, int N, int db, int pb, float* dens, float* pair, hipStream_t s);
void launch_monopole_orbitals(const float* pts, int n, int flux, float* out, hipStream_t s);
// Renyi-2 swap estimator (swap.hip): classify pairs by their counts in the caps theta < t[a],
// compact the matched ones (scan + gather of the swapped rows), reduce the swap values by angle
// and sector.  The cap angles travel as a kernel argument.  B >= 2, 1 <= A <= kSwapMaxAngles and
// 2 A (B / 2) < 2^31 are the callers' to check: then no grid is empty.
constexpr int kSwapMaxAngles = 64;
struct SwapThetas {
  float t[kSwapMaxAngles];
};
void launch_swap_classify(const float* x, int B, int N, int n_up, const SwapThetas& th, int A, int32_t* sector,
                          int32_t* counts, hipStream_t s);
// row [A (B / 2)]: workspace (each pair's output row, -1 when unmatched)
void launch_swap_compact(const float* x, int B, int N, int n_up, const SwapThetas& th, int A, const int32_t* sector,
                         int32_t* row, int32_t* start, int32_t* pair, float* xs, hipStream_t s);
void launch_swap_reduce(const float* logpsi, const float* logpsi_s, int B, int K, int A, int M, const int32_t* pair,
                        const int32_t* sector, const int32_t* start, double* sums, hipStream_t s);
// Landau-level-resolved one-body density matrix (rdm.hip): the harmonics Y_{Q,Q+n,m} of the levels
// n < levels, the displaced configurations, and rho = 4 pi sum over samples of u conj(v) reduced on
// the device in double.  The limits (levels <= kRdmMaxLevels, flux <= 126, nelec <= 32, P B <= 2^30,
// P B nelec^2 < 2^31) are the callers' to check.  table: rdm_table's device coefficients.
constexpr int kRdmMaxLevels = 4;
int rdm_norb(int flux, int levels);
int rdm_nsplit(int64_t samples, int flux, int levels);
size_t rdm_workspace_bytes(int64_t samples, int flux, int levels);
hipError_t rdm_table(int flux, int levels, const double** table);
void launch_monopole_harmonics(const float* pts, int n, int flux, int levels, const double* table, float* out,
                               hipStream_t s);
void launch_rdm_displace(const float* x, const float* r_prime, int B, int N, int P, float* xp, hipStream_t s);
hipError_t launch_rdm_accumulate(const float* x, const float* r_prime, const float* logpsi, const float* logpsi_p,
                                 int B, int N, int n_up, int flux, int levels, int P, int by_spin,
                                 const double* table, double* rho, int32_t* nvalid, void* workspace, hipStream_t s);
// Total-spin estimator (spin.hip): the exchanged rows of the pairs [pair0, pair1) (pair
// p = i n_dn + (j - n_up) of an up slot i and a down slot j), their ratios psi(R_p) / psi(R) into
// the workspace, and, once every pair is there, S^2_loc per walker with the sums over the valid
// walkers.  The limits (nelec <= 32, B n_up n_dn < 2^31, 0 <= pair0 < pair1 <= n_up n_dn for the
// first two) are the callers' to check: then no grid is empty.
size_t spin_workspace_bytes(int B, int P);
void launch_spin_exchange(const float* x, int B, int N, int n_up, int n_dn, int pair0, int pair1, float* xs,
                          hipStream_t s);
void launch_spin_ratios(const float* logpsi, const float* logpsi_s, int B, int pair0, int pair1, void* workspace,
                        hipStream_t s);
void launch_spin_reduce(const float* logpsi, int B, int n_up, int n_dn, void* workspace, double* s2, double* pairs,
                        double* total, int32_t* nvalid, hipStream_t s);
// Pair amplitudes (pairamp.hip): the rows with the electrons of pair q = (i < j), lexicographic,
// at r1[p][b] and r2[p][b]; (4 pi)^2 K_L of n quadruples; and A[3][flux + 1] complex, the sums over
// the kept samples of the ratio times K_L by class (up-up, up-down, down-down).  The limits
// (1 <= N <= 32, 0 <= flux <= kPairMaxFlux, P B <= 2^30, rows < 2^31, the pair window) are the callers' to check.
constexpr int kPairMaxFlux = 126;
constexpr int kPairMaxPairs = 32 * 31 / 2;
struct PairSlots {
  unsigned char i[kPairMaxPairs], j[kPairMaxPairs];
};
PairSlots pair_slots(int N);
size_t pair_workspace_bytes(int64_t samples, int N, int flux);
void launch_pair_displace(const float* x, const float* r1, const float* r2, int B, int N, int P, int pair0, int pair1,
                          float* xp, hipStream_t s);
void launch_pair_kernel(const float* points, int n, int flux, double* out, hipStream_t s);
hipError_t launch_pair_accumulate(const float* x, const float* r1, const float* r2, const float* logpsi,
                                  const float* logpsi_p, int B, int N, int n_up, int flux, int P, double* A,
                                  int32_t* nvalid, void* workspace, hipStream_t s);
// Static structure factor (sfactor.hip): per-walker pair sums T[B][3][lmax+1] (uu, ud, dd) of
// P_L(cos gamma_ij) and multipoles rho[B][2][nlm] complex of Y_LM, and their sums over the valid
// walkers reduced on the device in double.  The limits (nelec <= 32, 0 <= n_up <= nelec,
// 0 <= lmax <= kSfMaxL, B >= 1, B nelec < 2^31) are the callers' to check: then no grid is empty.
constexpr int kSfMaxL = 64;
int sf_nlm(int lmax);
size_t sf_workspace_bytes(int B, int lmax);
void launch_sf_pairs(const float* x, int B, int N, int n_up, int lmax, double* T, hipStream_t s);
void launch_sf_multipoles(const float* x, int B, int N, int n_up, int lmax, double* rho, hipStream_t s);
void launch_sf_accumulate(const float* x, int B, int N, int n_up, int lmax, bool want, double* pair_sums,
                          double* rho_sums, int32_t* nvalid, void* workspace, hipStream_t s);
bool det_precontract(const Dims& d);
void launch_det_energy(const Dims& d, const float* F, const float* x, const float* geo, const float* jastrow,
                       const float* norm, float* e_l, float* obs, int nw, hipStream_t s, float* phic);
size_t det_energy_smem_bytes(const Dims& d);
// envelope first (round 6, C4 / C5: one spin block, one determinant, N > 8; det.hip): the
// channel matrices PhiC from h directly — Weff = E2 W2 per electron, F of six special rows per
// electron, env_phi_kernel — instead of the full orbital map F and env_stream / env_contract
bool env_first(const Dims& d);
int env_first_k(const Dims& d);  // KE: the envelope-coefficient row length (2 M padded to 32)
// W2T [256 * 2N][KE] from the packed Worb (launch_split_planes makes its planes)
void launch_env_w2(const Dims& d, const float* Worb, float* W2T, hipStream_t s);
// S [round_up(6 ne, 256)][256], FS [round_up(6 ne, 256)][ld_orb], E2 [round_up(ne, 256)][KE],
// Weff [round_up(ne, 256)][256 * 2N] (ne = nw N): workspace; phic [nw][C][N][N] complex
void launch_env_first(const Dims& d, const float* h, const float* geo, const float* x, const float* norm,
                      const float* WorbT, const float* borb, const uint16_t* WorbP, const float* W2T,
                      const uint16_t* W2P, bool x6, int nw, float* S, float* FS, float* E2, float* Weff, float* phic,
                      hipStream_t s);
// det_energy_kernel<0, true> alone on precontracted channel matrices
void launch_det_energy_pc(const Dims& d, const float* x, const float* geo, const float* jastrow, const float* norm,
                          float* e_l, float* obs, int nw, hipStream_t s, const float* phic);
// test hook: env_leaf (e0, dth, dph, lb, d2th as re / im pairs: 10 floats) of n (theta, phi)
// pairs for every harmonic p < M, norm 1, the production gauge; sq: powers by squaring
void launch_env_leaf_probe(const float* thph, int n, int M, int sq, float* out, hipStream_t s);
void launch_potential(const Dims& d, const float* x, float* pe, int nw, hipStream_t s);
// mcmc.hip: accept/reject (mcmc.py:55-62).
void launch_accept(const Dims& d, float* x, const float* x2, float* lp, const float* logpsi2, int32_t* n_acc,
                   int nw, uint64_t seed, uint64_t step, int64_t walker_offset, const float* noise,
                   int noise_stride, hipStream_t s);
void launch_lp_from_logpsi(const float* logpsi, float* lp, int32_t* n_acc, int nw, hipStream_t s);

// kinetic.hip: KE / Lz / Lz^2 / L^2 of an arbitrary log psi from its derivatives
size_t kinetic_assembly_lds_bytes(int N);
void launch_kinetic_assembly(const double* x, const double* g, const double* H, int nw, int N, double Q, double r,
                             float* ke, float* mom, hipStream_t s);

// stats.hip
void launch_stats(const float* e_l, const float* obs, const int32_t* n_acc, int B, int steps, int penalties,
                  float* out, hipStream_t s);
// g: device pointer to the reduced stats; diff [B][2]; nvalid [1]
void launch_loss_diff(const float* e_l, const float* obs, int B, const float* g, float lz_penalty, float lz_center,
                      float l2_penalty, float* diff, float* nvalid, hipStream_t s);

// grad.hip: reverse mode of log psi w.r.t. the parameters (see the file header)
constexpr int kGradChunk = 512;       // rows per weight-gradient partial
constexpr int kLnRowsPerBlock = 64;   // rows per LayerNorm-backward block (one partial each)
int grad_chunks(int rows);
int ln_bwd_blocks(int rows);
void launch_ln_fwd(const float* a, const float* z, const float* ln, float* out, int rows, int D, hipStream_t s);
void launch_ln_bwd(const float* a, const float* z, const float* ln, const float* dy, const float* dres, float* da,
                   float* dz, float* pg, int rows, int D, hipStream_t s);
// rpb rows per block, one partial pair per block (rpb = N: per-walker partials, dh_ntk)
void launch_ln_bwd_rows(const float* a, const float* z, const float* ln, const float* dy, const float* dres,
                        float* da, float* dz, float* pg, int rows, int D, int rpb, hipStream_t s);
void launch_attn_bwd(const Dims& d, const float* qkv, const float* dO, float* dqkv, int nw, hipStream_t s);
void launch_tn_partial(const float* X, int ldx, const float* Y, int ldy, int rows, int M, int Nc, float* P,
                       hipStream_t s);
void launch_colsum_partial(const float* Y, int ldy, int rows, int Nc, float* P, hipStream_t s);
void launch_w0_partial(const Dims& d, const float* geo, const float* Y, int ldy, int rows, float* P, hipStream_t s);
// out[r * ldo + c] = scale * sum_ch P[ch * stride + r * ldp + c] (+ out if acc), r < nr, c < nc
void launch_reduce2d(const float* P, int nchunk, size_t stride, int ldp, int nr, int nc, float* out, int ldo,
                     float scale, int acc, hipStream_t s);
void launch_small_gemm(int M, int N, int K, const float* A, int lda, int ta, const float* B, int ldb, int tb, float* C,
                       int ldc, int acc, hipStream_t s);
void launch_copy2d(const float* src, int lds, float* dst, int ldd, int nr, int nc, hipStream_t s);
void launch_cotangent(const float* diff, const float* nvalid, int B, int part, float* ct, hipStream_t s);
void launch_adam(float* p, const float* g, float* mu, float* nu, size_t n, float lr, float b1, float b2, float eps,
                 int step, hipStream_t s);
// "sparse" orbitals (blocks.py:52-62): featured orbitals with 8 features per (j, k),
// mixed into the M harmonics by lll_weight (DenseGeneral over axis 1, real kernel, bias on
// the real part), folded into the full layout:
//   Wfull[d][m NK + jk] = sum_a W8[d][a NK + jk] Wl[a][m]  (rows d < D; row D = the bias,
//   with + bl[m] when `real_part`)
void launch_sparse_fold(const float* W8, const float* b8, const float* Wl, const float* bl, int real_part, int D,
                        int NK, int M, float* Wfull, int ldw, float* bfull, hipStream_t s);
// gradient: dW8[d][a NK + jk] (+)= sum_m dWfull[d][m NK + jk] Wl[a][m] (rows d < D, row D bias)
void launch_sparse_unfold(const float* dWfull, int ldw, const float* dbfull, const float* Wl, int D, int NK, int M,
                          float* dW8, float* db8, int acc, hipStream_t s);
// dWl[a][m] (+)= sum_{blocks i} [sum_d W8_i[d][a NK + jk] dWfull_i[d][m NK + jk] + b8_i . dbfull_i];
// dbl[m] (+)= sum_{real blocks} sum_jk dbfull_i[m NK + jk].  W8s/b8s: per-block pointers.
struct SparseBlocks {
  const float* W8[4];
  const float* b8[4];
  int n;
};
void launch_sparse_lll_grad(SparseBlocks blk, const float* dWfull, int ldw, const float* dbfull, int D, int NK, int M,
                            float* dWl, float* dbl, int acc, hipStream_t s);

// The parameter-free trial states (their common device code: trial_common.h; api_trial.cpp
// picks the launcher in launch_trial).
// laughlin.hip: log psi (e_l == nullptr) or the local energy (e_l [nw][2], obs [nw][8])
// of the Laughlin wavefunction; expo [2][N] = (Q1 + m_j, Q1 - m_j)
size_t laughlin_smem_bytes(int N);
void launch_laughlin(const Dims& d, const float* x, const int* expo, float* logpsi, float* e_l, float* obs, int nw,
                     hipStream_t s);

// cf.hip: the same two launches for a Jain state with two Lambda levels.  tab: per column
// (level, A = Q1 + m, B = Q1 - m), then the number of level-1 columns n_dense, p, and the
// column of each of them.  LDS per walker by instantiation.
size_t cf_smem_bytes(int N, int n_dense, bool energy);
void launch_cf(const Dims& d, const float* x, const int* tab, int n_dense, float* logpsi, float* e_l, float* obs,
               int nw, hipStream_t s);

// pfaffian.hip: the same two launches for the Moore-Read Pfaffian state with 2 p vortices per
// electron (N even, flux 2 p (N - 1) - 1; no table).  LDS per walker by instantiation.
size_t pfaffian_smem_bytes(int N, bool energy);
void launch_pfaffian(const Dims& d, const float* x, int p, float* logpsi, float* e_l, float* obs, int nw,
                     hipStream_t s);

// halperin.hip: the same two launches for a Halperin (m_up, m_dn, n) state: the slots below
// d.n_up up, the rest down, no table.  The value launch packs 256 / halperin_group(N) walkers into
// a workgroup; LDS per workgroup by instantiation.
int halperin_group(int N);
size_t halperin_smem_bytes(int N, bool energy);
void launch_halperin(const Dims& d, const float* x, int m_up, int m_dn, int n_int, float* logpsi, float* e_l,
                     float* obs, int nw, hipStream_t s);

// quasihole.hip: the same two launches for pinned quasiholes on a Halperin or a Moore-Read base.
// The state goes to the kernel by value: the pair weights (Pfaffian base: all three 2 p), the
// holes' kinds (DH_HOLE_*) and spinors (Re U, Im U, Re V, Im V).  LDS per walker by instantiation.
struct QuasiholeState {
  int pfaffian;  // 0: Halperin base, 1: Pfaffian base
  int m_up, m_dn, n_int;
  int n_holes;
  int kind[DH_QUASIHOLE_MAX_HOLES];
  double uv[DH_QUASIHOLE_MAX_HOLES][4];
};
size_t quasihole_smem_bytes(int N, bool pfaffian, bool energy);
void launch_quasihole(const Dims& d, const float* x, const QuasiholeState& q, float* logpsi, float* e_l, float* obs,
                      int nw, hipStream_t s);
// out[B][K][2] (double) = log psi_c of each walker for the K configurations of a device table
// (dh_hole_table's layout: uv [DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES][4] double, then kind
// [DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES] int); base: the weights, the base and n_holes.
void launch_hole_logs(const float* x, int B, int N, int n_up, const QuasiholeState& base, int K, const void* table,
                      double* out, hipStream_t s);

// holes.hip: the Gram matrix of the amplitude ratios over the walkers (dh_hole_gram)
size_t hole_workspace_bytes(int B, int K);
void launch_hole_gram(const double* L, int B, int K, const double* shift, double* S, int32_t* nvalid, void* workspace,
                      hipStream_t s);

// subspace.hip: the overlap, Hamiltonian and kinetic matrices of K states over the walkers
// (dh_subspace_accumulate); logs, e_l, ke [K][B][2] float32, out [3][K][K][2] double
constexpr int kSubspaceMaxStates = 32;  // = DH_SUBSPACE_MAX_STATES
size_t subspace_workspace_bytes(int B, int K);
void launch_subspace_accumulate(const float* logs, const float* e_l, const float* ke, int B, int K, const double* shift,
                                double* out, int32_t* nvalid, void* workspace, hipStream_t s);

// impurity.hip: the one-body impurity term of the local energy (dh_external_potential) and the
// histogram of the angle from an axis (dh_axis_histogram).  The table is a kernel argument: unit
// vectors and coefficients from the host, in double.  p, q: R^2 / w^2 and 0 (gaussian), 2 R^2 and
// h^2 (charge).  The limits (1 <= N <= 32, B >= 1, B N < 2^31, n <= kMaxImpurities, 1 <= bins <=
// 4096) are the callers' to check.
constexpr int kMaxImpurities = 8;
enum { kImpurityGaussian = 0, kImpurityCharge = 1 };
enum { kImpurityBoth = 0, kImpurityUp = 1, kImpurityDown = 2 };  // = DH_HOLE_BOTH, DH_HOLE_UP, DH_HOLE_DOWN
struct ImpurityTable {
  double ax[kMaxImpurities], ay[kMaxImpurities], az[kMaxImpurities];
  double strength[kMaxImpurities], p[kMaxImpurities], q[kMaxImpurities];
  int kind[kMaxImpurities], species[kMaxImpurities];
  int n;
};
void impurity_vector(double theta, double phi, double* v);  // (sin th cos ph, sin th sin ph, cos th)
void launch_external_potential(const float* x, int B, int N, int n_up, const ImpurityTable& tab, float* e_l,
                               float* ext, hipStream_t s);
void launch_axis_histogram(const float* x, int B, int N, int n_up, double axis_theta, double axis_phi, int bins,
                           unsigned* counts, hipStream_t s);

// det.hip: backward of log psi = J + log sum_k det Phi_k for per-walker cotangents ct[nw][2]:
// dF [nw*N][ld_orb] (all columns written) and jg[nw][2] = ct.re * dJ / d(ee_par, ee_anti)
void launch_det_bwd(const Dims& d, const float* F, const float* x, const float* jastrow, const float* norm,
                    const float* ct, float* dF, float* jg, int nw, hipStream_t s);

// kfac.hip: KFAC curvature statistics, damped inverses and update (api_grad.cpp dh_kfac_*)
struct KfacSlot {  // one factor matrix n x n (f32) at float offset `off` of the statistics buffer
  int n;
  size_t off;
};
struct KfacInvJob {  // one damped inverse: slot, the paired factor's slot (for pi), A or G side
  int slot, partner, is_a, n;
  float sqrt_scale;  // sqrt(fixed_scale) of the block
  size_t gj_off;     // f64 offset of the n x n matrix in the inverse buffer
};
struct KfacBlockJob {  // one dense block: gradient segments (ref layout) and f64 work offsets
  size_t kernel_off;
  long long bias_off;  // -1: no bias
  int din, dout;
  size_t v_off, t_off, pv_off;
};
struct KfacGemmJob {  // C[M][N] = A[M][K] B[K][N], f64 offsets into one buffer
  size_t a_off, b_off, c_off;
  int M, N, K;
};
constexpr int kKfacMaxGen = 80;
struct KfacGenTable {  // generic (diagonal) parameter segments: ref offset, compact offset
  int n, total;
  size_t ref[kKfacMaxGen];
  int cmp[kKfacMaxGen];
};
struct KfacDevPlan {  // device copies of the job tables (owned by the handle)
  KfacSlot* slots;
  KfacInvJob* inv_jobs;
  KfacBlockJob* block_jobs;
  KfacGemmJob *gemm1, *gemm2;
  int nslots, njobs, nblocks, nmax, max_v, max_m, max_n;
  KfacGenTable gen;
};
void launch_kfac_aug(const float* P, int nch, int n, float* out, int ld, float scale, float corner, int acc,
                     hipStream_t s);
void launch_kfac_feat_gram(const Dims& d, const float* geo, int rows, float* P, hipStream_t s);
// "sparse" orbitals: the featured-orbital tangent lll dF and the lll output tangent as rows of M
void launch_kfac_sparse_dphi(const float* dF, int ld, const float* lll, int M, int NK, int seg, int nr, int na, int N,
                             int lo, float* out, hipStream_t s);
void launch_kfac_sparse_regroup(const float* dF, int ld, int M, int NK, int seg, int nr, int na, int N, int lo,
                                float* out, hipStream_t s);
void launch_kfac_fisher_ct(const float* logpsi, int nw, float* ct, hipStream_t s);
void launch_kfac_generic(const float* fgrad, const KfacGenTable& tab, float* diag, float scale, hipStream_t s);
void launch_kfac_ema(float* raw, const float* st, size_t n, float ema, hipStream_t s);
size_t kfac_gj_tmp_doubles(int njobs, int nmax);
void launch_kfac_invert(const KfacDevPlan& p, const float* raw, double inv_weight, double sqrt_lambda, double* tr,
                        double* gj, double* tmp, hipStream_t s);
void launch_kfac_precondition(const KfacDevPlan& p, const float* grad, const float* raw_diag, double inv_weight,
                              double lambda, double* buf, float* pg, size_t nref, double* info, hipStream_t s);
void launch_kfac_update(float* params, const float* pg, size_t n, double* info, double lr, double norm_constraint,
                        hipStream_t s);

// ntk.hip: the per-walker gradient Gram matrix (api_grad.cpp dh_ntk)
constexpr int kNtkTileRows = 128;  // rows (walkers x n) of one Gram tile
int ntk_tile_walkers(int n);       // whole walkers of n rows per tile
// T[b][b'] (nwalk x nwalk) += sum_{t in b, t' in b'} (X_t . X_t' + a_t + a_t') (Y_t . Y_t'), rows t
// of walker b = b n .. b n + n - 1; a [rows] or null (0); Y == null: the second factor is 1.
// Upper-triangle tile pairs only (launch_ntk_mirror completes T); n <= kNtkTileRows.
// Only rows wi of T with (wi / tw_own) % nparts == part are added to (dh_ntk_part's ownership
// rule; tw_own = the dense maps' tile walkers; 0 of 1: every row).
void launch_ntk_gram(const float* X, int ldx, int Kx, const float* Y, int ldy, int Ky, const float* arow, int n,
                     int nwalk, int tw_own, int part, int nparts, float* T, hipStream_t s);
// U [rows][K] = X - mean (row stride K), a[r] = mean . U[r] + (mean . mean + bias) / 2, so that
// X_t . X_t' + bias = U_t . U_t' + a_t + a_t'
void launch_ntk_centre(const float* X, int ldx, int K, const float* mean, bool bias, int rows, float* U, float* a,
                       hipStream_t s);
// jv[w] += sum_{t in w, c < Ky} ((X V)[t][c] + cvec[c]) dY[t][c]: X [nwalk n][K], V [K][Ky] (row
// stride ldv), cvec [Ky] or null, dY [nwalk n][Ky]; one workgroup per tile of ntk_tile_walkers(n)
// walkers and block of 128 columns, its sums into part [ntk_jvp_col_blocks(Ky)][nwalk] (scratch),
// then the blocks summed in order into jv
int ntk_jvp_col_blocks(int Ky);
void launch_ntk_jvp(const float* X, int ldx, int K, const float* V, int ldv, const float* cvec, const float* dY,
                    int ldy, int Ky, int n, int nwalk, float* part, float* jv, hipStream_t s);
// cvec[c] = bias[c] + sum_k mean[k] V[k][c]; bias, mean: null = 0
void launch_ntk_jvp_cvec(const float* mean, int K, const float* V, int ldv, const float* bias, int Ky, float* cvec,
                         hipStream_t s);
// jv[w] += J[w][0 : ka] . va + J[w][ka : ka + kb] . vb
void launch_ntk_rowdot(const float* J, int ldj, const float* va, int ka, const float* vb, int kb, int nwalk, float* jv,
                       hipStream_t s);
void launch_ntk_mirror(float* T, int B, hipStream_t s);
void launch_ntk_mask_ct(const float* logpsi, const float* ct, float* out, int B, hipStream_t s);
void launch_ntk_features(const Dims& d, const float* geo, int rows, float* out, hipStream_t s);
// dh_minsr_matrix: A [2 Bg][2 Bg] float64 = C T C / n + damping I from the symmetric float32 T
// and the walkers' valid flags; ws: minsr_matrix_ws_doubles(Bg) doubles
size_t minsr_matrix_ws_doubles(int Bg);
void launch_minsr_matrix(const float* T, const unsigned char* valid, int Bg, double damping, double* A, double* ws,
                         hipStream_t s);
// fidelity.hip: dh_fidelity_partial (part [DH_NFID] doubles) and dh_fidelity_residual
void launch_fidelity_partial(const float* logpsi, const float* logphi, int B, double* part, hipStream_t s);
void launch_fidelity_residual(const float* logpsi, const float* logphi, int B, const double* total, float* resid,
                              hipStream_t s);
// orthogonal.hip: dh_ortho_partial (part [K][DH_NFID] doubles, workgroup k = state k) and
// dh_ortho_residual (e_l may be NULL)
void launch_ortho_partial(const float* logpsi, const float* logphi, int B, int K, double* part, hipStream_t s);
void launch_ortho_residual(const float* logpsi, const float* logphi, int B, int K, const double* total,
                           const double* weight, const float* e_l, float* out, hipStream_t s);

}  // namespace dh

