// Which launches make up one Psiformer pass: the one place that decides (dh_internal.h TrunkRoute;
// DESIGN.md §1 "Routes" tabulates what comes out, tests/test_abi_host.py pins it).  Host only.
#include <atomic>

#include "dh_internal.h"

namespace dh {

namespace {
std::atomic<int> g_det_in_chain{1};
}
int set_det_in_chain(int on) { return g_det_in_chain.exchange(on ? 1 : 0); }

int gemm_family(const Dims& d, bool want_x6) {
  const bool nt = d.D % 32 == 0;  // derive_weights keeps the transposed weights and their planes
  return nt && want_x6 && gemm_x6_supported(d.D) ? GEMM_X6 : nt ? GEMM_F32_NT : GEMM_F32_NN;
}

TrunkRoute trunk_route(const Dims& d, int gemm_mode, int C, int rows) {
  const int D = d.D;
  const bool channels = C > 1;  // the local energy's 2N + 5 channel rows; else log psi
  const bool unfused = gemm_mode == DH_GEMM_X6_ALL_UNFUSED;
  TrunkRoute r{};
  // channel rows (local energy) take the split-bf16 GEMM unless exact-f32 is requested;
  // the log-psi rows only in DH_GEMM_X6_ALL (and its unfused twin)
  r.family = gemm_family(d, channels ? gemm_mode != DH_GEMM_F32 : (gemm_mode == DH_GEMM_X6_ALL || unfused));
  const bool x6 = r.family == GEMM_X6, nt = r.family != GEMM_F32_NN;
  // Layer-1 q|k|v come straight from the K=4 features through the folded W0 Wqkv: inside
  // the attention kernel when it supports that, else written by the input kernel.
  const bool fused = d.L > 0 && attention_takes_features(d, C);
  r.attn_feat = fused;
  r.input_qkv = d.L > 0 && !fused;
  r.qkv_gemm = 1;
  r.form0 = r.form1 = LF_SEPARATE;
  // (the envelope-first local energy maps only six special rows per electron, det.hip)
  r.det = !channels ? DET_VALUE : env_first(d) ? DET_ENV_FIRST : det_precontract(d) ? DET_PRECONTRACT : DET_DIRECT;
  r.orbital = r.det == DET_ENV_FIRST ? ORB_NONE : ORB_GEMM;

  if (!channels && nt && gemm_ln_supported(D, D)) {
    // log psi, D = 256: each GEMM carries its LayerNorm in the epilogue, in place over h; in
    // split-bf16 arithmetic in the epilogue of gemm_x6_ln (96-row tiles of 3 x 4 waves: 34 / 38 us
    // at 24576 x 256 x 256 against 43 / 47 us for the exact-f32 gemm_ln_kernel;
    // tools/ln_gemm_bench.py on MI355X)
    r.form0 = r.form1 = LF_LN_EPILOGUE;
    // split-bf16: layer 1's residual h = features W0 is formed in the epilogue of its
    // LayerNorm GEMM from geo, so the input kernel only writes the geometry
    r.h0_epilogue = fused && x6;
    // split-bf16: each layer's tail (Wo Wl + LN1, Wm + LN2) and the next linear map (the next
    // layer's q|k|v, or the orbitals) run as ONE launch (chain_x6s_kernel).
    // Its 96-row tiles suit up to ~64K walker rows (C2 24576: 256 tiles, C4 40960: 427); at
    // C5 (81920 rows, 2320 orbital columns) the separate GEMMs with 128-row LayerNorm tiles are
    // faster (102.6 vs 103.6 ms per step, tools/chain_bench.py, profiles/)
    // At N = 20 (C5) the chain is taken past 64K rows too (round 6): layer 1 with its attention in
    // the prologue (attention, two LayerNorm GEMMs and layer 2's q|k|v in one launch), layer 2 with
    // the 2320-column orbital map as its last pass (C5 73.5 -> 74.2 K E_L/s, 2.53 -> 2.59 M
    // walker-steps/s same box, profiles/r06_v35_chain_big20_ab.txt)
    // (d.N >= 20 also covers N > 20, where chain_attn_supported is false: those run the chain
    // past 64K rows WITHOUT the attention prologue, in 96-row tiles, which nothing has measured;
    // only N = 20 was.  Kept as it is: no route changes here.)
    if (d.L > 0 && x6 && D == 256 && (rows < 65536 || d.N >= 20)) {
      // layer 1's attention runs in the chain kernel's prologue (its o never leaves the CU;
      // attn_val.h), contracting the o~ planes with U (K = 32)
      r.form0 = fused && chain_attn_supported(d.N, d.H, d.dh) ? LF_CHAIN_ATTN : LF_CHAIN;
      r.form1 = LF_CHAIN;
      r.ofeat = r.form0 == LF_CHAIN_ATTN;
      r.qkv_gemm = 0;  // a chained layer's last pass wrote the next layer's q|k|v
      r.orbital = ORB_IN_CHAIN;
    }
  } else if (channels) {
    r.ofeat = fused;  // layer 1's o~ rows (attention_feat2_kernel, the MFMA kernel) against U
    // split-bf16, D = 256, N <= 6: GEMM + channel LayerNorm fused per map, in place over h
    // (gemm_lnch.hip; the GEMM output never reaches HBM); layer 1 whole in one launch from the
    // o~ rows at H = 4 (MODE 2: LN1, Wm and tanh_ch in coefficient space, the residual h1 from
    // the same 32-deep rows, LN2).  The unfused mode keeps the separate form: tests
    if (x6 && C == 2 * d.N + 5 && !unfused && gemm_lnch_supported(d.N, D)) {
      r.form0 = fused && d.H == 4 ? LF_LNCH_WHOLE : LF_LNCH_PAIR;
      r.form1 = LF_LNCH_PAIR;
      r.h0_epilogue = fused;  // h0 = f W0 formed in the first launch's epilogue from geo
    } else if (fused && D == 256 && (d.N == 10 || d.N == 20)) {
      // N = 10, 20 (GEMM + layernorm_ch_quad): the same residual formed by the first LayerNorm
      // launch, the GEMM writing t without it
      r.h0_epilogue = 1;
      // layer 1 in one launch from the o~ rows (layernorm.hip layer1_ch_kernel: LN_ch1, Wm in
      // coefficient space, tanh_ch, LN_ch2), which reads V^T (derive_weights: dh = 64, H = 4);
      // the unfused mode keeps the two-kernel form: tests
      if (d.dh == 64 && d.H == 4 && layer1_ch_supported(d) && !unfused) r.form0 = LF_L1CH;
    }
  }
  r.input_h = !r.h0_epilogue;
  // log psi with nothing but the geometry to write: the MCMC proposal has written it already
  r.input_skip = !channels && r.h0_epilogue;
  // log psi whose last layer is a chain launch (chain_x6s_kernel<0>) with the orbital map as its
  // last pass: the value kernel's work runs as that launch's tail, on F rows still in LDS, when
  // the value kernel would take its two-walkers-per-wave form (each of the tile's 8 waves then
  // owns whole walker pairs: 96 / N is even for every N that form takes), the tile holds whole
  // walkers, the orbital map is one 256-column pass (a second pass would still read the planes
  // the F tile overwrites) and the F tile and the 16 walker regions fit the dead planes
  const int last_form = d.L > 1 ? r.form1 : r.form0;
  r.det_in_chain = g_det_in_chain.load() && !channels && d.L > 0 && last_form == LF_CHAIN && r.orbital == ORB_IN_CHAIN &&
                   det_value_half_wave(d) && kChainTileRows % d.N == 0 && d.orb_cols <= 256 &&
                   (size_t)kChainTileRows * det_chain_ldf(d) * 4 + 16 * (size_t)det_value_per(d) * 4 <= kChainPlaneBytes;
  return r;
}

}  // namespace dh
