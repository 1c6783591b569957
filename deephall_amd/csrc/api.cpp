// C ABI of the MI355X-native DeepHall VMC inner loop (include/deephall_amd.h).
// Sequences the HIP kernels of one Psiformer pass:
//
//   input (features x W0) -> per layer [ QKV GEMM -> attention -> (O.Wl) GEMM + residual
//   -> LayerNorm -> MLP GEMM -> tanh + residual + LayerNorm ] -> orbital GEMM -> det
//
// with either 1 channel (log psi, MCMC) or 2N+5 channels (local energy).  The gradient side: api_grad.cpp.
#include <cmath>
#include <cstring>

#include "api_internal.h"

using namespace dh;

thread_local std::string dh::g_err;

namespace {

// Workspace of one pass (floats), carved from the caller's buffer, and the route the pass takes.
struct Work {
  float *h, *qkv, *o, *t, *F, *geo, *x2, *logpsi, *lp;
  int32_t* nacc;
  size_t total_bytes;
  TrunkRoute route;
};

// envelope first (det.hip): floats of S, FS, E2, Weff for nw walkers (each padded to 256 rows)
size_t env_first_floats(const Dims& d, int nw) {
  const size_t ne = (size_t)nw * d.N, r6 = (size_t)round_up((int)(6 * ne), 256), r1 = (size_t)round_up((int)ne, 256);
  return align64(r6 * 256) + align64(r6 * d.ld_orb) + align64(r1 * env_first_k(d)) + align64(r1 * 256 * 2 * d.N);
}

Work carve(const Dims& d, int gemm_mode, int nw, int C, void* base) {
  const int rows = nw * d.N * C;
  const TrunkRoute route = trunk_route(d, gemm_mode, C, rows);
  // + CH_BM rows: the channel chain's electron-aligned 96-row tiles read past the last row
  const size_t rp = (size_t)round_up(std::max(rows, 1) + 96, kWalkerRowPad);
  const size_t nh = align64(rp * d.D);
  size_t nqkv = align64(rp * (size_t)std::max(3 * d.D, d.ld_orb));
  if (route.det == DET_ENV_FIRST)  // no F over the channel rows: S, FS, E2, Weff share the q|k|v buffer
    nqkv = align64(std::max(rp * (size_t)(3 * d.D), env_first_floats(d, nw)));
  Work w{};
  w.route = route;
  Carver c{reinterpret_cast<float*>(base)};
  w.h = c.take(nh);
  w.qkv = c.take(nqkv);
  w.o = c.take(nh);
  w.t = c.take(nh);
  // orbital features reuse the QKV buffer (free after the last attention)
  w.F = route.orbital == ORB_NONE ? nullptr : w.qkv;
  w.geo = c.take((size_t)nw * d.N * 4);
  w.x2 = c.take((size_t)nw * d.N * 2);
  w.logpsi = c.take((size_t)nw * 2);
  w.lp = c.take((size_t)nw);
  w.nacc = reinterpret_cast<int32_t*>(c.take((size_t)nw));
  w.total_bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" {

const char* dh_last_error(void) { return g_err.c_str(); }
const char* dh_version(void) { return "deephall_amd 0.1 (gfx950)"; }

int dh_create(const dh_config* cfg, dh_handle** out) {
  if (!cfg || !out) return fail(DH_EINVAL, "null argument");
  if (cfg->struct_size != sizeof(dh_config))
    return fail(DH_EINVAL, "dh_config.struct_size must equal sizeof(dh_config) (" + std::to_string(sizeof(dh_config)) +
                               " bytes); the caller's binding has a different layout");
  if (cfg->network_type != DH_NETWORK_PSIFORMER) return create_trial(cfg, out);  // api_trial.cpp
  const int N = cfg->n_up + cfg->n_dn;
  if (cfg->n_up < 0 || cfg->n_dn < 0 || N < 1 || N > 32) return fail(DH_EINVAL, "need 1 <= N <= 32 electrons");
  if (cfg->flux < 0 || cfg->flux > 126) return fail(DH_EINVAL, "need 0 <= flux <= 126");
  if (cfg->num_layers < 0 || cfg->num_layers > 16) return fail(DH_EINVAL, "need num_layers <= 16");
  if (cfg->ndets < 1 || cfg->ndets > 16) return fail(DH_EINVAL, "need 1 <= determinants <= 16");
  if (cfg->num_heads < 1 || cfg->heads_dim < 1) return fail(DH_EINVAL, "bad attention shape");
  if (cfg->orbital_type != DH_ORBITAL_FULL && cfg->orbital_type != DH_ORBITAL_SPARSE)
    return fail(DH_EINVAL, "orbital type must be DH_ORBITAL_FULL or DH_ORBITAL_SPARSE");
  if (cfg->interaction_type != DH_INTERACTION_COULOMB && cfg->interaction_type != DH_INTERACTION_HARMONIC)
    return fail(DH_EINVAL, "bad interaction type");
  const int D = cfg->num_heads * cfg->heads_dim;
  if (D % 4 != 0) return fail(DH_EINVAL, "num_heads * heads_dim must be a multiple of 4");
  if (cfg->flux == 0 && cfg->interaction_type == DH_INTERACTION_HARMONIC)
    return fail(DH_EINVAL, "harmonic potential needs flux > 0");
  auto* h = new dh_handle();
  h->cfg = *cfg;
  Dims& d = h->d;
  d.N = N;
  d.n_up = cfg->n_up;
  d.n_dn = cfg->n_dn;
  d.T = 2 * N;
  d.C = 2 * N + 5;
  d.M = cfg->flux + 1;
  d.Q = 0.5f * cfg->flux;
  d.r = cfg->radius > 0.f ? cfg->radius : std::sqrt(d.Q);
  d.H = cfg->num_heads;
  d.dh = cfg->heads_dim;
  d.D = D;
  d.L = cfg->num_layers;
  d.K = cfg->ndets;
  d.NB = (cfg->n_dn > 0 && cfg->n_up > 0) ? 2 : 1;
  d.orb_cols = d.NB * 2 * d.M * N * d.K;
  d.ld_orb = round_up(d.orb_cols, 128);
  d.interaction = cfg->interaction_type;
  d.lambda = cfg->interaction_strength;
  d.sparse = cfg->orbital_type == DH_ORBITAL_SPARSE;
  // packed layout
  std::vector<size_t> sizes;
  sizes.push_back((size_t)4 * D);
  for (int l = 0; l < d.L; ++l) {
    sizes.push_back((size_t)D * 3 * D);
    sizes.push_back((size_t)3 * D);
    sizes.push_back((size_t)D * D);
    sizes.push_back((size_t)D);
    sizes.push_back((size_t)2 * D);
    sizes.push_back((size_t)D * D);
    sizes.push_back((size_t)D);
    sizes.push_back((size_t)2 * D);
  }
  sizes.push_back((size_t)D * d.ld_orb);
  sizes.push_back((size_t)d.ld_orb);
  sizes.push_back(2);
  sizes.push_back((size_t)4 * 3 * D);  // W0 @ Wqkv of layer 0 (folded input projection)
  size_t off = 0;
  for (size_t s : sizes) {
    h->offsets.push_back(off);
    off += align64(s);
  }
  h->offsets.push_back(off);
  // reference parameter tree, flattened in SURVEY.md Appendix B order (ref_seg below)
  {
    const size_t DD = (size_t)D * D, FNK = (size_t)(d.sparse ? kSparseFeatures : d.M) * N * d.K;
    std::vector<size_t> rs;
    rs.push_back((size_t)4 * D);
    for (int l = 0; l < d.L; ++l)
      for (size_t v : {DD, (size_t)D, DD, (size_t)D, DD, (size_t)D, DD, (size_t)D, DD, (size_t)D, (size_t)D, DD,
                       (size_t)D, (size_t)D, (size_t)D})
        rs.push_back(v);
    for (int i = 0; i < 2 * d.NB; ++i) {
      rs.push_back((size_t)D * FNK);
      rs.push_back(FNK);
    }
    if (d.sparse) {  // Orbitals_0/lll_weight
      rs.push_back((size_t)kSparseFeatures * d.M);
      rs.push_back((size_t)d.M);
    }
    rs.push_back(1);
    rs.push_back(1);
    size_t ro = 0;
    for (size_t v : rs) {
      h->ref_offsets.push_back(ro);
      ro += align64(v);
    }
    h->ref_offsets.push_back(ro);
  }
  // monopole-harmonic normalisation sqrt(C(2Q, Q-m)) (blocks.py:45-46), index p = Q+m
  std::vector<float> norm(d.M);
  for (int p = 0; p < d.M; ++p) {
    const int n = d.M - 1, k = d.M - 1 - p;
    const double lc = std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0);
    norm[p] = (float)std::sqrt(std::exp(lc));
  }
  h->norm_host = norm;  // uploaded by dh_set_params (dh_create makes no HIP calls)
  *out = h;
  return DH_OK;
}

void dh_destroy(dh_handle* h) {
  if (!h) return;
  for (auto& r : h->prof.recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  if (h->params) (void)hipFree(h->params);
  if (h->norm) (void)hipFree(h->norm);
  if (h->wt) (void)hipFree(h->wt);
  if (h->wp) (void)hipFree(h->wp);
  if (h->mqk) (void)hipFree(h->mqk);
  if (h->ofw) (void)hipFree(h->ofw);
  if (h->ofp) (void)hipFree(h->ofp);
  if (h->l1w) (void)hipFree(h->l1w);
  if (h->w2t) (void)hipFree(h->w2t);
  if (h->w2p) (void)hipFree(h->w2p);
  if (h->l1p) (void)hipFree(h->l1p);
  if (h->ref) (void)hipFree(h->ref);
  if (h->wb) (void)hipFree(h->wb);
  if (h->wbt) (void)hipFree(h->wbt);
  if (h->trial.table) (void)hipFree(h->trial.table);
  if (h->kfac) {
    if (h->kfac->dev_mem) (void)hipFree(h->kfac->dev_mem);
    delete h->kfac;
  }
  delete h;
}

int dh_param_layout(const dh_handle* h, size_t* offsets, int n) {
  if (!h) return fail(DH_EINVAL, "null handle");
  const int nseg = (int)h->offsets.size() - 1;
  for (int i = 0; i < n && i <= nseg; ++i) offsets[i] = h->offsets[i];
  return nseg;
}

}  // extern "C"

namespace {

// Device pointers of the packed segments.
void assign_packed(dh_handle* h) {
  const Dims& d = h->d;
  const float* P = h->params;
  int s = 0;
  h->p.W0 = P + h->offsets[s++];
  for (int l = 0; l < d.L; ++l) {
    LayerParams& lp = h->p.layer[l];
    lp.Wqkv = P + h->offsets[s++];
    lp.bqkv = P + h->offsets[s++];
    lp.Wol = P + h->offsets[s++];
    lp.bol = P + h->offsets[s++];
    lp.ln1 = P + h->offsets[s++];
    lp.Wm = P + h->offsets[s++];
    lp.bm = P + h->offsets[s++];
    lp.ln2 = P + h->offsets[s++];
  }
  h->p.Worb = P + h->offsets[s++];
  h->p.borb = P + h->offsets[s++];
  h->p.jastrow = P + h->offsets[s++];
  h->p.W0qkv = P + h->offsets[s++];
}

// Derived weight copies: transposed + split-bf16 planes for the forward NT/x6 GEMMs, and the
// backward copies (planes of the untransposed weights, or W^T when D % 32 != 0).
int derive_weights(dh_handle* h, hipStream_t st) {
  const Dims& d = h->d;
  const int D = d.D;
  if (d.L > 0 && d.dh == 64) {  // layer 1's score forms of the feature-space attention
    if (!h->mqk) HIP_TRY(hipMalloc(&h->mqk, (size_t)d.H * kMqkStride * sizeof(float)));
    launch_lowrank_qk(d, h->p.W0qkv, h->p.layer[0].bqkv, h->mqk, st);
    h->p.Mqk = h->mqk;
    // layer 1's attention output in feature space (round 6): o = o~ Wv~, so o Wol = o~ U with
    // U = Wv~ Wol per head (8 H rows, zero padded to KO); the NT / x6 kernels read U^T
    const int KO = ofeat_k(d);
    const size_t nu = (size_t)round_up(d.D, kRowPad) * KO;
    if (!h->ofw) HIP_TRY(hipMalloc(&h->ofw, nu * sizeof(float)));
    if (!h->ofp) HIP_TRY(hipMalloc(&h->ofp, (size_t)3 * x6_plane_rows(d.D) * KO * sizeof(uint16_t)));
    HIP_TRY(hipMemsetAsync(h->ofw, 0, nu * sizeof(float), st));
    launch_ofeat_weight(d, h->p.W0qkv, h->p.layer[0].bqkv, h->p.layer[0].Wol, h->ofw, st);
    launch_split_planes(h->ofw, KO, d.D, KO, h->ofp, st);
    h->p.UT = h->ofw;
    h->p.UP = h->ofp;
    // layer 1 in coefficient space (gemm_lnch MODE 2): B^T, V^T [256 pad][32] and their planes
    if (d.H == 4) {
      const size_t nb = (size_t)round_up(d.D, kRowPad) * 32, pb = (size_t)3 * x6_plane_rows(d.D) * 32;
      if (!h->l1w) HIP_TRY(hipMalloc(&h->l1w, 2 * nb * sizeof(float)));
      if (!h->l1p) HIP_TRY(hipMalloc(&h->l1p, 2 * pb * sizeof(uint16_t)));
      HIP_TRY(hipMemsetAsync(h->l1w, 0, 2 * nb * sizeof(float), st));
      const LayerParams& l0 = h->p.layer[0];
      launch_l1_basis(d, h->p.W0, h->ofw, l0.bol, l0.ln1, l0.Wm, l0.bm, h->l1w, h->l1w + nb, st);
      launch_split_planes(h->l1w, 32, d.D, 32, h->l1p, st);
      launch_split_planes(h->l1w + nb, 32, d.D, 32, h->l1p + pb, st);
      h->p.L1BP = h->l1p;
      h->p.L1VP = h->l1p + pb;
      h->p.L1VT = h->l1w + nb;
    }
  }
  if (d.D % 32 == 0) {
    // Transposed copies Wt[n][k] (rows zero-padded to 256) of every GEMM weight, for the
    // NT GEMM kernels whose LDS-DMA staging wants k contiguous in both operands.
    const size_t sq = (size_t)round_up(D, kRowPad) * D, sqkv = (size_t)round_up(3 * D, kRowPad) * D;
    const size_t sorb = (size_t)round_up(d.orb_cols, kRowPad) * D;
    const size_t total = (size_t)d.L * (sqkv + 2 * sq) + sorb;
    if (!h->wt) HIP_TRY(hipMalloc(&h->wt, total * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->wt, 0, total * sizeof(float), st));
    float* q = h->wt;
    for (int l = 0; l < d.L; ++l) {
      LayerParams& lp = h->p.layer[l];
      launch_transpose(lp.Wqkv, 3 * D, D, 3 * D, q, D, st);
      lp.WqkvT = q;
      q += sqkv;
      launch_transpose(lp.Wol, D, D, D, q, D, st);
      lp.WolT = q;
      q += sq;
      launch_transpose(lp.Wm, D, D, D, q, D, st);
      lp.WmT = q;
      q += sq;
    }
    launch_transpose(h->p.Worb, d.ld_orb, D, d.orb_cols, q, D, st);
    h->p.WorbT = q;
    // split-bf16 planes of the same weights (gemm_x6.hip), from the transposed copies
    const size_t pq = (size_t)3 * x6_plane_rows(3 * D) * D, pd = (size_t)3 * x6_plane_rows(D) * D;
    const size_t po = (size_t)3 * x6_plane_rows(d.orb_cols) * D;
    const size_t ptotal = (size_t)d.L * (pq + 2 * pd) + po;
    if (!h->wp) HIP_TRY(hipMalloc(&h->wp, ptotal * sizeof(uint16_t)));
    uint16_t* w = h->wp;
    for (int l = 0; l < d.L; ++l) {
      LayerParams& lp = h->p.layer[l];
      launch_split_planes(lp.WqkvT, D, 3 * D, D, w, st);
      lp.WqkvP = w;
      w += pq;
      launch_split_planes(lp.WolT, D, D, D, w, st);
      lp.WolP = w;
      w += pd;
      launch_split_planes(lp.WmT, D, D, D, w, st);
      lp.WmP = w;
      w += pd;
    }
    launch_split_planes(h->p.WorbT, D, d.orb_cols, D, w, st);
    h->p.WorbP = w;
    if (env_first(d)) {  // envelope first (C4 / C5): the envelope-coefficient map of Worb
      const int KE = env_first_k(d), n2 = 256 * 2 * d.N;
      if (!h->w2t) HIP_TRY(hipMalloc(&h->w2t, (size_t)n2 * KE * sizeof(float)));
      if (!h->w2p) HIP_TRY(hipMalloc(&h->w2p, (size_t)3 * x6_plane_rows(n2) * KE * sizeof(uint16_t)));
      launch_env_w2(d, h->p.Worb, h->w2t, st);
      launch_split_planes(h->w2t, KE, n2, KE, h->w2p, st);
      h->p.W2T = h->w2t;
      h->p.W2P = h->w2p;
    }
    // backward planes: the untransposed W [K = D][n] read as a transposed weight with D
    // output rows and contraction length n (dX = dY W^T)
    const int pr = x6_plane_rows(D);
    const size_t bq = (size_t)3 * pr * 3 * D, bd = (size_t)3 * pr * D, bo = (size_t)3 * pr * d.ld_orb;
    const size_t btotal = (size_t)d.L * (bq + 2 * bd) + bo;
    if (!h->wb) HIP_TRY(hipMalloc(&h->wb, btotal * sizeof(uint16_t)));
    uint16_t* b = h->wb;
    for (int l = 0; l < d.L; ++l) {
      LayerParams& lp = h->p.layer[l];
      launch_split_planes(lp.Wqkv, 3 * D, D, 3 * D, b, st);
      lp.WqkvB = b;
      b += bq;
      launch_split_planes(lp.Wol, D, D, D, b, st);
      lp.WolB = b;
      b += bd;
      launch_split_planes(lp.Wm, D, D, D, b, st);
      lp.WmB = b;
      b += bd;
    }
    launch_split_planes(h->p.Worb, d.ld_orb, D, d.ld_orb, b, st);
    h->p.WorbB = b;
  } else {
    // exact-f32 backward: W^T [n][D]
    const size_t total = (size_t)d.L * (5 * (size_t)D * D) + (size_t)d.ld_orb * D;
    if (!h->wbt) HIP_TRY(hipMalloc(&h->wbt, total * sizeof(float)));
    HIP_TRY(hipMemsetAsync(h->wbt, 0, total * sizeof(float), st));
    float* q = h->wbt;
    for (int l = 0; l < d.L; ++l) {
      LayerParams& lp = h->p.layer[l];
      launch_transpose(lp.Wqkv, 3 * D, D, 3 * D, q, D, st);
      lp.WqkvBT = q;
      q += (size_t)3 * D * D;
      launch_transpose(lp.Wol, D, D, D, q, D, st);
      lp.WolBT = q;
      q += (size_t)D * D;
      launch_transpose(lp.Wm, D, D, D, q, D, st);
      lp.WmBT = q;
      q += (size_t)D * D;
    }
    launch_transpose(h->p.Worb, d.ld_orb, D, d.orb_cols, q, D, st);
    h->p.WorbBT = q;
  }
  HIP_TRY(hipGetLastError());
  return DH_OK;
}

int ensure_param_buffers(dh_handle* h) {
  if (!h->params) HIP_TRY(hipMalloc(&h->params, h->offsets.back() * sizeof(float)));
  if (!h->norm) {
    HIP_TRY(hipMalloc(&h->norm, h->norm_host.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(h->norm, h->norm_host.data(), h->norm_host.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return DH_OK;
}

// Pack the reference tree (h->ref) into the kernel layout: concatenations, zero padding and
// the three folds (Wo Wl, bo Wl, W0 Wqkv) as double-accumulated products.
void pack_from_ref(dh_handle* h, hipStream_t st) {
  const Dims& d = h->d;
  const int D = d.D, MNK = d.M * d.N * d.K;
  const RefSeg R{d.L, d.NB, d.sparse};
  auto ref = [&](int seg) { return h->ref + h->ref_offsets[seg]; };
  auto pk = [&](int seg) { return h->params + h->offsets[seg]; };
  launch_copy2d(ref(R.W0()), D, pk(0), D, 4, D, st);
  for (int l = 0; l < d.L; ++l) {
    const int b = 1 + 8 * l;
    for (int part = 0; part < 3; ++part) {
      launch_copy2d(ref(R.lay(l, RWq + 2 * part)), D, pk(b + 0) + part * D, 3 * D, D, D, st);
      launch_copy2d(ref(R.lay(l, Rbq + 2 * part)), D, pk(b + 1) + part * D, 3 * D, 1, D, st);
    }
    launch_small_gemm(D, D, D, ref(R.lay(l, RWo)), D, 0, ref(R.lay(l, RWl)), D, 0, pk(b + 2), D, 0, st);
    launch_small_gemm(1, D, D, ref(R.lay(l, Rbo)), D, 0, ref(R.lay(l, RWl)), D, 0, pk(b + 3), D, 0, st);
    launch_copy2d(ref(R.lay(l, Rln1s)), D, pk(b + 4), D, 1, D, st);
    launch_copy2d(ref(R.lay(l, Rln1b)), D, pk(b + 4) + D, D, 1, D, st);
    launch_copy2d(ref(R.lay(l, RWm)), D, pk(b + 5), D, D, D, st);
    launch_copy2d(ref(R.lay(l, Rbm)), D, pk(b + 6), D, 1, D, st);
    launch_copy2d(ref(R.lay(l, Rln2s)), D, pk(b + 7), D, 1, D, st);
    launch_copy2d(ref(R.lay(l, Rln2b)), D, pk(b + 7) + D, D, 1, D, st);
  }
  const int so = 1 + 8 * d.L;
  launch_copy2d(nullptr, 0, pk(so), d.ld_orb, D, d.ld_orb, st);
  launch_copy2d(nullptr, 0, pk(so + 1), d.ld_orb, 1, d.ld_orb, st);
  for (int i = 0; i < 2 * d.NB; ++i) {
    if (d.sparse)  // fold lll_weight into the full layout (blocks.py:52-62)
      launch_sparse_fold(ref(R.orb_kernel(i)), ref(R.orb_bias(i)), ref(R.lll(0)), ref(R.lll(1)), i % 2 == 0, D,
                         d.N * d.K, d.M, pk(so) + i * MNK, d.ld_orb, pk(so + 1) + i * MNK, st);
    else {
      launch_copy2d(ref(R.orb_kernel(i)), MNK, pk(so) + i * MNK, d.ld_orb, D, MNK, st);
      launch_copy2d(ref(R.orb_bias(i)), MNK, pk(so + 1) + i * MNK, d.ld_orb, 1, MNK, st);
    }
  }
  launch_copy2d(ref(R.jas(0)), 1, pk(so + 2), 1, 1, 1, st);
  launch_copy2d(ref(R.jas(1)), 1, pk(so + 2) + 1, 1, 1, 1, st);
  if (d.L > 0) launch_small_gemm(4, 3 * D, D, pk(0), D, 0, pk(1), 3 * D, 0, pk(so + 3), 3 * D, 0, st);
}

}  // namespace

extern "C" {

int dh_set_params(dh_handle* h, const float* params, size_t count, void* stream) {
  if (h && h->analytic()) return count == 0 ? DH_OK : fail(DH_EINVAL, "the Laughlin wavefunction has no parameters");
  if (!h || !params) return fail(DH_EINVAL, "null argument");
  if (count != h->offsets.back()) return fail(DH_EINVAL, "parameter count mismatch");
  if (int rc = ensure_param_buffers(h)) return rc;
  HIP_TRY(hipMemcpyAsync(h->params, params, count * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  assign_packed(h);
  if (int rc = derive_weights(h, (hipStream_t)stream)) return rc;
  h->params_set = true;
  h->ref_set = false;  // a packed upload has no reference tree (the VJP needs one)
  return DH_OK;
}

int dh_ref_layout(const dh_handle* h, size_t* offsets, int n) {
  if (!h) return fail(DH_EINVAL, "null handle");
  const int nseg = (int)h->ref_offsets.size() - 1;
  for (int i = 0; i < n && i <= nseg; ++i) offsets[i] = h->ref_offsets[i];
  return nseg;
}

int dh_set_params_ref(dh_handle* h, const float* ref, size_t count, void* stream) {
  if (h && h->analytic()) return count == 0 ? DH_OK : fail(DH_EINVAL, "the Laughlin wavefunction has no parameters");
  if (!h || !ref) return fail(DH_EINVAL, "null argument");
  if (count != h->ref_offsets.back()) return fail(DH_EINVAL, "reference parameter count mismatch");
  if (int rc = ensure_param_buffers(h)) return rc;
  if (!h->ref) HIP_TRY(hipMalloc(&h->ref, count * sizeof(float)));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(h->ref, ref, count * sizeof(float), hipMemcpyDeviceToDevice, st));
  pack_from_ref(h, st);
  HIP_TRY(hipGetLastError());
  assign_packed(h);
  if (int rc = derive_weights(h, st)) return rc;
  h->params_set = true;
  h->ref_set = true;
  return DH_OK;
}

int dh_set_gemm_mode(dh_handle* h, int mode) {
  if (!h) return fail(DH_EINVAL, "null handle");
  if (mode != DH_GEMM_F32 && mode != DH_GEMM_X6 && mode != DH_GEMM_X6_ALL && mode != DH_GEMM_X6_ALL_UNFUSED)
    return fail(DH_EINVAL, "bad GEMM mode");
  h->gemm_mode = mode;
  return DH_OK;
}

size_t dh_workspace_bytes(const dh_handle* h, int batch, int op) {
  if (!h || batch < 1) return 0;
  return carve(h->d, h->gemm_mode, batch, op == 1 ? h->d.C : 1, nullptr).total_bytes;
}

}  // extern "C"

namespace {

// One Psiformer pass over nw walkers with C channels, walking its TrunkRoute.
struct Trunk {
  dh_handle* h;
  const Dims& d;
  const Params& P;
  const Work& w;
  hipStream_t s;
  const int nw, C, rows;
  const TrunkRoute r;
  const bool keep_h;
  // the value kernel's work as the tail of the last layer's chain launch (route.det_in_chain;
  // null: F to HBM for a launch of its own); keep_F: the tail's launch writes F to HBM as well
  const ChainDet* det = nullptr;
  const bool keep_F = false;
  const int D = d.D, KO = ofeat_k(d);  // KO: layer 1's o~ row length
  const int ch = C > 1 ? PK_CH : 0;    // profiler class offset of channel-row launches
  const double R = rows, DD = D, f4 = 4.0;

  void gemm(const float* X, int ldx, const float* W, const float* Wt, const uint16_t* Wp, int ldw, const float* bias,
            const float* Res, int ldr, float* Y, int ldy, int ncols, int K) const {
    PROF(PK_GEMM + ch, 2.0 * R * ncols * K, f4 * (R * K + (double)K * ncols + R * ncols * (Res ? 2 : 1)));
    dense_gemm(r.family, X, ldx, W, Wt, Wp, ldw, bias, Res, ldr, Y, ldy, rows, ncols, K, C, s);
  }
  X6Feat h0_feat(int l) const { return (r.h0_epilogue && l == 0) ? X6Feat{P.W0, w.geo, d.N, d.n_up} : X6Feat{}; }

  // log psi: Wo Wl + LN1, Wm + LN2 and the next linear map (the next layer's q|k|v, or the
  // orbitals) in one launch; attn: layer 1's attention in its prologue
  void layer_chain(int l, bool attn) const {
    const LayerParams& lp = P.layer[l];
    const bool last = l + 1 == d.L;
    const int n3 = last ? d.orb_cols : 3 * D;
    PROF(PK_GEMM, 2.0 * R * DD * (2.0 * DD + n3), f4 * (2.0 * R * DD + R * n3 + 2.0 * DD * DD + DD * n3));
    X6Feat feat = h0_feat(l);
    if (attn) {
      feat.W0qkv = P.W0qkv;
      feat.bqkv = lp.bqkv;
      feat.Mqk = P.Mqk;
      feat.L1V = P.L1VP;
      feat.L1B = P.L1BP;
    }
    // layer 1 with its attention in the prologue: P1 contracts the o~ planes with U (K = 32)
    launch_chain_x6(w.o, attn ? P.UP : lp.WolP, x6_plane_rows(D), lp.bol, lp.ln1, lp.WmP, x6_plane_rows(D), lp.bm,
                    lp.ln2, last ? P.WorbP : P.layer[l + 1].WqkvP, x6_plane_rows(n3),
                    last ? P.borb : P.layer[l + 1].bqkv, n3, last ? w.F : w.qkv, last ? d.ld_orb : 3 * D, w.h, rows,
                    feat, s, /*store_h=*/!last || keep_h,  // the last layer's h is dead: only its orbitals are read
                    last ? det : nullptr, /*store_F=*/!(last && det) || keep_F);
  }
  // log psi: each GEMM carries its LayerNorm in the epilogue, in place over h
  void layer_ln_epilogue(int l) const {
    const LayerParams& lp = P.layer[l];
    const bool x6 = r.family == GEMM_X6;
    {
      PROF(PK_GEMM, 2.0 * R * DD * DD, f4 * (3.0 * R * DD + DD * DD));
      if (x6)
        launch_gemm_x6_ln(w.o, D, lp.WolP, x6_plane_rows(D), lp.bol, lp.ln1, w.h, rows, D, 0, 0, s, h0_feat(l));
      else
        launch_gemm_ln(w.o, D, lp.WolT, D, lp.bol, lp.ln1, w.h, rows, D, 0, 0, s);
    }
    PROF(PK_GEMM, 2.0 * R * DD * DD, f4 * (2.0 * R * DD + DD * DD));
    if (x6)
      launch_gemm_x6_ln(w.h, D, lp.WmP, x6_plane_rows(D), lp.bm, lp.ln2, w.h, rows, D, 1, 0, s);
    else
      launch_gemm_ln(w.h, D, lp.WmT, D, lp.bm, lp.ln2, w.h, rows, D, 1, 0, s);
  }
  // channel rows: each linear map and its channel LayerNorm in one launch, in place over h
  void layer_lnch(int l) const {
    const LayerParams& lp = P.layer[l];
    {
      // layer 1 (fused attention): the o~ rows against U, K = ofeat_k
      const bool of = r.ofeat && l == 0;
      const double KK = of ? KO : DD;
      PROF(PK_GEMM + PK_CH, 2.0 * R * DD * KK, f4 * (R * KK + 2.0 * R * DD + DD * KK));
      launch_gemm_lnch(d.N, w.o, of ? P.UP : lp.WolP, x6_plane_rows(D), lp.bol, lp.ln1, w.geo, w.h, nw * d.N, 0, s,
                       (r.h0_epilogue && l == 0) ? P.W0 : nullptr, d.n_up, of ? KO : D);
    }
    PROF(PK_GEMM + PK_CH, 2.0 * R * DD * DD, f4 * (3.0 * R * DD + DD * DD));
    launch_gemm_lnch(d.N, w.h, lp.WmP, x6_plane_rows(D), lp.bm, lp.ln2, w.geo, w.h, nw * d.N, 1, s);
  }
  // channel rows: layer 1 whole in one launch from the o~ rows (gemm_lnch MODE 2)
  void layer_lnch_whole() const {
    const LayerParams& lp = P.layer[0];
    PROF(PK_L1CH, 2.0 * R * DD * 3.0 * KO, f4 * (R * KO + R * DD));
    launch_gemm_lnch(d.N, w.o, P.UP, x6_plane_rows(D), lp.bol, lp.ln2, w.geo, w.h, nw * d.N, 2, s, P.W0, d.n_up, KO,
                     P.L1VP, P.L1BP);
  }
  // channel rows, N = 10, 20: layer 1 whole in one launch from the o~ rows (layer1_ch_kernel)
  void layer_l1ch() const {
    const LayerParams& lp = P.layer[0];
    PROF(PK_L1CH, 2.0 * R * DD * (24.0 + 27.0), f4 * (R * KO + R * DD));
    launch_layer1_ch(d, w.o, P.UT, P.L1VT, P.W0, lp.bol, lp.ln1, lp.ln2, w.geo, w.h, nw, s);
  }
  void layer_separate(int l) const {
    const LayerParams& lp = P.layer[l];
    // t = h + o (Wo Wl) + bo Wl    (psiformer.py:44-45, two adjacent linear maps folded);
    // layer 1 with the residual in the LayerNorm: t = o (Wo Wl) + bo Wl, the LayerNorm adds h0 = f W0
    const bool lf = r.h0_epilogue && l == 0;
    if (r.ofeat && l == 0)  // layer 1's o~ rows against U
      gemm(w.o, KO, nullptr, P.UT, P.UP, KO, lp.bol, lf ? nullptr : w.h, D, w.t, D, D, KO);
    else
      gemm(w.o, D, lp.Wol, lp.WolT, lp.WolP, D, lp.bol, lf ? nullptr : w.h, D, w.t, D, D, D);
    {
      PROF(PK_LN + ch, 0.0, f4 * R * 2.0 * DD);
      launch_layernorm(d, w.t, nullptr, lp.ln1, w.geo, w.h, nw, C, 0, s, lf ? P.W0 : nullptr);
    }
    gemm(w.h, D, lp.Wm, lp.WmT, lp.WmP, D, lp.bm, nullptr, 0, w.o, D, D, D);
    PROF(PK_LN + ch, 0.0, f4 * R * 3.0 * DD);
    launch_layernorm(d, nullptr, w.o, lp.ln2, w.geo, w.h, nw, C, 1, s);
  }

  // geo_ready: w.geo already holds the walkers' geometry (written by the MCMC proposal)
  int run(const float* x, bool geo_ready) const {
    if (!(geo_ready && r.input_skip)) {
      const bool wq = r.input_qkv;
      PROF(PK_INPUT + ch, 8.0 * R * DD * (wq ? 4 : 1), f4 * R * DD * (wq ? 4 : 1));
      launch_input(d, x, P.W0, wq ? P.W0qkv : nullptr, wq ? P.layer[0].bqkv : nullptr, r.input_h ? w.h : nullptr,
                   wq ? w.qkv : nullptr, w.geo, nw, C, s);
    }
    for (int l = 0; l < d.L; ++l) {
      const LayerParams& lp = P.layer[l];
      const int form = l == 0 ? r.form0 : r.form1;
      if (l > 0 && r.qkv_gemm)
        gemm(w.h, D, lp.Wqkv, lp.WqkvT, lp.WqkvP, 3 * D, lp.bqkv, nullptr, 0, w.qkv, 3 * D, 3 * D, D);
      if (form != LF_CHAIN_ATTN) {
        const bool f = r.attn_feat && l == 0;
        PROF(PK_ATTN + ch, 0.0, f4 * R * (f ? 1.0 : 4.0) * DD);
        launch_attention(d, w.qkv, w.geo, w.o, nw, C, s, f ? P.W0qkv : nullptr, f ? lp.bqkv : nullptr,
                         f ? P.Mqk : nullptr);
      }
      switch (form) {
        case LF_CHAIN:
        case LF_CHAIN_ATTN: layer_chain(l, form == LF_CHAIN_ATTN); break;
        case LF_LN_EPILOGUE: layer_ln_epilogue(l); break;
        case LF_LNCH_WHOLE: layer_lnch_whole(); break;
        case LF_LNCH_PAIR: layer_lnch(l); break;
        case LF_L1CH: layer_l1ch(); break;
        default: layer_separate(l); break;
      }
    }
    if (r.orbital == ORB_GEMM)
      gemm(w.h, D, P.Worb, P.WorbT, P.WorbP, d.ld_orb, P.borb, nullptr, 0, w.F, d.ld_orb, d.orb_cols, D);
    return check_launch();
  }
};

// The pass w was carved for: leaves the orbital features in w.F (where the route maps them) and,
// with keep_h, the trunk's h in w.h (the chain form skips the last layer's otherwise).
int run_trunk(dh_handle* h, const float* x, int nw, int C, const Work& w, hipStream_t s, bool geo_ready = false,
              bool keep_h = false, const ChainDet* det = nullptr, bool keep_F = false) {
  return Trunk{h, h->d, h->p, w, s, nw, C, nw * h->d.N * C, w.route, keep_h, det, keep_F}.run(x, geo_ready);
}

// launch_det_value's arguments for a pass whose route carries the determinant tail
ChainDet chain_det(const dh_handle* h, const float* x, int nw, float* logpsi, const McmcEpi& epi) {
  const Dims& d = h->d;
  ChainDet c;
  c.x = x;
  c.jastrow = h->p.jastrow;
  c.norm = h->norm;
  c.logpsi = logpsi;
  c.N = d.N;
  c.n_up = d.n_up;
  c.M = d.M;
  c.K = d.K;
  c.nw = nw;
  c.per = det_value_per(d);
  c.ldf = det_chain_ldf(d);
  c.epi = epi;
  return c;
}

// log psi of nw walkers into logpsi [nw][2]: the Psiformer pass or an analytic state's kernel (launch_trial)
// epi (Psiformer only): the MCMC accept / next proposal fused into the value kernel
int value_pass(dh_handle* h, const float* x, int nw, const Work& w, float* logpsi, hipStream_t s,
               bool geo_ready = false, const McmcEpi& epi = McmcEpi{}) {
  if (h->analytic()) return launch_trial(h, x, logpsi, nullptr, nullptr, nw, s);
  // envelope, Jastrow, determinant, accept and proposal in the last chain launch.  Not while the
  // profiler records (dh_profile_enable): it times kernel classes by events around launches, and
  // the determinant class inside a GEMM-class launch cannot be timed (nor that launch's FLOP
  // rate read), so a profiled pass launches the value kernel on its own: the same bits
  if (w.route.det_in_chain && !h->prof.on) {
    const ChainDet det = chain_det(h, x, nw, logpsi, epi);
    return run_trunk(h, x, nw, 1, w, s, geo_ready, false, &det);
  }
  if (int rc = run_trunk(h, x, nw, 1, w, s, geo_ready)) return rc;
  {
    PROF(PK_DET_VALUE, 0.0, 4.0 * nw * h->d.N * h->d.ld_orb);
    launch_det_value(h->d, w.F, x, h->p.jastrow, h->norm, logpsi, nw, s, epi);
  }
  return check_launch();
}

}  // namespace

extern "C" {

int dh_logpsi(dh_handle* h, const float* x, int B, float* logpsi, void* ws, size_t ws_bytes, void* stream) {
  const size_t need = h ? dh_workspace_bytes(h, B, 0) : 0;
  if (int rc = check_common(h, x, B, ws, ws_bytes, need)) return rc;
  if (!logpsi) return fail(DH_EINVAL, "null output");
  hipStream_t s = (hipStream_t)stream;
  Work w = carve(h->d, h->gemm_mode, B, 1, ws);
  return value_pass(h, x, B, w, logpsi, s);
}

int dh_mcmc_step(dh_handle* h, float* x, float* lp, int32_t* n_accept, int B, int steps, float width, uint64_t seed,
                 uint64_t counter, int64_t walker_offset, const float* noise, void* ws, size_t ws_bytes,
                 void* stream) {
  const size_t need = h ? dh_workspace_bytes(h, B, 0) : 0;
  if (int rc = check_common(h, x, B, ws, ws_bytes, need)) return rc;
  if (!lp || !n_accept || steps < 0) return fail(DH_EINVAL, "bad MCMC arguments");
  hipStream_t s = (hipStream_t)stream;
  const Dims& d = h->d;
  Work w = carve(d, h->gemm_mode, B, 1, ws);
  // initial log-probability (mcmc.py:142)
  if (int rc = value_pass(h, x, B, w, w.logpsi, s)) return rc;
  launch_lp_from_logpsi(w.logpsi, lp, n_accept, B, s);
  const size_t nstride = (size_t)B * (2 * d.N + 1);
  // step st: accept of st - 1 and the proposal of st in one launch (which also writes the
  // proposal's geometry, so the trunk skips its input kernel); the last accept alone
  const bool geo = !h->analytic();
  // Psiformer: step st's accept and step st + 1's proposal run in the epilogue of step st's
  // value kernel (McmcEpi, det.hip): one launch fewer per move, bit-identical results; the
  // analytic states' kernels (launch_trial) keep the separate accept / proposal launches
  const bool fuse = geo;
  for (int st = 0; st < steps; ++st) {
    const float* nz = noise ? noise + st * nstride : nullptr;
    const uint64_t step = counter + (uint64_t)st;
    if (!fuse || st == 0) {
      PROF(PK_MCMC, 0.0, 16.0 * B * d.N);
      if (st == 0)
        launch_propose(d, x, w.x2, B, width, seed, step, walker_offset, nz, 0, s, geo ? w.geo : nullptr);
      else
        launch_accept_propose(d, x, w.x2, geo ? w.geo : nullptr, lp, w.logpsi, n_accept, B, width, seed, step - 1,
                              walker_offset, noise ? noise + (st - 1) * nstride : nullptr, nz, s);
    }
    McmcEpi epi{};
    if (fuse) {
      epi.on = 1;
      epi.propose = st + 1 < steps;
      epi.x = x;
      epi.x2 = w.x2;
      epi.geo = w.geo;
      epi.lp = lp;
      epi.nacc = n_accept;
      epi.width = width;
      epi.seed = seed;
      epi.step = step;
      epi.woff = walker_offset;
      epi.noise = nz;
      epi.noise2 = (noise && st + 1 < steps) ? noise + (st + 1) * nstride : nullptr;
    }
    if (int rc = value_pass(h, w.x2, B, w, w.logpsi, s, geo, epi)) return rc;
  }
  if (steps > 0 && !fuse) {
    PROF(PK_MCMC, 0.0, 16.0 * B * d.N);
    launch_accept(d, x, w.x2, lp, w.logpsi, n_accept, B, seed, counter + (uint64_t)(steps - 1), walker_offset,
                  noise ? noise + (steps - 1) * nstride : nullptr, 0, s);
  }
  return check_launch();
}

int dh_local_energy(dh_handle* h, const float* x, int B, float* e_l, float* obs, void* ws, size_t ws_bytes,
                    void* stream) {
  const size_t need1 = h ? dh_workspace_bytes(h, 1, 1) : 0;
  if (int rc = check_common(h, x, B, ws, ws_bytes, need1)) return rc;
  if (!e_l || !obs) return fail(DH_EINVAL, "null output");
  const Dims& d = h->d;
  if (h->analytic()) return launch_trial(h, x, nullptr, e_l, obs, B, (hipStream_t)stream);
  // largest chunk that fits the workspace
  int chunk = B;
  while (chunk > 1 && dh_workspace_bytes(h, chunk, 1) > ws_bytes) chunk = (chunk + 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nw = std::min(chunk, B - b0);
    Work w = carve(d, h->gemm_mode, nw, d.C, ws);
    const float* xc = x + (size_t)b0 * d.N * 2;
    if (int rc = run_trunk(h, xc, nw, d.C, w, s)) return rc;
    if (w.route.det == DET_ENV_FIRST) {
      // envelope first (det.hip): PhiC straight from h, then the determinant algebra
      const size_t ne = (size_t)nw * d.N, r6 = (size_t)round_up((int)(6 * ne), 256);
      const size_t r1 = (size_t)round_up((int)ne, 256);
      float* S = w.qkv;
      float* FS = S + align64(r6 * 256);
      float* E2 = FS + align64(r6 * d.ld_orb);
      float* Weff = E2 + align64(r1 * env_first_k(d));
      {
        PROF(PK_GEMM + PK_CH, 2.0 * 6 * ne * d.D * d.orb_cols + 2.0 * ne * env_first_k(d) * 256 * 2 * d.N +
                                  2.0 * ne * d.C * 256 * 2 * d.N,
             4.0 * ne * (7.0 * 256 + 6.0 * d.ld_orb + env_first_k(d) + 2.0 * 256 * 2 * d.N + d.C * 256));
        launch_env_first(d, w.h, w.geo, xc, h->norm, h->p.WorbT, h->p.borb, h->p.WorbP, h->p.W2T, h->p.W2P,
                         w.route.family == GEMM_X6, nw, S, FS, E2, Weff, w.o, s);
      }
      {
        PROF(PK_DET_ENERGY, 0.0, 8.0 * nw * d.C * d.N * d.N);
        launch_det_energy_pc(d, xc, w.geo, h->p.jastrow, h->norm, e_l + 2 * (size_t)b0, obs + 8 * (size_t)b0, nw, s, w.o);
      }
      if (int rc = check_launch()) return rc;
      continue;
    }
    {
      PROF(PK_DET_ENERGY, 0.0, 4.0 * nw * d.N * d.C * d.ld_orb);
      // the trunk's o buffer (rows x D floats) is free here and holds nw K C N N complex when 2 K N <= D
      launch_det_energy(d, w.F, xc, w.geo, h->p.jastrow, h->norm, e_l + 2 * (size_t)b0, obs + 8 * (size_t)b0, nw, s,
                        w.route.det == DET_PRECONTRACT ? w.o : nullptr);
    }
    if (int rc = check_launch()) return rc;
  }
  return DH_OK;
}

int dh_grad_cotangent(const float* diff, const float* nvalid, int B, int part, float* ct, void* stream) {
  if (!diff || !nvalid || !ct || B < 1 || (part != 0 && part != 1)) return fail(DH_EINVAL, "bad arguments");
  launch_cotangent(diff, nvalid, B, part, ct, (hipStream_t)stream);
  return check_launch();
}

int dh_adam_update(float* params, const float* grad, float* mu, float* nu, size_t n, float lr, float b1, float b2,
                   float eps, int step, void* stream) {
  if (!params || !grad || !mu || !nu || n == 0 || step < 0) return fail(DH_EINVAL, "bad arguments");
  launch_adam(params, grad, mu, nu, n, lr, b1, b2, eps, step, (hipStream_t)stream);
  return check_launch();
}

int dh_energy_stats(dh_handle* h, const float* e_l, const float* obs, const int32_t* n_accept, int B, int steps,
                    int penalties, float* out, void* stream) {
  (void)h;  // statistics of any wavefunction's E_L (NULL: a log-psi callable of the caller)
  if (!e_l || !obs || !out) return fail(DH_EINVAL, "null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_energy_stats needs B >= 1");
  launch_stats(e_l, obs, n_accept, B, steps, penalties, out, (hipStream_t)stream);
  return check_launch();
}

int dh_loss_diff(dh_handle* h, const float* e_l, const float* obs, int B, const float* stats, float lz_penalty,
                 float lz_center, float l2_penalty, float* diff, float* nvalid, void* stream) {
  (void)h;  // as dh_energy_stats: h may be NULL
  if (!e_l || !obs || !stats || !diff || !nvalid) return fail(DH_EINVAL, "null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_loss_diff needs B >= 1");
  launch_loss_diff(e_l, obs, B, stats, lz_penalty, lz_center, l2_penalty, diff, nvalid, (hipStream_t)stream);
  return check_launch();
}

int dh_fidelity_partial(const float* logpsi, const float* logphi, int B, double* part, void* stream) {
  if (!logpsi || !logphi || !part) return fail(DH_EINVAL, "dh_fidelity_partial: null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_fidelity_partial needs B >= 1");
  launch_fidelity_partial(logpsi, logphi, B, part, (hipStream_t)stream);
  return check_launch();
}

int dh_fidelity_residual(const float* logpsi, const float* logphi, int B, const double* total, float* resid,
                         void* stream) {
  if (!logpsi || !logphi || !total || !resid) return fail(DH_EINVAL, "dh_fidelity_residual: null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_fidelity_residual needs B >= 1");
  launch_fidelity_residual(logpsi, logphi, B, total, resid, (hipStream_t)stream);
  return check_launch();
}

int dh_ortho_partial(const float* logpsi, const float* logphi, int B, int K, double* part, void* stream) {
  if (!logpsi || !logphi || !part) return fail(DH_EINVAL, "dh_ortho_partial: null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_ortho_partial needs B >= 1");
  if (K < 1 || K > DH_ORTHO_MAX_STATES) return fail(DH_EINVAL, "dh_ortho_partial needs 1 <= K <= DH_ORTHO_MAX_STATES");
  launch_ortho_partial(logpsi, logphi, B, K, part, (hipStream_t)stream);
  return check_launch();
}

int dh_ortho_residual(const float* logpsi, const float* logphi, int B, int K, const double* total,
                      const double* weight, const float* e_l, float* out, void* stream) {
  if (!logpsi || !logphi || !total || !weight || !out) return fail(DH_EINVAL, "dh_ortho_residual: null argument");
  if (B < 1) return fail(DH_EINVAL, "dh_ortho_residual needs B >= 1");
  if (K < 1 || K > DH_ORTHO_MAX_STATES) return fail(DH_EINVAL, "dh_ortho_residual needs 1 <= K <= DH_ORTHO_MAX_STATES");
  launch_ortho_residual(logpsi, logphi, B, K, total, weight, e_l, out, (hipStream_t)stream);
  return check_launch();
}

// Debug hook (tests only): run input + trunk + orbital GEMM for B walkers with
// C = 1 (op 0) or 2N+5 (op 1) channels and leave the results in the workspace:
// final trunk activations at float offset 0 ([rows][D]) and orbital features at
// float offset dh_debug_f_offset ([rows][ld_orb]).  Refused where the route maps no F.
int dh_debug_trunk(dh_handle* h, const float* x, int B, int op, void* ws, size_t ws_bytes, void* stream) {
  const size_t need = h ? dh_workspace_bytes(h, B, op) : 0;
  if (int rc = check_common(h, x, B, ws, ws_bytes, need)) return rc;
  Work w = carve(h->d, h->gemm_mode, B, op == 1 ? h->d.C : 1, ws);
  if (!w.F)
    return fail(DH_EINVAL, "dh_debug_trunk: this config's local energy goes envelope first and maps no orbital "
                           "features F over the channel rows");
  // keep_h: the chain form writes the last layer's h too (the production path skips it)
  if (op != 1 && w.route.det_in_chain) {  // the production launch (log psi into w.logpsi), F kept as well
    const ChainDet det = chain_det(h, x, B, w.logpsi, McmcEpi{});
    return run_trunk(h, x, B, 1, w, (hipStream_t)stream, false, /*keep_h=*/true, &det, /*keep_F=*/true);
  }
  return run_trunk(h, x, B, op == 1 ? h->d.C : 1, w, (hipStream_t)stream, false, /*keep_h=*/true);
}

int dh_debug_env_leaf(const float* thph, int n, int M, int sq, float* out, void* stream) {
  if (!thph || !out || n < 1 || M < 1) return fail(DH_EINVAL, "bad env_leaf probe args");
  launch_env_leaf_probe(thph, n, M, sq, out, (hipStream_t)stream);
  return check_launch();
}

size_t dh_debug_f_offset(const dh_handle* h, int B, int op) {
  if (!h || B < 1) return (size_t)-1;
  Work w = carve(h->d, h->gemm_mode, B, op == 1 ? h->d.C : 1, reinterpret_cast<void*>(size_t(64)));
  if (!w.F) return (size_t)-1;  // no F on this route (dh_debug_trunk refuses it too)
  return (size_t)(w.F - reinterpret_cast<float*>(size_t(64)));
}

// Test hook: one GEMM launch of kernel variant `variant` (the codes of launch_gemm_variant, or
// 100 + a code of launch_gemm_nt_variant; -1 = code 0).  The launchers check
// the code before they touch an argument.
int dh_debug_gemm(int variant, const float* X, int ldx, const float* W, int ldw, const float* bias, const float* R,
                  int ldr, float* Y, int ldy, int rows, int ncols, int K, int C, void* stream) {
  bool known = true;
  if (variant >= 100) {
    if (K % 32 != 0) return fail(DH_EINVAL, "NT GEMM needs K % 32 == 0");
    known = launch_gemm_nt_variant(variant - 100, X, ldx, W, ldw, bias, R, ldr, Y, ldy, rows, ncols, K, C,
                                   (hipStream_t)stream);
  } else {
    known = launch_gemm_variant(variant < 0 ? 0 : variant, X, ldx, W, ldw, bias, R, ldr, Y, ldy, rows, ncols, K, C,
                                (hipStream_t)stream);
  }
  if (!known) return fail(DH_EINVAL, "no GEMM variant " + std::to_string(variant));
  return check_launch();
}

int dh_debug_gemm_x6_choice(int rows, int ncols) { return gemm_x6_choose(rows, ncols); }

int dh_debug_route(const dh_handle* h, int B, int op, int* out, int n) {
  if (!h || h->analytic() || B < 1 || (n > 0 && !out)) return fail(DH_EINVAL, "bad route query");
  const int C = op == 1 ? h->d.C : 1;
  const TrunkRoute r = trunk_route(h->d, h->gemm_mode, C, B * h->d.N * C);
  if (n > 0) std::memcpy(out, &r, sizeof(int) * std::min(n, kTrunkRouteFields));
  return kTrunkRouteFields;
}

int dh_debug_x6_plane_rows(int ncols) { return x6_plane_rows(ncols); }

int dh_debug_split_planes(const float* Wt, int ldw, int ncols, int K, uint16_t* Wp, void* stream) {
  if (!Wt || !Wp || ncols < 1 || K < 1) return fail(DH_EINVAL, "bad split_planes args");
  launch_split_planes(Wt, ldw, ncols, K, Wp, (hipStream_t)stream);
  return check_launch();
}

int dh_debug_gemm_x6(int variant, const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias,
                     const float* R, int ldr, float* Y, int ldy, int rows, int ncols, int K, int C, void* stream) {
  if (!gemm_x6_supported(K) || ldp < x6_plane_rows(ncols)) return fail(DH_EINVAL, "bad gemm_x6 args");
  if (variant >= 10 && K > 256) return fail(DH_EINVAL, "persistent gemm_x6 needs K <= 256");
  if (variant < 0) variant = gemm_x6_choose(rows, ncols);
  if (!launch_gemm_x6_variant(variant, X, ldx, Wp, ldp, bias, R, ldr, Y, ldy, rows, ncols, K, C, (hipStream_t)stream))
    return fail(DH_EINVAL, "no gemm_x6 variant " + std::to_string(variant));
  return check_launch();
}

int dh_debug_gemm_x6_ln(int mode, int nw, const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias,
                        const float* ln, float* h, int rows, int K, void* stream) {
  if (!gemm_x6_supported(K) || K > 256 || ldp < x6_plane_rows(256) || rows < 1 || (mode != 0 && mode != 1))
    return fail(DH_EINVAL, "bad gemm_x6_ln args");
  if (!launch_gemm_x6_ln(X, ldx, Wp, ldp, bias, ln, h, rows, K, mode, nw, (hipStream_t)stream))
    return fail(DH_EINVAL, "no gemm_x6_ln form " + std::to_string(nw));
  return check_launch();
}

int dh_debug_chain_x6(const float* X1, const uint16_t* Wp1, int ldp1, const float* b1, const float* ln1,
                      const uint16_t* Wp2, int ldp2, const float* b2, const float* ln2, const uint16_t* Wp3,
                      int ldp3, const float* b3, int n3, float* Y3, int ldy3, float* h, int rows, void* stream) {
  if (!X1 || !Wp1 || !Wp2 || !b1 || !ln1 || !b2 || !ln2 || !h || rows < 1 || ldp1 < x6_plane_rows(256) ||
      ldp2 < x6_plane_rows(256) || (Wp3 && (!b3 || !Y3 || n3 < 1 || ldy3 < n3 || ldy3 % 4 || ldp3 < x6_plane_rows(n3))))
    return fail(DH_EINVAL, "bad chain_x6 args");
  launch_chain_x6(X1, Wp1, ldp1, b1, ln1, Wp2, ldp2, b2, ln2, Wp3, ldp3, b3, n3, Y3, ldy3, h, rows, X6Feat{},
                  (hipStream_t)stream);
  return check_launch();
}

int dh_debug_gemm_lnch(int N, int mode, const float* X, const uint16_t* Wp, int ldp, const float* bias,
                       const float* ln, const float* geo, float* h, int ne, void* stream) {
  if (!gemm_lnch_supported(N, 256) || (mode != 0 && mode != 1) || (mode == 0 && !X) || !Wp || !ln || !geo || !h ||
      ne < 1 || ldp < x6_plane_rows(256) || ne % N)
    return fail(DH_EINVAL, "bad gemm_lnch args");
  launch_gemm_lnch(N, mode == 0 ? X : h, Wp, ldp, bias, ln, geo, h, ne, mode, (hipStream_t)stream);
  return check_launch();
}

// which fused channel-tail kernel the local energy uses (DH_LNCH at start-up): tests only
int dh_debug_set_lnch_form(int form) { return set_lnch_form(form); }

// whether a log-psi pass runs the value kernel's work in its last chain launch where the route
// allows it (1, the default) or always as a launch of its own (0): tests only
int dh_debug_set_det_in_chain(int on) { return set_det_in_chain(on); }

int dh_debug_det_in_chain(const dh_handle* h, int B, int op) {
  if (!h || h->analytic() || B < 1) return fail(DH_EINVAL, "bad route query");
  const int C = op == 1 ? h->d.C : 1;
  return trunk_route(h->d, h->gemm_mode, C, B * h->d.N * C).det_in_chain;
}

int dh_debug_gemm_ln(int mode, int bm, const float* X, int ldx, const float* Wt, int ldw, const float* bias,
                     const float* ln, float* h, int rows, int K, void* stream) {
  if (!gemm_ln_supported(256, K) || rows < 1 || (mode != 0 && mode != 1)) return fail(DH_EINVAL, "bad gemm_ln args");
  launch_gemm_ln(X, ldx, Wt, ldw, bias, ln, h, rows, K, mode, bm, (hipStream_t)stream);
  return check_launch();
}

int dh_profile_enable(dh_handle* h, int on) {
  if (!h) return fail(DH_EINVAL, "null handle");
  h->prof.on = on != 0;
  h->prof.used = 0;
  return DH_OK;
}

int dh_profile_read(dh_handle* h, double* out, int reset) {
  if (!h || !out) return fail(DH_EINVAL, "null argument");
  for (int i = 0; i < 4 * PK_TOTAL; ++i) out[i] = 0.0;
  for (size_t i = 0; i < h->prof.used; ++i) {
    ProfRec& r = h->prof.recs[i];
    HIP_TRY(hipEventSynchronize(r.b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    out[4 * r.kind + 0] += 1.0;
    out[4 * r.kind + 1] += ms;
    out[4 * r.kind + 2] += r.flops;
    out[4 * r.kind + 3] += r.bytes;
  }
  if (reset) h->prof.used = 0;
  return PK_TOTAL;
}

int dh_potential(dh_handle* h, const float* x, int B, float* pe, void* stream) {
  if (!h || !x || !pe || B < 1) return fail(DH_EINVAL, "bad arguments");
  launch_potential(h->d, x, pe, B, (hipStream_t)stream);
  return check_launch();
}

// ---- log psi supplied by the caller (arbitrary callables, mcmc.py:105 / hamiltonian.py:83) ----

int dh_mh_init(const float* logpsi, float* lp, int32_t* n_accept, int B, void* stream) {
  if (!logpsi || !lp || !n_accept || B < 1) return fail(DH_EINVAL, "bad arguments");
  launch_lp_from_logpsi(logpsi, lp, n_accept, B, (hipStream_t)stream);
  return check_launch();
}

int dh_mh_propose(const float* x, float* x2, int B, int nelec, float width, uint64_t seed, uint64_t step,
                  int64_t walker_offset, const float* noise, void* stream) {
  if (!x || !x2 || B < 1 || nelec < 1 || x == x2) return fail(DH_EINVAL, "bad arguments");
  Dims d{};
  d.N = nelec;
  launch_propose(d, x, x2, B, width, seed, step, walker_offset, noise, 0, (hipStream_t)stream);
  return check_launch();
}

int dh_mh_accept(float* x, const float* x2, float* lp, const float* logpsi2, int32_t* n_accept, int B, int nelec,
                 uint64_t seed, uint64_t step, int64_t walker_offset, const float* noise, void* stream) {
  if (!x || !x2 || !lp || !logpsi2 || !n_accept || B < 1 || nelec < 1) return fail(DH_EINVAL, "bad arguments");
  Dims d{};
  d.N = nelec;
  launch_accept(d, x, x2, lp, logpsi2, n_accept, B, seed, step, walker_offset, noise, 0, (hipStream_t)stream);
  return check_launch();
}

int dh_kinetic_from_derivatives(const double* x, const double* grad, const double* hess, int B, int nelec, double Q,
                                double r, float* ke, float* mom, void* stream) {
  if (!x || !grad || !hess || !ke || !mom || B < 1 || nelec < 1 || !(r > 0.0) || Q < 0.0)
    return fail(DH_EINVAL, "bad arguments");
  if (kinetic_assembly_lds_bytes(nelec) > 64 * 1024) return fail(DH_EINVAL, "nelec > 256");
  launch_kinetic_assembly(x, grad, hess, B, nelec, Q, r, ke, mom, (hipStream_t)stream);
  return check_launch();
}

int dh_init_walkers(dh_handle* h, float* x, int B, uint64_t seed, int64_t walker_offset, void* stream) {
  if (!h || !x || B < 1) return fail(DH_EINVAL, "bad arguments");
  launch_init_walkers(h->d, x, B, seed, walker_offset, (hipStream_t)stream);
  return check_launch();
}

}  // extern "C"
