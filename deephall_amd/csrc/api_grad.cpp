// The parameter-gradient side of the C ABI (include/deephall_amd.h): dh_logpsi_vjp, dh_ntk*, dh_kfac_*,
// dh_minsr_matrix*.  One forward pass with saved activations (vjp_forward), one reverse walk over them
// (reverse_walk) that hands every parameter site to the gradient, the Fisher or the NTK / JVP consumer.
#include <cmath>

#include "api_internal.h"

using namespace dh;

namespace {

// Workspace of one gradient (VJP) pass over nw walkers (floats).
struct GradWork {
  float *geo, *logpsi, *F, *dF, *jg;
  float *hs[17], *qkv[16], *o[16], *t[16], *h1[16], *z[16];  // saved activations per layer
  float *dh, *dA, *dz, *dqkv, *dO;                            // backward temporaries
  float *P, *dWol, *dbol;                                     // chunk partials, folded-weight grads
  float *dWorb, *dborb;                                       // full-layout orbital grads ("sparse")
  float *fgrad, *ctf;                                         // KFAC: Fisher tangent (ref layout), cotangent
  float *kfs0, *kfs1;                                         // KFAC "sparse": featured-orbital rows
  size_t total_bytes;
};

GradWork carve_grad(const Dims& d, int nw, void* base, size_t nref = 0) {
  const int rows = nw * d.N;
  const size_t rp = (size_t)round_up(std::max(rows, 1), kRowPad);
  const size_t D = d.D, nh = align64(rp * D);
  GradWork w{};
  Carver c{reinterpret_cast<float*>(base)};
  w.geo = c.take((size_t)rows * 4);
  w.logpsi = c.take((size_t)nw * 2);
  w.jg = c.take((size_t)nw * 2);
  w.F = c.take(rp * d.ld_orb);
  w.dF = c.take(rp * d.ld_orb);
  for (int l = 0; l <= d.L; ++l) w.hs[l] = c.take(nh);
  for (int l = 0; l < d.L; ++l) {
    w.qkv[l] = c.take(3 * nh);
    w.o[l] = c.take(nh);
    w.t[l] = c.take(nh);
    w.h1[l] = c.take(nh);
    w.z[l] = c.take(nh);
  }
  w.dh = c.take(nh);
  w.dA = c.take(nh);
  w.dz = c.take(nh);
  w.dqkv = c.take(3 * nh);
  w.dO = c.take(nh);
  const size_t nch = (size_t)grad_chunks(rows);
  const size_t MNK = (size_t)d.M * d.N * d.K;
  // (KFAC: the orbital output Gram matrices need MNK^2 per chunk)
  // ("sparse" KFAC: the featured-orbital tangent Gram (8 N K)^2, the lll_weight factors over
  //  N K times as many rows: 64 and M^2 per chunk of those)
  const size_t F8 = (size_t)8 * d.N * d.K, pls = (nref && d.sparse) ? std::max(F8 * F8, (size_t)d.N * d.K *
                                                                       std::max<size_t>(64, (size_t)d.M * d.M)) : 0;
  const size_t pw = std::max({D * 3 * D, D * (size_t)d.ld_orb, (size_t)4 * D, nref ? MNK * MNK : (size_t)0, pls});
  const size_t pc = std::max((size_t)3 * D, (size_t)d.ld_orb);
  w.P = c.take(std::max({nch * pw, nch * pc, (size_t)ln_bwd_blocks(rows) * 2 * D, (size_t)nw * 2}));
  w.dWol = c.take(D * D);
  w.dbol = c.take(D);
  if (d.sparse) {
    w.dWorb = c.take(D * d.ld_orb);
    w.dborb = c.take(d.ld_orb);
  }
  if (nref) {
    w.fgrad = c.take(nref);
    w.ctf = c.take((size_t)nw * 2);
    if (d.sparse) {
      w.kfs0 = c.take(rp * 8 * d.N * d.K);
      w.kfs1 = c.take(rp * 8 * d.N * d.K);
    }
  }
  w.total_bytes = c.bytes();
  return w;
}

// Workspace of dh_ntk over nw walkers: the VJP's (one chunk), then the masked cotangents, one LayerNorm's
// per-walker scale | bias tangents [nw][2 D], and one dense map's centred input rows [rows][D], their
// offsets [rows] and mean row [D].  dh_ntk_jvp (jvp) adds one dense map's slice of the direction, packed
// [K_in + 1 bias row][K_out] and sized to the largest map, its per-column constant and the column
// blocks' partial sums [blocks][nw].
struct NtkWork {
  GradWork g;
  float *ctm, *lnp, *xc, *arow, *mean;
  float *vpk, *cvec, *jpart;  // dh_ntk_jvp only
  size_t total_bytes;
};

NtkWork carve_ntk(const Dims& d, int nw, void* base, bool jvp = false) {
  NtkWork w{};
  w.g = carve_grad(d, nw, base);
  Carver c{reinterpret_cast<float*>(base), w.g.total_bytes / sizeof(float)};
  w.ctm = c.take((size_t)nw * 2);
  w.lnp = c.take((size_t)nw * 2 * d.D);
  w.xc = c.take((size_t)nw * d.N * std::max(d.D, 4));
  w.arow = c.take((size_t)nw * d.N);
  w.mean = c.take((size_t)std::max(d.D, 4));
  if (jvp) {
    const size_t kout = std::max((size_t)3 * d.D, (size_t)d.ld_orb);
    w.vpk = c.take(((size_t)d.D + 1) * kout);
    w.cvec = c.take(kout);
    w.jpart = c.take((size_t)ntk_jvp_col_blocks((int)kout) * nw);
  }
  w.total_bytes = c.bytes();
  return w;
}

// forward with saved activations (the same arithmetic as the log-psi pass)
void vjp_forward(dh_handle* h, const float* x, int nw, float* logpsi, const GradWork& w, hipStream_t s) {
  const Dims& d = h->d;
  const Params& P = h->p;
  const int rows = nw * d.N, D = d.D;
  const int family = gemm_family(d, /*want_x6=*/true);  // whatever the handle's GEMM mode
  auto fwd = [&](const float* X, const float* W, const float* Wt, const uint16_t* Wp, int ncols, const float* bias,
                 const float* Rr, float* Y, int ldy) {
    dense_gemm(family, X, D, W, Wt, Wp, ldy, bias, Rr, Rr ? ncols : 0, Y, ldy, rows, ncols, D, 1, s);
  };
  launch_input(d, x, P.W0, nullptr, nullptr, w.hs[0], nullptr, w.geo, nw, 1, s);
  for (int l = 0; l < d.L; ++l) {
    const LayerParams& lp = P.layer[l];
    fwd(w.hs[l], lp.Wqkv, lp.WqkvT, lp.WqkvP, 3 * D, lp.bqkv, nullptr, w.qkv[l], 3 * D);
    launch_attention(d, w.qkv[l], w.geo, w.o[l], nw, 1, s);
    fwd(w.o[l], lp.Wol, lp.WolT, lp.WolP, D, lp.bol, w.hs[l], w.t[l], D);
    launch_ln_fwd(w.t[l], nullptr, lp.ln1, w.h1[l], rows, D, s);
    fwd(w.h1[l], lp.Wm, lp.WmT, lp.WmP, D, lp.bm, nullptr, w.z[l], D);
    launch_ln_fwd(w.h1[l], w.z[l], lp.ln2, w.hs[l + 1], rows, D, s);
  }
  fwd(w.hs[d.L], P.Worb, P.WorbT, P.WorbP, d.orb_cols, P.borb, nullptr, w.F, d.ld_orb);
  launch_det_value(d, w.F, x, P.jastrow, h->norm, logpsi ? logpsi : w.logpsi, nw, s);
}

// ---- the reverse pass: one walk (reverse_walk, below) and the three consumers of its parameter sites.
// What they share: one chunk of nw walkers on stream s
struct Rev {
  dh_handle* h;
  const GradWork& w;
  int nw;
  hipStream_t s;
  const Dims& d = h->d;
  const int rows = nw * d.N, D = d.D, nch = grad_chunks(rows);
  const RefSeg RS{d.L, d.NB, d.sparse};
  const float* ref(int seg) const { return h->ref + h->ref_offsets[seg]; }
};

// Gradient consumer: the parameter gradient, written (acc = 0) or accumulated (acc = 1) into `grad` (dh_ref_layout)
struct GradSites : Rev {
  float* grad;
  int acc;
  int ln_rows() const { return kLnRowsPerBlock; }
  float* ln_partials() const { return w.P; }
  float* g(int seg) const { return grad + h->ref_offsets[seg]; }
  // weight gradient: out[:, c0:c0+nc] (ldo) (+)= X^T dY[:, c0:c0+nc] over this chunk's rows
  void wgrad(const float* X, const float* dY, int n) const { launch_tn_partial(X, D, dY, n, rows, D, n, w.P, s); }
  void wout(int n, int c0, int nc, float* out, int ldo) const {
    launch_reduce2d(w.P + c0, nch, (size_t)D * n, n, D, nc, out, ldo, 1.f, acc, s);
  }
  void bgrad(const float* dY, int n, int c0, int nc, float* out) const {
    launch_colsum_partial(dY, n, rows, n, w.P, s);
    launch_reduce2d(w.P + c0, nch, (size_t)n, n, 1, nc, out, nc, 1.f, acc, s);
  }
  void jastrow() const {
    launch_reduce2d(w.jg, nw, 2, 2, 1, 1, g(RS.jas(0)), 1, 1.f, acc, s);
    launch_reduce2d(w.jg + 1, nw, 2, 2, 1, 1, g(RS.jas(1)), 1, 1.f, acc, s);
  }
  void orbital() const {
    const int MNK = d.M * d.N * d.K;
    wgrad(w.hs[d.L], w.dF, d.ld_orb);
    if (!d.sparse) {
      for (int i = 0; i < 2 * d.NB; ++i) wout(d.ld_orb, i * MNK, MNK, g(RS.orb_kernel(i)), MNK);
      launch_colsum_partial(w.dF, d.ld_orb, rows, d.ld_orb, w.P, s);
      for (int i = 0; i < 2 * d.NB; ++i)
        launch_reduce2d(w.P + i * MNK, nch, (size_t)d.ld_orb, d.ld_orb, 1, MNK, g(RS.orb_bias(i)), MNK, 1.f, acc, s);
    } else {
      // full-layout gradients of this chunk, then through the lll_weight fold
      launch_reduce2d(w.P, nch, (size_t)D * d.ld_orb, d.ld_orb, D, d.orb_cols, w.dWorb, d.ld_orb, 1.f, 0, s);
      launch_colsum_partial(w.dF, d.ld_orb, rows, d.ld_orb, w.P, s);
      launch_reduce2d(w.P, nch, (size_t)d.ld_orb, d.ld_orb, 1, d.orb_cols, w.dborb, d.ld_orb, 1.f, 0, s);
      SparseBlocks sb{};
      sb.n = 2 * d.NB;
      for (int i = 0; i < sb.n; ++i) {
        sb.W8[i] = ref(RS.orb_kernel(i));
        sb.b8[i] = ref(RS.orb_bias(i));
        launch_sparse_unfold(w.dWorb + i * MNK, d.ld_orb, w.dborb + i * MNK, ref(RS.lll(0)), D, d.N * d.K, d.M,
                             g(RS.orb_kernel(i)), g(RS.orb_bias(i)), acc, s);
      }
      launch_sparse_lll_grad(sb, w.dWorb, d.ld_orb, w.dborb, D, d.N * d.K, d.M, g(RS.lll(0)), g(RS.lll(1)), acc, s);
    }
  }
  void layernorm(int l, int scale) const {  // scale: Rln2s or Rln1s, its bias the next segment
    const int nb = ln_bwd_blocks(rows);
    launch_reduce2d(w.P, nb, (size_t)2 * D, D, 1, D, g(RS.lay(l, scale)), D, 1.f, acc, s);
    launch_reduce2d(w.P + D, nb, (size_t)2 * D, D, 1, D, g(RS.lay(l, scale + 1)), D, 1.f, acc, s);
  }
  void mlp(int l) const {  // z = h1 Wm + bm
    wgrad(w.h1[l], w.dz, D);
    wout(D, 0, D, g(RS.lay(l, RWm)), D);
    bgrad(w.dz, D, 0, D, g(RS.lay(l, Rbm)));
  }
  void attn_out(int l) const {  // t = h + o Wol + bol: folded-weight gradients, then unfolded onto Wo, bo, Wl
    wgrad(w.o[l], w.dA, D);
    launch_reduce2d(w.P, nch, (size_t)D * D, D, D, D, w.dWol, D, 1.f, 0, s);
    launch_colsum_partial(w.dA, D, rows, D, w.P, s);
    launch_reduce2d(w.P, nch, (size_t)D, D, 1, D, w.dbol, D, 1.f, 0, s);
    //   Wol = Wo Wl, bol = bo Wl:  dWo = dWol Wl^T, dbo = dbol Wl^T, dWl = Wo^T dWol + bo^T dbol
    launch_small_gemm(D, D, D, w.dWol, D, 0, ref(RS.lay(l, RWl)), D, 1, g(RS.lay(l, RWo)), D, acc, s);
    launch_small_gemm(1, D, D, w.dbol, D, 0, ref(RS.lay(l, RWl)), D, 1, g(RS.lay(l, Rbo)), D, acc, s);
    launch_small_gemm(D, D, D, ref(RS.lay(l, RWo)), D, 1, w.dWol, D, 0, g(RS.lay(l, RWl)), D, acc, s);
    launch_small_gemm(D, D, 1, ref(RS.lay(l, Rbo)), 1, 0, w.dbol, D, 0, g(RS.lay(l, RWl)), D, 1, s);
  }
  void qkv(int l) const {  // qkv = h Wqkv + bqkv
    wgrad(w.hs[l], w.dqkv, 3 * D);
    for (int part = 0; part < 3; ++part) wout(3 * D, part * D, D, g(RS.lay(l, RWq + 2 * part)), D);
    launch_colsum_partial(w.dqkv, 3 * D, rows, 3 * D, w.P, s);
    for (int part = 0; part < 3; ++part)
      launch_reduce2d(w.P + part * D, nch, (size_t)3 * D, 3 * D, 1, D, g(RS.lay(l, Rbq + 2 * part)), D, 1.f, acc, s);
  }
  void input() const {  // h_0 = features W0
    launch_w0_partial(d, w.geo, w.dh, D, rows, w.P, s);
    launch_reduce2d(w.P, nch, (size_t)4 * D, D, 4, D, g(RS.W0()), D, 1.f, acc, s);
  }
};

// KFAC statistics of one dh_kfac_vjp call: factor Gram matrices into `stats` (KfacHost slots), per total row
struct KfacAcc {
  const KfacHost* plan;
  float* stats;
  float inv_rows;         // 1 / (B N)
  float inv_rows_blk[2];  // 1 / (B N_alpha) (orbital blocks)
};

// Fisher consumer: no dense weight gradient; every dense layer's input / output-tangent Gram
// matrices go into kf.stats.  The Jastrow and LayerNorm sites are the gradient consumer's: KFAC's
// generic tangents, the only entries of `grad` (fgrad) this mode writes besides the lll bias.
struct FisherSites : GradSites {
  const KfacAcc& kf;
  // slot (+)= scale X^T X (n columns of X, row stride ldx, `nr` rows), with the bias row / column / corner
  // of [X, 1] when aug (accum: add to the slot instead of overwriting it; default acc, the chunk loop's flag)
  void gram(const float* X, int ldx, int n, int slot, float scale, int nr, bool aug, int accum = -1) const {
    const KfacSlot& sl = kf.plan->slots[slot];
    float* out = kf.stats + sl.off;
    const int nc2 = grad_chunks(nr);
    const int a = accum < 0 ? acc : accum;
    launch_tn_partial(X, ldx, X, ldx, nr, n, n, w.P, s);
    launch_reduce2d(w.P, nc2, (size_t)n * n, n, n, n, out, sl.n, scale, a, s);
    if (aug) {
      launch_colsum_partial(X, ldx, nr, n, w.P, s);
      launch_kfac_aug(w.P, nc2, n, out, sl.n, scale, (float)nr * scale, a, s);
    }
  }
  void orbital() const {
    const KfacHost& K = *kf.plan;
    const int MNK = d.M * d.N * d.K, NK = d.N * d.K, F8 = 8 * NK;
    const float inv_lll = kf.inv_rows / (float)NK;  // rows of the lll block: B N N K
    int lo = 0;
    for (int a = 0, blk = 0; a < 2; ++a) {
      const int na = a == 0 ? d.n_up : d.n_dn;
      if (na == 0) continue;
      const int nr = d.NB == 1 ? rows : nw * na;
      if (!d.sparse)
        for (int part = 0; part < 2; ++part)
          gram(w.dF + (size_t)(blk * 2 + part) * MNK, d.ld_orb, MNK, K.G_orb[blk][part], kf.inv_rows_blk[blk], rows,
               false);
      const float* hb = w.hs[d.L];
      if (d.NB > 1) {  // this spin block's rows of every walker, gathered
        launch_copy2d(w.hs[d.L] + (size_t)lo * D, d.N * D, w.dqkv, na * D, nw, na * D, s);
        hb = w.dqkv;
      }
      gram(hb, D, D, K.A_orb[blk], kf.inv_rows_blk[blk], nr, true);
      if (d.sparse) {
        const int nlo = d.NB == 1 ? 0 : lo, nna = d.NB == 1 ? d.N : na;
        // featured-orbital tangents (lll dF) -> the DenseGeneral G factors
        for (int part = 0; part < 2; ++part) {
          launch_kfac_sparse_dphi(w.dF, d.ld_orb, ref(RS.lll(0)), d.M, NK, blk * 2 + part, nr, nna, d.N, nlo, w.kfs0,
                                  s);
          gram(w.kfs0, F8, F8, K.G_orb[blk][part], kf.inv_rows_blk[blk], nr, false);
        }
        // the lll_weight input (the real featured orbitals h W + b, exact f32) in rows of 8,
        // its output tangent (the real feature segment) in rows of M; spin blocks accumulate
        const int acc_lll = (acc || blk > 0) ? 1 : 0;
        launch_gemm(hb, D, ref(RS.orb_kernel(2 * blk)), F8, ref(RS.orb_bias(2 * blk)), nullptr, 0, w.kfs1, F8, nr, F8,
                    D, 1, s);
        gram(w.kfs1, 8, 8, K.A_lll, inv_lll, nr * NK, false, acc_lll);
        launch_kfac_sparse_regroup(w.dF, d.ld_orb, d.M, NK, blk * 2, nr, nna, d.N, nlo, w.F, s);  // w.F: scratch
        gram(w.F, d.M, d.M, K.G_lll, inv_lll, nr * NK, false, acc_lll);
        // the generic lll bias tangent: sum over rows of the real feature segment
        launch_colsum_partial(w.F, d.M, nr * NK, d.M, w.P, s);
        launch_reduce2d(w.P, grad_chunks(nr * NK), (size_t)d.M, d.M, 1, d.M, g(RS.lll(1)), d.M, 1.f, acc || blk > 0, s);
      }
      lo += na;
      ++blk;
    }
  }
  void mlp(int l) const {
    gram(w.dz, D, D, kf.plan->lay[l].G_z, kf.inv_rows, rows, false);
    gram(w.h1[l], D, D, kf.plan->lay[l].A_h1, kf.inv_rows, rows, true);
  }
  void attn_out(int l) const {  // Dense_{2l+1}'s output tangent is dT; the attention output's input is o
    gram(w.dA, D, D, kf.plan->lay[l].G_T, kf.inv_rows, rows, false);
    gram(w.o[l], D, D, kf.plan->lay[l].A_o, kf.inv_rows, rows, true);
  }
  void qkv(int l) const {
    const KfacLayerSlots& ls = kf.plan->lay[l];
    const int gs[3] = {ls.G_q, ls.G_k, ls.G_v};
    for (int part = 0; part < 3; ++part) gram(w.dqkv + part * D, 3 * D, D, gs[part], kf.inv_rows, rows, false);
    gram(w.hs[l], D, D, ls.A_h, kf.inv_rows, rows, true);
  }
  void input() const {
    gram(w.dh, D, D, kf.plan->s_h0, kf.inv_rows, rows, false);
    const KfacSlot& sl = kf.plan->slots[kf.plan->s_feat];
    launch_kfac_feat_gram(d, w.geo, rows, w.P, s);
    launch_reduce2d(w.P, nch, 16, 4, 4, 4, kf.stats + sl.off, 4, kf.inv_rows, acc, s);
  }
};

// NTK / JVP consumer (ntk.hip): no weight gradient formed.  At every dense map of the REFERENCE
// tree (not the folded kernel layout) the saved input rows and the output tangents go to launch_ntk_gram,
// which adds the map's <dW_b, dW_b'> (+ <db_b, db_b'>) to T [nw][nw]; the LayerNorm and Jastrow parameters
// add J J^T of their explicit per-walker tangents.  T must be zero at entry; the upper triangle of tile pairs
// is accumulated, of the rows that part `part` of `nparts` owns (ntk.hip "Sharding"); the caller mirrors it.
// With a direction v (flat, dh_ref_layout) the same sites add <g_b, v> into jv [nw] (zero at entry), for every
// walker whatever the part: next to each map's Gram launch, launch_ntk_jvp on the same centred rows and
// tangents against the map's slice of v (as it lies, or packed into nt.vpk where the map's columns come from
// several leaves); launch_ntk_rowdot for the explicit rows.
struct NtkSites : Rev {
  const NtkWork& nt;
  float* T;  // null: no Gram launches
  int part, nparts;
  const float* v;  // null: no JVP launches
  float* jv;
  const int N = d.N, tw_own = ntk_tile_walkers(N);
  float* const vpb = v ? nt.vpk + (size_t)D * std::max(3 * D, d.ld_orb) : nullptr;  // the packed maps' bias row
  int ln_rows() const { return N; }  // per-walker scale | bias tangents
  float* ln_partials() const { return nt.lnp; }
  const float* vs(int seg) const { return v ? v + h->ref_offsets[seg] : nullptr; }
  // one dense map: input rows X [rows][kx] (augmented with a 1 when the map has a bias), tangents dY [rows][ky]
  // (kx <= D; the rows are centred on their batch mean first, ntk.hip "Precision")
  // (V [kx][ky] with row stride ldv, vb [ky] or null: the direction's slices for the map)
  void gram(const float* X, int ldx, int kx, const float* dY, int ldy, int ky, bool bias, const float* V, int ldv,
            const float* vb) const {
    launch_colsum_partial(X, ldx, rows, kx, w.P, s);
    launch_reduce2d(w.P, grad_chunks(rows), (size_t)kx, kx, 1, kx, nt.mean, kx, 1.f / (float)rows, 0, s);
    launch_ntk_centre(X, ldx, kx, nt.mean, bias, rows, nt.xc, nt.arow, s);
    if (T) launch_ntk_gram(nt.xc, kx, kx, dY, ldy, ky, nt.arow, N, nw, tw_own, part, nparts, T, s);
    if (v) {
#ifdef DH_NTK_JVP_RAW  // A/B builds only (FILE=api_grad.cpp tools/build_variant.sh): the raw rows, DESIGN.md §3g
      launch_ntk_jvp_cvec(nullptr, kx, V, ldv, vb, ky, nt.cvec, s);
      launch_ntk_jvp(X, ldx, kx, V, ldv, nt.cvec, dY, ldy, ky, N, nw, nt.jpart, jv, s);
#else
      // (x V + v_b) . dy = (u V + (m V + v_b)) . dy
      launch_ntk_jvp_cvec(nt.mean, kx, V, ldv, vb, ky, nt.cvec, s);
      launch_ntk_jvp(nt.xc, kx, kx, V, ldv, nt.cvec, dY, ldy, ky, N, nw, nt.jpart, jv, s);
#endif
    }
  }
  // explicit per-walker tangents J [nw][ka + kb]: T += J J^T; sega, segb: their two leaves of v
  void gram_rows(const float* J, int ka, int sega, int kb, int segb) const {
    if (T) launch_ntk_gram(J, ka + kb, ka + kb, nullptr, 0, 0, nullptr, 1, nw, tw_own, part, nparts, T, s);
    if (v) launch_ntk_rowdot(J, ka + kb, v + h->ref_offsets[sega], ka, v + h->ref_offsets[segb], kb, nw, jv, s);
  }
  void jastrow() const { gram_rows(w.jg, 1, RS.jas(0), 1, RS.jas(1)); }
  // the orbital DenseGenerals: a row's dF is zero in the other spin block's columns, so the
  // blocks' Gram products add up to the one over all orb_cols
  // (columns rounded up to 4 for the kernel's float4 loads: det_bwd writes the padding 0)
  void orbital() const {
    if (v) {  // kernels | biases at columns i MNK of ld_orb, the padding 0 (as pack_from_ref)
      const int MNK = d.M * d.N * d.K;
      launch_copy2d(nullptr, 0, nt.vpk, d.ld_orb, D, d.ld_orb, s);
      launch_copy2d(nullptr, 0, vpb, d.ld_orb, 1, d.ld_orb, s);
      for (int i = 0; i < 2 * d.NB; ++i) {
        launch_copy2d(vs(RS.orb_kernel(i)), MNK, nt.vpk + i * MNK, d.ld_orb, D, MNK, s);
        launch_copy2d(vs(RS.orb_bias(i)), MNK, vpb + i * MNK, d.ld_orb, 1, MNK, s);
      }
    }
    gram(w.hs[d.L], D, D, w.dF, d.ld_orb, round_up(d.orb_cols, 4), true, nt.vpk, d.ld_orb, vpb);
  }
  void layernorm(int l, int scale) const { gram_rows(nt.lnp, D, RS.lay(l, scale), D, RS.lay(l, scale + 1)); }
  void mlp(int l) const { gram(w.h1[l], D, D, w.dz, D, D, true, vs(RS.lay(l, RWm)), D, vs(RS.lay(l, Rbm))); }
  // t = h + (o Wo + bo) Wl, the kernels' folded map taken apart again
  void attn_out(int l) const {
    //   Wo, bo: input [o, 1], output tangent dT Wl^T
    launch_transpose(ref(RS.lay(l, RWl)), D, D, D, w.dWol, D, s);
    launch_gemm(w.dA, D, w.dWol, D, nullptr, nullptr, 0, w.dO, D, rows, D, D, 1, s);
    gram(w.o[l], D, D, w.dO, D, D, true, vs(RS.lay(l, RWo)), D, vs(RS.lay(l, Rbo)));
    //   Wl (no bias): input o Wo + bo, output tangent dT
    launch_gemm(w.o[l], D, ref(RS.lay(l, RWo)), D, ref(RS.lay(l, Rbo)), nullptr, 0, w.dO, D, rows, D, D, 1, s);
    gram(w.dO, D, D, w.dA, D, D, false, vs(RS.lay(l, RWl)), D, nullptr);
  }
  void qkv(int l) const {
    if (v)  // Wq | Wk | Wv side by side, their biases below (as pack_from_ref)
      for (int p3 = 0; p3 < 3; ++p3) {
        launch_copy2d(vs(RS.lay(l, RWq + 2 * p3)), D, nt.vpk + p3 * D, 3 * D, D, D, s);
        launch_copy2d(vs(RS.lay(l, Rbq + 2 * p3)), D, vpb + p3 * D, 3 * D, 1, D, s);
      }
    gram(w.hs[l], D, D, w.dqkv, 3 * D, 3 * D, true, nt.vpk, 3 * D, vpb);  // Wq | Wk | Wv and their biases
  }
  void input() const {  // h_0 = features W0 (no bias)
    launch_ntk_features(d, w.geo, rows, w.dO, s);
    gram(w.dO, 4, 4, w.dh, D, D, false, vs(RS.W0()), D, nullptr);
  }
};

// The reverse pass over the saved activations of vjp_forward for the per-walker cotangents ct
// [nw][2]: the chain-rule launches, issued once, in one order, for every consumer.  At each
// parameter site the walk calls the consumer `c`, which reads the site's saved input and tangent.
// GradWork buffers along the walk (geo, hs, qkv, o, t, h1, z: saved, read-only; dWol, dbol, dWorb, dborb, kfs0,
// kfs1, P: the consumers' own, but the walk's LayerNorm backward writes P for the gradient and Fisher consumers):
//   site       input   tangent  still live  also free for the consumer
//   jastrow    -       jg       dF
//   orbital    hs[L]   dF       -           dqkv, dO, dh; F only for the LAST pass over this chunk's
//              forward: the Fisher consumer's "sparse" site regroups tangents into F, so dh_kfac_vjp
//              must run a chunk's gradient pass before its Fisher pass (the next forward rewrites F)
//   layernorm  -       the partials, one per c.ln_rows() rows in c.ln_partials(), just written
//   mlp        h1[l]   dz       dA          dqkv, dO
//   attn_out   o[l]    dA       -           dO (the Wol backward GEMM writes it next), dqkv, dz
//   qkv        hs[l]   dqkv     dA          dO, dz
//   input      geo     dh       -           every other tangent buffer
template <class Sites>
int reverse_walk(const Sites& c, const float* x, const float* ct) {
  const Dims& d = c.d;
  const Params& P = c.h->p;
  const GradWork& w = c.w;
  const int rows = c.rows, D = c.D, nw = c.nw;
  hipStream_t s = c.s;
  const bool x6 = d.D % 32 == 0 && gemm_x6_supported(D);
  // backward GEMM dX = dY W^T (+ R) with W [D][n]
  auto bwd = [&](const float* dY, int n, const uint16_t* WB, const float* WBT, const float* Rr, float* dX) {
    if (x6)
      launch_gemm_x6(dY, n, WB, x6_plane_rows(D), nullptr, Rr, D, dX, D, rows, D, n, 1, s);
    else
      launch_gemm(dY, n, WBT, D, nullptr, Rr, D, dX, D, rows, D, n, 1, s);
  };
  launch_det_bwd(d, w.F, x, P.jastrow, c.h->norm, ct, w.dF, w.jg, nw, s);
  c.jastrow();
  c.orbital();
  bwd(w.dF, d.ld_orb, P.WorbB, P.WorbBT, nullptr, w.dh);
  for (int l = d.L - 1; l >= 0; --l) {
    const LayerParams& lp = P.layer[l];
    // h_{l+1} = LN2(h1 + tanh z): dU -> dA (the residual path into h1), dz
    launch_ln_bwd_rows(w.h1[l], w.z[l], lp.ln2, w.dh, nullptr, w.dA, w.dz, c.ln_partials(), rows, D, c.ln_rows(), s);
    c.layernorm(l, Rln2s);
    c.mlp(l);
    bwd(w.dz, D, lp.WmB, lp.WmBT, w.dA, w.dh);  // dh1 = dU + dz Wm^T
    // h1 = LN1(t): dT -> dA
    launch_ln_bwd_rows(w.t[l], nullptr, lp.ln1, w.dh, nullptr, w.dA, nullptr, c.ln_partials(), rows, D, c.ln_rows(), s);
    c.layernorm(l, Rln1s);
    c.attn_out(l);
    bwd(w.dA, D, lp.WolB, lp.WolBT, nullptr, w.dO);  // dO = dT Wol^T
    launch_attn_bwd(d, w.qkv[l], w.dO, w.dqkv, nw, s);
    c.qkv(l);
    bwd(w.dqkv, 3 * D, lp.WqkvB, lp.WqkvBT, w.dA, w.dh);  // dh_l = dT + dqkv Wqkv^T
  }
  c.input();
  return check_launch();
}

// ---- KFAC (optimizers/kfac.py:195-241; oracle/kfac.py)

// Build the factor slots, dense blocks, generic segments and device job tables.
int kfac_plan(dh_handle* h) {
  if (h->kfac) return DH_OK;
  const Dims& d = h->d;
  if (d.L > 16) return fail(DH_EINVAL, "KFAC: too many layers");
  auto* K = new KfacHost();
  const int D = d.D, N = d.N, MNK = d.M * d.N * d.K;
  auto slot = [&](int n) {
    K->slots.push_back(KfacSlot{n, K->nmat});
    K->nmat += align64((size_t)n * n);
    return (int)K->slots.size() - 1;
  };
  const RefSeg RS{d.L, d.NB, d.sparse};
  auto blk = [&](int kseg, int bseg, int din, int dout, int a, int g, float scale) {
    K->blocks.push_back(KfacHost::Blk{kseg, bseg, din, dout, a, g, scale});
  };
  K->s_feat = slot(4);
  K->s_h0 = slot(D);
  blk(RS.W0(), -1, 4, D, K->s_feat, K->s_h0, (float)N);
  for (int l = 0; l < d.L; ++l) {
    KfacLayerSlots& L = K->lay[l];
    L.A_h = slot(D + 1);
    L.G_q = slot(D);
    L.G_k = slot(D);
    L.G_v = slot(D);
    L.A_o = slot(D + 1);
    L.G_out = slot(D);
    L.A_Wl = slot(D);
    L.G_T = slot(D);
    L.A_h1 = slot(D + 1);
    L.G_z = slot(D);
    blk(RS.lay(l, RWq), RS.lay(l, Rbq), D, D, L.A_h, L.G_q, (float)N);
    blk(RS.lay(l, RWk), RS.lay(l, Rbk), D, D, L.A_h, L.G_k, (float)N);
    blk(RS.lay(l, RWv), RS.lay(l, Rbv), D, D, L.A_h, L.G_v, (float)N);
    blk(RS.lay(l, RWo), RS.lay(l, Rbo), D, D, L.A_o, L.G_out, (float)(N * d.H));  // x [B, N, H, dh]
    blk(RS.lay(l, RWl), -1, D, D, L.A_Wl, L.G_T, (float)N);
    blk(RS.lay(l, RWm), RS.lay(l, Rbm), D, D, L.A_h1, L.G_z, (float)N);
  }
  // featured orbitals: M N K outputs, or 8 N K for "sparse" (then mixed by lll_weight)
  const int FNK = d.sparse ? 8 * N * d.K : MNK;
  for (int a = 0, b = 0; a < 2; ++a) {
    const int na = a == 0 ? d.n_up : d.n_dn;
    if (na == 0) continue;
    K->A_orb[b] = slot(D + 1);
    for (int part = 0; part < 2; ++part) {
      K->G_orb[b][part] = slot(FNK);
      blk(RS.orb_kernel(2 * b + part), RS.orb_bias(2 * b + part), D, FNK, K->A_orb[b], K->G_orb[b][part], (float)na);
    }
    ++b;
  }
  if (d.sparse) {
    // lll_weight: kfac.py's repeated_dense_complex_no_bias block, its statistics as
    // RepeatedDenseBlock computes them (inputs regrouped into rows of 8, scale 8 N^2)
    K->A_lll = slot(8);
    K->G_lll = slot(d.M);
    blk(RS.lll(0), -1, 8, d.M, K->A_lll, K->G_lll, (float)(8 * N * N));
  }
  // generic (diagonal) parameters: LayerNorm scale / bias, Jastrow alphas
  KfacGenTable& G = K->dev.gen;
  G = KfacGenTable{};
  auto gen = [&](int seg, int n) {
    G.ref[G.n] = h->ref_offsets[seg];
    G.cmp[G.n] = G.total;
    G.total += n;
    ++G.n;
  };
  for (int l = 0; l < d.L; ++l)
    for (int k : {Rln1s, Rln1b, Rln2s, Rln2b}) gen(RS.lay(l, k), D);
  if (d.sparse) gen(RS.lll(1), d.M);  // lll_weight's bias: no pattern covers it
  gen(RS.jas(0), 1);
  gen(RS.jas(1), 1);
  K->nstats = K->nmat + (size_t)G.total;
  // inverse jobs (2 per block: A side, G side), then V / T / P V per block, all in one f64 buffer
  size_t off = 0;
  int nmax = 0, max_v = 0, max_m = 0, max_n = 0;
  for (const auto& b : K->blocks) {
    for (int side = 0; side < 2; ++side) {
      KfacInvJob j{};
      j.slot = side == 0 ? b.a : b.g;
      j.partner = side == 0 ? b.g : b.a;
      j.is_a = side == 0;
      j.n = K->slots[j.slot].n;
      j.sqrt_scale = std::sqrt(b.scale);
      j.gj_off = off;
      off += (size_t)j.n * j.n;
      nmax = std::max(nmax, j.n);
      K->inv.push_back(j);
    }
  }
  for (size_t i = 0; i < K->blocks.size(); ++i) {
    const auto& b = K->blocks[i];
    const int dA = b.din + (b.bseg >= 0 ? 1 : 0);
    KfacBlockJob j{};
    j.kernel_off = h->ref_offsets[b.kseg];
    j.bias_off = b.bseg >= 0 ? (long long)h->ref_offsets[b.bseg] : -1;
    j.din = b.din;
    j.dout = b.dout;
    const size_t nv = (size_t)dA * b.dout;
    j.v_off = off;
    j.t_off = off + nv;
    j.pv_off = off + 2 * nv;
    off += 3 * nv;
    K->bjobs.push_back(j);
    K->g1.push_back(KfacGemmJob{K->inv[2 * i].gj_off, j.v_off, j.t_off, dA, b.dout, dA});
    K->g2.push_back(KfacGemmJob{j.t_off, K->inv[2 * i + 1].gj_off, j.pv_off, dA, b.dout, b.dout});
    max_v = std::max(max_v, (int)nv);
    max_m = std::max(max_m, dA);
    max_n = std::max(max_n, b.dout);
  }
  K->kbuf_doubles = off;
  K->dev.nslots = (int)K->slots.size();
  K->dev.njobs = (int)K->inv.size();
  K->dev.nblocks = (int)K->blocks.size();
  K->dev.nmax = nmax;
  K->dev.max_v = max_v;
  K->dev.max_m = max_m;
  K->dev.max_n = max_n;
  h->kfac = K;
  return DH_OK;
}

// Upload the job tables (once, at the first device call).
int kfac_device(dh_handle* h) {
  if (int rc = kfac_plan(h)) return rc;
  KfacHost* K = h->kfac;
  if (K->dev_mem) return DH_OK;
  // device tables
  const size_t b1 = K->slots.size() * sizeof(KfacSlot), b2 = K->inv.size() * sizeof(KfacInvJob),
               b3 = K->bjobs.size() * sizeof(KfacBlockJob), b4 = K->g1.size() * sizeof(KfacGemmJob);
  auto al = [](size_t n) { return (n + 255) / 256 * 256; };
  char* mem = nullptr;
  if (hipMalloc(&mem, al(b1) + al(b2) + al(b3) + 2 * al(b4)) != hipSuccess)
    return fail(DH_EHIP, "KFAC: device table allocation failed");
  K->dev_mem = mem;
  K->dev.slots = reinterpret_cast<KfacSlot*>(mem);
  K->dev.inv_jobs = reinterpret_cast<KfacInvJob*>(mem + al(b1));
  K->dev.block_jobs = reinterpret_cast<KfacBlockJob*>(mem + al(b1) + al(b2));
  K->dev.gemm1 = reinterpret_cast<KfacGemmJob*>(mem + al(b1) + al(b2) + al(b3));
  K->dev.gemm2 = reinterpret_cast<KfacGemmJob*>(mem + al(b1) + al(b2) + al(b3) + al(b4));
  bool ok = hipMemcpy(K->dev.slots, K->slots.data(), b1, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(K->dev.inv_jobs, K->inv.data(), b2, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(K->dev.block_jobs, K->bjobs.data(), b3, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(K->dev.gemm1, K->g1.data(), b4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(K->dev.gemm2, K->g2.data(), b4, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipFree(mem);
    K->dev_mem = nullptr;
    return fail(DH_EHIP, "KFAC: device table upload failed");
  }
  return DH_OK;
}

size_t kfac_step_ws(const KfacHost* K) {
  // kbuf (inverses, V, T, P V) | traces | GJ panel temporaries, doubles
  const size_t nd = align64(K->kbuf_doubles) + align64(K->slots.size()) +
                    align64(kfac_gj_tmp_doubles(K->dev.njobs, K->dev.nmax));
  return nd * sizeof(double);
}

}  // namespace

extern "C" {

size_t dh_vjp_workspace_bytes(const dh_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return carve_grad(h->d, batch, nullptr).total_bytes;
}

// Per chunk of walkers: forward, then the chain rule back to every reference parameter (chunks after the first add)
int dh_logpsi_vjp(dh_handle* h, const float* x, int B, const float* ct, float* grad, float* logpsi, void* ws,
                  size_t ws_bytes, void* stream) {
  const size_t need1 = h ? dh_vjp_workspace_bytes(h, 1) : 0;
  if (int rc = check_common(h, x, B, ws, ws_bytes, need1)) return rc;
  if (h && h->analytic()) return fail(DH_EINVAL, "the Laughlin wavefunction has no parameters to differentiate");
  if (!h->ref_set) return fail(DH_ESTATE, "the VJP needs parameters uploaded with dh_set_params_ref");
  if (!ct || !grad) return fail(DH_EINVAL, "null argument");
  if (h->d.D > 1024 || h->d.dh > 1024) return fail(DH_EINVAL, "VJP supports D <= 1024");
  int chunk = B;
  while (chunk > 1 && dh_vjp_workspace_bytes(h, chunk) > ws_bytes) chunk = (chunk + 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nw = std::min(chunk, B - b0);
    const GradWork w = carve_grad(h->d, nw, ws);
    const float* xc = x + (size_t)b0 * h->d.N * 2;
    vjp_forward(h, xc, nw, logpsi ? logpsi + 2 * (size_t)b0 : nullptr, w, s);
    if (int rc = reverse_walk(GradSites{{h, w, nw, s}, grad, b0 > 0}, xc, ct + 2 * (size_t)b0)) return rc;
  }
  return DH_OK;
}

// ---- the per-walker gradient Gram matrix (dh_ntk; ntk.hip)

size_t dh_ntk_workspace_bytes(const dh_handle* h, int batch) {
  if (!h || h->analytic() || h->d.sparse || batch < 1) return 0;
  return carve_ntk(h->d, batch, nullptr).total_bytes;
}

size_t dh_ntk_jvp_workspace_bytes(const dh_handle* h, int batch) {
  if (!h || h->analytic() || h->d.sparse || batch < 1) return 0;
  return carve_ntk(h->d, batch, nullptr, /*jvp=*/true).total_bytes;
}

int dh_ntk_tile_walkers(const dh_handle* h) {
  if (!h || h->analytic() || h->d.sparse) return 0;
  return ntk_tile_walkers(h->d.N);
}

// The argument checks of dh_ntk and dh_ntk_part (name "dh_ntk") and of dh_ntk_jvp (jvp: T may be
// null, then part 0 of 1, and the part is checked before the workspace); every one comes before
// the first device call.  args: the call's required pointers are all there
static int ntk_check(dh_handle* h, const std::string& name, bool jvp, const float* x, int B, bool args, const float* T,
                     void* ws, size_t ws_bytes, int part, int nparts) {
  if (!h) return fail(DH_EINVAL, "null handle");
  if (h->analytic()) return fail(DH_EINVAL, "the Laughlin wavefunction has no parameters to differentiate");
  if (h->d.sparse) return fail(DH_EINVAL, name + " supports orbital type \"full\" only");
  if (!x || B < 1) return fail(DH_EINVAL, "bad walkers");
  if (!args) return fail(DH_EINVAL, "null argument");
  if (h->d.D > 1024 || h->d.dh > 1024) return fail(DH_EINVAL, name + " supports D <= 1024");
  if (h->d.N > 32 || h->d.L > 16) return fail(DH_EINVAL, name + " supports N <= 32, L <= 16");
  const bool bad_part = nparts < 1 || part < 0 || part >= nparts;
  if (jvp && bad_part) return fail(DH_EINVAL, name + " needs 0 <= part < nparts");
  if (jvp && !T && nparts != 1) return fail(DH_EINVAL, name + " without T is part 0 of 1");
  // one chunk only: a pair of walkers from two chunks would need both chunks' activations
  if (!ws || ws_bytes < (jvp ? dh_ntk_jvp_workspace_bytes(h, B) : dh_ntk_workspace_bytes(h, B)))
    return fail(DH_ENOMEM, "workspace too small: " + name + " takes the whole batch in one chunk");
  if (bad_part) return fail(DH_EINVAL, "dh_ntk_part needs 0 <= part < nparts");
  if (!h->params_set) return fail(DH_ESTATE, "parameters not set");
  if (!h->ref_set) return fail(DH_ESTATE, name + " needs parameters uploaded with dh_set_params_ref");
  return DH_OK;
}

// the upper triangle of T (may be null with v), the rows of part `part` of `nparts` (everything else 0),
// not mirrored; with a direction v, jv [B] from the same walk
static int ntk_run(dh_handle* h, const float* x, int B, const float* ct, const float* v, float* T, float* jv,
                   float* logpsi, void* ws, int part, int nparts, hipStream_t s) {
  const NtkWork w = carve_ntk(h->d, B, ws, /*jvp=*/v != nullptr);
  float* lp = logpsi ? logpsi : w.g.logpsi;
  if ((T && hipMemsetAsync(T, 0, (size_t)B * B * sizeof(float), s) != hipSuccess) ||
      (jv && hipMemsetAsync(jv, 0, (size_t)B * sizeof(float), s) != hipSuccess))
    return fail(DH_EHIP, v ? "dh_ntk_jvp: clearing T / jv failed" : "dh_ntk: clearing T failed");
  vjp_forward(h, x, B, lp, w.g, s);
  launch_ntk_mask_ct(lp, ct, w.ctm, B, s);
  return reverse_walk(NtkSites{{h, w.g, B, s}, w, T, part, nparts, v, jv}, x, w.ctm);
}

int dh_ntk_part(dh_handle* h, const float* x, int B, const float* ct, float* T, float* logpsi, void* ws,
                size_t ws_bytes, int part, int nparts, void* stream) {
  if (int rc = ntk_check(h, "dh_ntk", false, x, B, ct && T, T, ws, ws_bytes, part, nparts)) return rc;
  return ntk_run(h, x, B, ct, nullptr, T, nullptr, logpsi, ws, part, nparts, (hipStream_t)stream);
}

int dh_ntk(dh_handle* h, const float* x, int B, const float* ct, float* T, float* logpsi, void* ws, size_t ws_bytes,
           void* stream) {
  if (int rc = dh_ntk_part(h, x, B, ct, T, logpsi, ws, ws_bytes, 0, 1, stream)) return rc;
  launch_ntk_mirror(T, B, (hipStream_t)stream);
  return check_launch();
}

int dh_ntk_jvp(dh_handle* h, const float* x, int B, const float* ct, const float* v, float* T, float* jv,
               float* logpsi, void* ws, size_t ws_bytes, int part, int nparts, void* stream) {
  if (int rc = ntk_check(h, "dh_ntk_jvp", true, x, B, ct && v && jv, T, ws, ws_bytes, part, nparts)) return rc;
  return ntk_run(h, x, B, ct, v, T, jv, logpsi, ws, part, nparts, (hipStream_t)stream);
}

int dh_ntk_mirror(float* T, int B, void* stream) {
  if (!T || B < 1) return fail(DH_EINVAL, "dh_ntk_mirror: null T or B < 1");
  launch_ntk_mirror(T, B, (hipStream_t)stream);
  return check_launch();
}

int dh_ntk_owner(const dh_handle* h, int walker, int nparts) {
  const int tw = dh_ntk_tile_walkers(h);
  if (tw < 1 || h->d.N > 32 || walker < 0 || nparts < 1) return -1;
  return (walker / tw) % nparts;
}

size_t dh_minsr_matrix_workspace_bytes(int Bg) { return Bg < 1 ? 0 : minsr_matrix_ws_doubles(Bg) * sizeof(double); }

int dh_minsr_matrix(const float* T, const unsigned char* valid, int Bg, double damping, double* A, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!T || !valid || !A) return fail(DH_EINVAL, "dh_minsr_matrix: null argument");
  if (Bg < 1 || Bg > (1 << 29)) return fail(DH_EINVAL, "dh_minsr_matrix: bad walker count");
  if (!ws || ws_bytes < dh_minsr_matrix_workspace_bytes(Bg))
    return fail(DH_ENOMEM, "dh_minsr_matrix: workspace too small");
  if (reinterpret_cast<uintptr_t>(ws) % 8 != 0) return fail(DH_EINVAL, "dh_minsr_matrix: workspace not 8-byte aligned");
  launch_minsr_matrix(T, valid, Bg, damping, A, reinterpret_cast<double*>(ws), (hipStream_t)stream);
  return check_launch();
}

int dh_kfac_layout(dh_handle* h, size_t* out, int n) {
  if (!h || h->analytic()) return fail(DH_EINVAL, "KFAC needs a Psiformer handle");
  if (int rc = kfac_plan(h)) return rc;
  const KfacHost& K = *h->kfac;
  // [0] statistics floats, [1] factor-matrix floats, [2] slots, [3] dense blocks, [4] generic
  // floats, [5] dh_kfac_step workspace bytes, then per block (kernel seg, bias seg or -1 as
  // SIZE_MAX, din, dout, A slot, G slot, scale x 1000), then per slot (n, offset)
  std::vector<size_t> v = {K.nstats, K.nmat, K.slots.size(), K.blocks.size(), (size_t)K.dev.gen.total,
                           kfac_step_ws(&K)};
  for (const auto& b : K.blocks)
    v.insert(v.end(), {(size_t)b.kseg, b.bseg >= 0 ? (size_t)b.bseg : SIZE_MAX, (size_t)b.din, (size_t)b.dout,
                       (size_t)b.a, (size_t)b.g, (size_t)std::lround(b.scale * 1000.f)});
  for (const auto& sl : K.slots) v.insert(v.end(), {(size_t)sl.n, sl.off});
  if (out)
    for (int i = 0; i < n && i < (int)v.size(); ++i) out[i] = v[i];
  return (int)v.size();
}

size_t dh_kfac_workspace_bytes(const dh_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return carve_grad(h->d, batch, nullptr, h->ref_offsets.back()).total_bytes;
}

int dh_kfac_vjp(dh_handle* h, const float* x, int B, const float* ct, float* grad, float* stats, float* logpsi,
                void* ws, size_t ws_bytes, void* stream) {
  if (!h || h->analytic()) return fail(DH_EINVAL, "KFAC needs a Psiformer handle");
  const size_t nref = h->ref_offsets.back();
  const size_t need1 = dh_kfac_workspace_bytes(h, 1);
  if (int rc = check_common(h, x, B, ws, ws_bytes, need1)) return rc;
  if (!h->ref_set) return fail(DH_ESTATE, "KFAC needs parameters uploaded with dh_set_params_ref");
  if (!stats) return fail(DH_EINVAL, "null statistics buffer");
  if (ct && !grad) return fail(DH_EINVAL, "ct given without grad");
  if (h->d.D > 1024 || h->d.dh > 1024) return fail(DH_EINVAL, "KFAC supports D <= 1024");
  if (int rc = kfac_device(h)) return rc;
  const KfacHost& K = *h->kfac;
  const Dims& d = h->d;
  int chunk = B;
  while (chunk > 1 && carve_grad(d, chunk, nullptr, nref).total_bytes > ws_bytes) chunk = (chunk + 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  KfacAcc kf{&K, stats, 1.f / ((float)B * d.N), {}};
  for (int a = 0, b = 0; a < 2; ++a) {
    const int na = a == 0 ? d.n_up : d.n_dn;
    if (na) kf.inv_rows_blk[b++] = 1.f / ((float)B * na);
  }
  const GradWork w = carve_grad(d, chunk, ws, nref);  // one layout: fgrad accumulates over chunks
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nw = std::min(chunk, B - b0);
    const float* xc = x + (size_t)b0 * d.N * 2;
    float* lp = logpsi ? logpsi + 2 * (size_t)b0 : w.logpsi;
    vjp_forward(h, xc, nw, lp, w, s);
    // the gradient pass first: the Fisher pass is the last reader of this chunk's w.F (reverse_walk)
    if (ct)
      if (int rc = reverse_walk(GradSites{{h, w, nw, s}, grad, b0 > 0}, xc, ct + 2 * (size_t)b0)) return rc;
    launch_kfac_fisher_ct(lp, nw, w.ctf, s);
    if (int rc = reverse_walk(FisherSites{{{h, w, nw, s}, w.fgrad, b0 > 0}, kf}, xc, w.ctf)) return rc;
  }
  // derived factors of the folded attention output (the kernels run Wol = Wo Wl as one map):
  // Dense_{2l+1}'s input a = [o, 1] [Wo; bo]:  A_Wl = [Wo; bo]^T A_o [Wo; bo]
  // the attention output's tangent dT Wl^T:    G_out = Wl G_T Wl^T
  const Rev r{h, w, chunk, s};  // for its reference-tree lookups
  const int D = d.D;
  float* Wt = w.P;                        // [D + 1][D]
  float* T = w.P + (size_t)(D + 1) * D;   // [D + 1][D]
  for (int l = 0; l < d.L; ++l) {
    const KfacLayerSlots& L = K.lay[l];
    launch_copy2d(r.ref(r.RS.lay(l, RWo)), D, Wt, D, D, D, s);
    launch_copy2d(r.ref(r.RS.lay(l, Rbo)), D, Wt + (size_t)D * D, D, 1, D, s);
    launch_small_gemm(D + 1, D, D + 1, stats + K.slots[L.A_o].off, D + 1, 0, Wt, D, 0, T, D, 0, s);
    launch_small_gemm(D, D, D + 1, Wt, D, 1, T, D, 0, stats + K.slots[L.A_Wl].off, D, 0, s);
    launch_small_gemm(D, D, D, r.ref(r.RS.lay(l, RWl)), D, 0, stats + K.slots[L.G_T].off, D, 0, T, D, 0, s);
    launch_small_gemm(D, D, D, T, D, 0, r.ref(r.RS.lay(l, RWl)), D, 1, stats + K.slots[L.G_out].off, D, 0, s);
  }
  launch_kfac_generic(w.fgrad, K.dev.gen, stats + K.nmat, 1.f / (float)B, s);
  return check_launch();
}

int dh_kfac_step(dh_handle* h, float* raw, const float* stats, float ema, float weight, const float* grad,
                 float* params, float lr, float damping, float norm_constraint, float* pgrad, double* info, void* ws,
                 size_t ws_bytes, void* stream) {
  if (!h || h->analytic()) return fail(DH_EINVAL, "KFAC needs a Psiformer handle");
  if (!raw || !grad || !pgrad || !info || !ws) return fail(DH_EINVAL, "null argument");
  if (!(weight > 0.f) || !(damping > 0.f)) return fail(DH_EINVAL, "KFAC needs weight > 0 and damping > 0");
  if (int rc = kfac_device(h)) return rc;
  const KfacHost& K = *h->kfac;
  const size_t nref = h->ref_offsets.back();
  if (ws_bytes < kfac_step_ws(&K)) return fail(DH_ENOMEM, "KFAC step workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double* kbuf = reinterpret_cast<double*>(ws);
  double* tr = kbuf + align64(K.kbuf_doubles);
  double* tmp = tr + align64(K.slots.size());
  if (stats) launch_kfac_ema(raw, stats, K.nstats, ema, s);
  launch_kfac_invert(K.dev, raw, 1.0 / weight, std::sqrt((double)damping), tr, kbuf, tmp, s);
  launch_kfac_precondition(K.dev, grad, raw + K.nmat, 1.0 / weight, damping, kbuf, pgrad, nref, info, s);
  if (params) launch_kfac_update(params, pgrad, nref, info, lr, norm_constraint, s);
  return check_launch();
}

}  // extern "C"
