// What the host files of the C ABI share: api.cpp (create / destroy, parameters, the forward
// Trunk, the value / MCMC / energy passes, debug hooks), api_grad.cpp (the gradient side),
// api_trial.cpp (the parameter-free trial states) and api_netobs.cpp (the handle-free estimators).
#pragma once
#include <string>
#include <vector>

#include "dh_internal.h"

namespace dh {

extern thread_local std::string g_err;  // dh_last_error's message (defined in api.cpp)

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(DH_EHIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

inline int check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(DH_EHIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return DH_OK;
}
inline size_t align64(size_t n) { return (n + 63) / 64 * 64; }

// Hands out 64-float-aligned pieces of a workspace (null base: sizes only) and counts the floats.
struct Carver {
  float* base;
  size_t off = 0;
  float* take(size_t n) {
    float* p = base ? base + off : nullptr;
    off += align64(n);
    return p;
  }
  size_t bytes() const { return off * sizeof(float); }
};

// Optional per-kernel HIP-event timing (bench.py reads it to compute the live roofline).
struct ProfRec {
  hipEvent_t a, b;
  int kind;
  double flops, bytes;
};
struct Profiler {
  bool on = false;
  std::vector<ProfRec> recs;
  size_t used = 0;
};

// KFAC plan (dh_kfac_*): factor slots of the statistics buffer, the dense blocks and the
// generic parameters (oracle/kfac.py restates the algorithm), plus device job tables.
struct KfacLayerSlots {
  int A_h, G_q, G_k, G_v, A_o, G_T, A_Wl, G_out, A_h1, G_z;
};
struct KfacHost {
  std::vector<KfacSlot> slots;
  size_t nmat = 0;     // floats of all factor slots
  size_t nstats = 0;   // + the generic diagonal
  int s_feat = -1, s_h0 = -1;
  KfacLayerSlots lay[16];
  int A_orb[2] = {-1, -1}, G_orb[2][2] = {{-1, -1}, {-1, -1}};
  int A_lll = -1, G_lll = -1;  // "sparse" orbitals: the complex lll_weight block
  struct Blk {
    int kseg, bseg, din, dout, a, g;
    float scale;
  };
  std::vector<Blk> blocks;
  std::vector<KfacInvJob> inv;
  std::vector<KfacBlockJob> bjobs;
  std::vector<KfacGemmJob> g1, g2;
  size_t kbuf_doubles = 0;  // inverse matrices + V, T, P V per block
  KfacDevPlan dev{};
  void* dev_mem = nullptr;  // one allocation for the device tables
};

}  // namespace dh

struct dh_handle {
  dh_config cfg;
  dh::Dims d;
  dh::Params p{};
  std::vector<size_t> offsets;      // packed layout, nseg + 1
  std::vector<size_t> ref_offsets;  // reference-tree layout (dh_ref_layout), nseg + 1
  float* params = nullptr;
  float* ref = nullptr;      // reference-layout copy (dh_set_params_ref; needed by the VJP)
  uint16_t* wb = nullptr;    // backward split-bf16 planes (untransposed weights)
  float* wbt = nullptr;      // backward exact-f32 transposed weights (D % 32 != 0)
  float* norm = nullptr;  // sqrt(binom(2Q, Q-m)), M floats (device)
  float* wt = nullptr;    // transposed GEMM weights for the NT kernels (device)
  uint16_t* wp = nullptr;  // split-bf16 weight planes for the x6 kernels (device)
  float* mqk = nullptr;    // layer 1's per-head score forms (attn_val.h, launch_lowrank_qk)
  float* ofw = nullptr;    // layer 1's feature-space output map U^T [256 pad][KO] (launch_ofeat_weight)
  uint16_t* ofp = nullptr;  // its split-bf16 planes [3][x6_plane_rows(D)][KO]
  float* l1w = nullptr;     // layer 1's coefficient-space maps B^T, V^T (launch_l1_basis)
  float* w2t = nullptr;     // envelope first: W2T [256 2N][KE] (launch_env_w2)
  uint16_t* w2p = nullptr;  // its planes
  uint16_t* l1p = nullptr;  // their planes
  int gemm_mode = DH_GEMM_X6_ALL;
  std::vector<float> norm_host;
  bool params_set = false;
  bool ref_set = false;
  // Which wavefunction the handle is.  All but the Psiformer are analytic: no parameters, one
  // kernel file each (laughlin.hip, cf.hip, pfaffian.hip, halperin.hip, quasihole.hip), created
  // and launched by api_trial.cpp, which alone reads what its state keeps here
  enum State { PSIFORMER, LAUGHLIN, JAIN, PFAFFIAN, HALPERIN, QUASIHOLE };
  struct Trial {
    State state = PSIFORMER;
    std::vector<int> table_host;     // Laughlin: the exponents [2][N] = (Q1 + m_j, Q1 - m_j) and the quasiparticle
                                     // flag; Jain: cf.hip's column table; the other states: empty
    int* table = nullptr;            // its device copy (uploaded at first use, freed by dh_destroy)
    int cf_dense = 0;                // Jain: the number of level-1 (dense) columns
    int halperin[3] = {0, 0, 0};     // Halperin: m_up, m_dn, n (arguments of dh_create_halperin, not dh_config fields)
    dh::QuasiholeState quasihole{};  // Quasihole: the base's weights and the holes (dh_create_quasihole)
  } trial;
  bool analytic() const { return trial.state != PSIFORMER; }
  dh::KfacHost* kfac = nullptr;   // KFAC plan (built at first dh_kfac_* call)
  dh::Profiler prof;
};

namespace dh {

struct ProfScope {
  dh_handle* h;
  hipStream_t s;
  ProfRec* r = nullptr;
  ProfScope(dh_handle* h_, int kind, double flops, double bytes, hipStream_t s_) : h(h_), s(s_) {
    if (!h->prof.on) return;
    Profiler& P = h->prof;
    if (P.used == P.recs.size()) {
      ProfRec nr{};
      (void)hipEventCreate(&nr.a);
      (void)hipEventCreate(&nr.b);
      P.recs.push_back(nr);
    }
    r = &P.recs[P.used++];
    r->kind = kind;
    r->flops = flops;
    r->bytes = bytes;
    (void)hipEventRecord(r->a, s);
  }
  ~ProfScope() {
    if (r) (void)hipEventRecord(r->b, s);
  }
};
#define PROF(kind, flops, bytes) ProfScope prof_scope_##__LINE__(h, kind, (double)(flops), (double)(bytes), s)

// The kernel classes of the profiler's records
enum ProfKind { PK_GEMM = 0, PK_ATTN, PK_LN, PK_INPUT, PK_DET_VALUE, PK_DET_ENERGY, PK_MCMC, PK_COUNT };
// channel-mode (C > 1) launches of GEMM/attention/LayerNorm/input are recorded as kind + PK_CH;
// PK_L1CH: the local energy's layer 1 in one launch (gemm_lnch MODE 2)
constexpr int PK_CH = PK_COUNT, PK_L1CH = PK_COUNT + 4, PK_TOTAL = PK_COUNT + 5;

// api_trial.cpp.  create_trial: dh_create for every network type but the Psiformer (the handle
// of an analytic state, or the refusal).  launch_trial: the kernel of an analytic state on nw
// walkers, log psi [nw][2] (e_l == nullptr), or the local energy e_l [nw][2] and obs [nw][8];
// uploads the state's table at first use if it has one.
int create_trial(const dh_config* cfg, dh_handle** out);
int launch_trial(dh_handle* h, const float* x, float* logpsi, float* e_l, float* obs, int nw, hipStream_t s);
// api_netobs.cpp: the size check of dh_hole_gram, which dh_hole_logs (api_trial.cpp) shares
const char* hole_gram_error(int B, int K);

inline int check_common(dh_handle* h, const void* x, int B, void* ws, size_t ws_bytes, size_t need) {
  if (!h) return fail(DH_EINVAL, "null handle");
  if (!h->params_set) return fail(DH_ESTATE, "parameters not set");
  if (!x || B < 1) return fail(DH_EINVAL, "bad walkers");
  if (!ws || ws_bytes < need) return fail(DH_ENOMEM, "workspace too small");
  return DH_OK;
}

// Reference-tree segment indices (dh_ref_layout)
struct RefSeg {
  int L, NB, sparse;
  int W0() const { return 0; }
  int lay(int l, int k) const { return 1 + 15 * l + k; }  // k: Wq bq Wk bk Wv bv Wo bo Wl ln1s ln1b Wm bm ln2s ln2b
  int orb_kernel(int i) const { return 1 + 15 * L + 2 * i; }
  int orb_bias(int i) const { return 2 + 15 * L + 2 * i; }
  int lll(int k) const { return 1 + 15 * L + 4 * NB + k; }  // "sparse": lll_weight kernel, bias
  int jas(int k) const { return 1 + 15 * L + 4 * NB + (sparse ? 2 : 0) + k; }
};
enum { RWq = 0, Rbq, RWk, Rbk, RWv, Rbv, RWo, Rbo, RWl, Rln1s, Rln1b, RWm, Rbm, Rln2s, Rln2b };

// One dense GEMM Y = X W (+ bias) (+ Res) of the family: the split-bf16 planes Wp, the transposed
// copy Wt (NT) or W itself (row stride ldw).
inline void dense_gemm(int family, const float* X, int ldx, const float* W, const float* Wt, const uint16_t* Wp,
                       int ldw, const float* bias, const float* Res, int ldr, float* Y, int ldy, int rows, int ncols,
                       int K, int C, hipStream_t s) {
  if (family == GEMM_X6)
    launch_gemm_x6(X, ldx, Wp, x6_plane_rows(ncols), bias, Res, ldr, Y, ldy, rows, ncols, K, C, s);
  else if (family == GEMM_F32_NT)
    launch_gemm_nt(X, ldx, Wt, K, bias, Res, ldr, Y, ldy, rows, ncols, K, C, s);
  else
    launch_gemm(X, ldx, W, ldw, bias, Res, ldr, Y, ldy, rows, ncols, K, C, s);
}

}  // namespace dh
