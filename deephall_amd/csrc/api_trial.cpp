// The host side of the parameter-free trial states (laughlin.hip, cf.hip, pfaffian.hip, halperin.hip,
// quasihole.hip): what each state asks of N, the flux and its own arguments, the handle it gets, and
// the one launcher behind dh_logpsi, dh_mcmc_step and dh_local_energy.  Also the handle-free dh_hole_*
// calls: a table of hole configurations checked as dh_create_quasihole checks one, log psi of all of
// them on the same walkers, and the Gram matrix of their ratios.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "api_internal.h"

using namespace dh;

namespace {

// What every analytic state asks of N, the flux and the interaction; name starts the messages
int check_analytic(const dh_config* cfg, const std::string& name, int n_min) {
  const int N = cfg->n_up + cfg->n_dn;
  if (cfg->n_up < 0 || cfg->n_dn < 0 || N < n_min || N > 32)
    return fail(DH_EINVAL, name + ": need " + std::to_string(n_min) + " <= N <= 32 electrons");
  if (cfg->flux < 1 || cfg->flux > 126) return fail(DH_EINVAL, name + " needs 1 <= flux <= 126");
  if (cfg->interaction_type != DH_INTERACTION_COULOMB && cfg->interaction_type != DH_INTERACTION_HARMONIC)
    return fail(DH_EINVAL, name + ": bad interaction type");
  return DH_OK;
}

// An energy kernel is one workgroup per walker with everything in LDS: refuse what does not fit.
// who: who needs the bytes, "Pfaffian: N = 30 needs"
int check_lds(const std::string& who, size_t bytes) {
  if (bytes <= 160 * 1024) return DH_OK;
  return fail(DH_EINVAL, who + " " + std::to_string(bytes) + " bytes of LDS; the one-workgroup kernel has 160 KiB");
}
std::string n_needs(const char* name, int N) { return std::string(name) + ": N = " + std::to_string(N) + " needs"; }

// What dh_create_cf, dh_create_halperin and dh_create_quasihole check first: no null argument,
// dh_config's size, a second argument struct's (aux) if there is one, the network type.  pre starts
// the first messages ("" for dh_create_cf), name the last.
int check_entry(bool args, const dh_config* cfg, const std::string& pre, const std::string& name, int type,
                const char* fn, const char* type_name, const char* aux = nullptr, size_t aux_got = 0, size_t aux_want = 0) {
  if (!args) return fail(DH_EINVAL, pre + "null argument");
  if (cfg->struct_size != sizeof(dh_config))
    return fail(DH_EINVAL, pre + "dh_config.struct_size must equal sizeof(dh_config)");
  if (aux && aux_got != aux_want)
    return fail(DH_EINVAL, pre + aux + ".struct_size must equal sizeof(" + aux + ") (" + std::to_string(aux_want) + " bytes)");
  if (cfg->network_type != type) return fail(DH_EINVAL, name + ": " + fn + " needs network_type " + type_name);
  return DH_OK;
}

// The Halperin rule: m_up, m_dn odd, n >= 0, and both species at the flux of their degree in (u, v)
// (the exponent of an empty or single-electron species is free beyond its parity).  holes: null for
// the plain state, else the degree (h_up, h_dn) that pinned holes add, which the messages then name.
int check_halperin(const dh_config* cfg, const std::string& name, int m_up, int m_dn, int n_int, const int* holes) {
  if (m_up < 1 || m_dn < 1 || m_up % 2 == 0 || m_dn % 2 == 0)
    return fail(DH_EINVAL, name + ": m_up and m_dn must be odd and >= 1, got " + std::to_string(m_up) + ", " +
                               std::to_string(m_dn));
  if (n_int < 0) return fail(DH_EINVAL, name + ": need n >= 0, got " + std::to_string(n_int));
  const int64_t f_up = (int64_t)m_up * (cfg->n_up - 1) + (int64_t)n_int * cfg->n_dn + (holes ? holes[0] : 0);
  const int64_t f_dn = (int64_t)m_dn * (cfg->n_dn - 1) + (int64_t)n_int * cfg->n_up + (holes ? holes[1] : 0);
  if (cfg->n_up > 0 && cfg->flux != f_up)
    return fail(DH_EINVAL, name + ": the up electrons live at flux m_up (n_up - 1) + n n_dn" + (holes ? " + h_up" : "") +
                               " = " + std::to_string(f_up) + ", got " + std::to_string(cfg->flux));
  if (cfg->n_dn > 0 && cfg->flux != f_dn)
    return fail(DH_EINVAL, name + ": the down electrons live at flux m_dn (n_dn - 1) + n n_up" +
                               (holes ? " + h_dn" : "") + " = " + std::to_string(f_dn) + ", got " +
                               std::to_string(cfg->flux));
  return DH_OK;
}

// The Moore-Read rule: the flux of N electrons with 2 p vortices each and the degree extra that holes
// add (k + the Abelian holes).  Its refusals are worded differently by the plain state and by the
// quasihole base, which also checks its groups between them: the messages stay with the callers.
int64_t moore_read_flux(int N, int p, int extra) { return (int64_t)2 * p * (N - 1) - 1 + extra; }

// Laughlin(nspins, flux, cf_flux, excitation_lz) (laughlin.py:19-46): exponents of the
// composite-fermion orbitals, in doubled units (2 Q1, 2 m are integers)
int laughlin_exponents(const dh_config* cfg, std::vector<int>& ex) {
  const int N = cfg->n_up + cfg->n_dn;
  const int p = cfg->cf_flux < 1 ? 1 : cfg->cf_flux;
  const int q2 = cfg->flux - 2 * p * (N - 1);  // 2 Q1
  if (q2 < 0) return fail(DH_EINVAL, "Laughlin: flux too small for N electrons (Q1 < 0)");
  std::vector<int> m2;  // 2 m
  if (N == q2 + 1) {  // ground state
    for (int m = -q2; m <= q2; m += 2) m2.push_back(m);
  } else if (N == q2) {  // quasihole: m = -Q1 .. Q1 without -lz (laughlin.py:66-73)
    const double lz2 = 2.0 * cfg->excitation_lz;
    const int l2 = (int)std::lround(lz2);
    if (std::fabs(lz2 - l2) > 1e-6 || ((l2 - q2) % 2) != 0 || std::abs(l2) > q2)
      return fail(DH_EINVAL, "Laughlin quasihole: impossible excitation_lz");
    for (int m = -q2; m < -l2; m += 2) m2.push_back(m);
    for (int m = q2; m > -l2; m -= 2) m2.push_back(m);
  } else if (N == q2 + 2) {  // quasiparticle: m = -Q1 .. Q1, then the excited orbital (laughlin.py:82-100)
    const double lz2 = 2.0 * cfg->excitation_lz;
    const int l2 = (int)std::lround(lz2);
    if (std::fabs(lz2 - l2) > 1e-6 || ((l2 - q2) % 2) != 0 || std::abs(l2) > q2 + 2)
      return fail(DH_EINVAL, "Laughlin quasiparticle: impossible excitation_lz");
    for (int m = -q2; m <= q2; m += 2) m2.push_back(m);
    m2.push_back(l2);  // last column: A = Q1 + m1, B = Q1 - m1 (each >= -1)
  } else {
    return fail(DH_EINVAL, "Laughlin: filling not supported");
  }
  if ((int)m2.size() != N) return fail(DH_EINVAL, "Laughlin: orbital count mismatch");
  ex.assign(2 * N + 1, 0);
  for (int j = 0; j < N; ++j) {
    ex[j] = (q2 + m2[j]) / 2;
    ex[N + j] = (q2 - m2[j]) / 2;
  }
  ex[2 * N] = N == q2 + 2 ? 1 : 0;  // the kernel's quasiparticle flag
  if (laughlin_smem_bytes(N) > 160 * 1024)  // its own wording, no byte count
    return fail(DH_EINVAL, "Laughlin: N too large for the one-workgroup kernel's LDS (160 KiB)");
  return DH_OK;
}

// The handle of an analytic state: no network dimensions.  table: Laughlin's exponents, Jain's columns
dh_handle* analytic_handle(const dh_config* cfg, dh_handle::State state, const std::vector<int>& table) {
  const int N = cfg->n_up + cfg->n_dn;
  auto* h = new dh_handle();
  h->cfg = *cfg;
  h->trial.state = state;
  h->trial.table_host = table;
  Dims& d = h->d;
  d = Dims{};
  d.N = N;
  d.n_up = cfg->n_up;
  d.n_dn = cfg->n_dn;
  d.T = 2 * N;
  d.C = 2 * N + 5;
  d.M = 1;
  d.Q = 0.5f * cfg->flux;
  d.r = cfg->radius > 0.f ? cfg->radius : std::sqrt(d.Q);
  d.H = 1;
  d.dh = 4;
  d.D = 4;
  d.L = 0;
  d.K = 1;
  d.NB = 1;
  d.orb_cols = 0;
  d.ld_orb = 0;
  d.interaction = cfg->interaction_type;
  d.lambda = cfg->interaction_strength;
  h->offsets = {0};
  h->ref_offsets = {0};
  h->params_set = h->ref_set = true;  // nothing to upload
  return h;
}

// Jain state with two Lambda levels (cf.hip).  occ: [n_occ][2] = (level, 2 m), or null for the
// ground state with both levels filled (N = 4 Q1 + 4: all of level 0, then all of level 1, m
// ascending).  Fills the kernel's column table.
int jain_table(const dh_config* cfg, const int* occ, int n_occ, std::vector<int>& tab, int& n_dense) {
  const int N = cfg->n_up + cfg->n_dn;
  const int p = cfg->cf_flux < 1 ? 1 : cfg->cf_flux;
  const int q2 = cfg->flux - 2 * p * (N - 1);  // 2 Q1
  if (q2 < 0) return fail(DH_EINVAL, "Jain: flux too small for N electrons (Q1 < 0)");
  std::vector<int> lev, m2;
  if (!occ) {
    if (N != 2 * q2 + 4)
      return fail(DH_EINVAL, "Jain: no ground state of two filled levels at this filling (needs N = 4 Q1 + 4)");
    for (int n = 0; n < 2; ++n)
      for (int m = -q2 - 2 * n; m <= q2 + 2 * n; m += 2) {
        lev.push_back(n);
        m2.push_back(m);
      }
  } else {
    if (n_occ != N) return fail(DH_EINVAL, "Jain: the occupation needs one orbital per electron (n_occ = N)");
    for (int j = 0; j < N; ++j) {
      const int n = occ[2 * j], m = occ[2 * j + 1];
      if (n != 0 && n != 1) return fail(DH_EINVAL, "Jain: Lambda level must be 0 or 1");
      if (((m - q2) % 2) != 0) return fail(DH_EINVAL, "Jain: 2 m must have the parity of 2 Q1");
      if (std::abs(m) > q2 + 2 * n) return fail(DH_EINVAL, "Jain: |m| > Q1 + level");
      for (int k = 0; k < j; ++k)
        if (lev[k] == n && m2[k] == m) return fail(DH_EINVAL, "Jain: orbital occupied twice");
      lev.push_back(n);
      m2.push_back(m);
    }
  }
  n_dense = 0;
  tab.assign(3 * N + 2, 0);
  for (int j = 0; j < N; ++j) {
    tab[3 * j] = lev[j];
    tab[3 * j + 1] = (q2 + m2[j]) / 2;  // A >= -1
    tab[3 * j + 2] = (q2 - m2[j]) / 2;  // B >= -1
    if (lev[j]) {
      tab.push_back(j);
      ++n_dense;
    }
  }
  tab[3 * N] = n_dense;
  tab[3 * N + 1] = p;
  return check_lds("Jain: N and the number of level-1 orbitals need", cf_smem_bytes(N, n_dense, true));
}

int create_jain(const dh_config* cfg, const int* occ, int n_occ, dh_handle** out) {
  if (int rc = check_analytic(cfg, "Jain", 1)) return rc;
  std::vector<int> tab;
  int n_dense = 0;
  if (int rc = jain_table(cfg, occ, n_occ, tab, n_dense)) return rc;
  dh_handle* h = analytic_handle(cfg, dh_handle::JAIN, tab);
  h->trial.cf_dense = n_dense;
  *out = h;
  return DH_OK;
}

// Moore-Read Pfaffian (pfaffian.hip): N even at flux 2 p (N - 1) - 1, nothing else to choose
int create_pfaffian(const dh_config* cfg, dh_handle** out) {
  const int N = cfg->n_up + cfg->n_dn, p = cfg->cf_flux;
  if (int rc = check_analytic(cfg, "Pfaffian", 2)) return rc;
  if (N % 2) return fail(DH_EINVAL, "Pfaffian: the paired state needs an even number of electrons");
  if (p < 1) return fail(DH_EINVAL, "Pfaffian: need cf_flux >= 1");
  const int64_t f = moore_read_flux(N, p, 0);
  if (cfg->flux != f)
    return fail(DH_EINVAL, "Pfaffian: the state lives at flux 2 cf_flux (N - 1) - 1 = " + std::to_string(f) + ", got " +
                               std::to_string(cfg->flux));
  if (int rc = check_lds(n_needs("Pfaffian", N), pfaffian_smem_bytes(N, true))) return rc;
  *out = analytic_handle(cfg, dh_handle::PFAFFIAN, {});
  return DH_OK;
}

// Halperin (m_up, m_dn, n) (halperin.hip)
int create_halperin(const dh_config* cfg, int m_up, int m_dn, int n_int, dh_handle** out) {
  const int N = cfg->n_up + cfg->n_dn;
  if (int rc = check_analytic(cfg, "Halperin", 1)) return rc;
  if (int rc = check_halperin(cfg, "Halperin", m_up, m_dn, n_int, nullptr)) return rc;
  if (int rc = check_lds(n_needs("Halperin", N), halperin_smem_bytes(N, true))) return rc;
  dh_handle* h = analytic_handle(cfg, dh_handle::HALPERIN, {});
  h->trial.halperin[0] = m_up;
  h->trial.halperin[1] = m_dn;
  h->trial.halperin[2] = n_int;
  *out = h;
  return DH_OK;
}

// Pinned quasiholes (quasihole.hip) on a Halperin or a Pfaffian base: every hole adds one to the
// degree of the electrons it acts on, a group of k holes k to the degree of every electron.
// Everything dh_create_quasihole asks of cfg and q, and the kernel's state with the holes' spinors:
// shared with the configurations of dh_hole_table.  name starts the messages.
int quasihole_state(const dh_config* cfg, const dh_quasihole* q, const std::string& name, QuasiholeState& st) {
  const int N = cfg->n_up + cfg->n_dn;
  const bool pf = q->base == DH_QUASIHOLE_PFAFFIAN;
  if (q->base != DH_QUASIHOLE_HALPERIN && !pf)
    return fail(DH_EINVAL, name + ": base must be DH_QUASIHOLE_HALPERIN or DH_QUASIHOLE_PFAFFIAN, got " +
                               std::to_string(q->base));
  if (int rc = check_analytic(cfg, name, pf ? 2 : 1)) return rc;
  if (q->n_holes < 1 || q->n_holes > DH_QUASIHOLE_MAX_HOLES)
    return fail(DH_EINVAL, name + ": need 1 <= n_holes <= " + std::to_string(DH_QUASIHOLE_MAX_HOLES) + ", got " +
                               std::to_string(q->n_holes) +
                               (q->n_holes == 0 ? (pf ? " (without holes this is the pfaffian state: dh_create)"
                                                      : " (without holes this is the halperin state: dh_create_halperin)")
                                                : ""));
  int count[5] = {0, 0, 0, 0, 0};
  st = QuasiholeState{};
  st.pfaffian = pf;
  st.n_holes = q->n_holes;
  for (int a = 0; a < q->n_holes; ++a) {
    const double th = q->holes[a][0], ph = q->holes[a][1];
    const int kind = q->kind[a];
    if (!std::isfinite(th) || !std::isfinite(ph))
      return fail(DH_EINVAL, name + ": hole " + std::to_string(a) + " has a non-finite angle");
    if (th < 0.0 || th > M_PI)
      return fail(DH_EINVAL, name + ": hole " + std::to_string(a) + " needs 0 <= theta <= pi, got " + std::to_string(th));
    const bool ok = pf ? (kind == DH_HOLE_BOTH || kind == DH_HOLE_GROUP_A || kind == DH_HOLE_GROUP_B)
                       : (kind == DH_HOLE_BOTH || kind == DH_HOLE_UP || kind == DH_HOLE_DOWN);
    if (!ok)
      return fail(DH_EINVAL, name + ": hole " + std::to_string(a) + " has kind " + std::to_string(kind) +
                                 (pf ? ", the pfaffian base takes DH_HOLE_BOTH, DH_HOLE_GROUP_A and DH_HOLE_GROUP_B"
                                     : ", the halperin base takes DH_HOLE_BOTH, DH_HOLE_UP and DH_HOLE_DOWN"));
    ++count[kind];
    st.kind[a] = kind;
    st.uv[a][0] = std::cos(0.5 * th) * std::cos(0.5 * ph);
    st.uv[a][1] = std::cos(0.5 * th) * std::sin(0.5 * ph);
    st.uv[a][2] = std::sin(0.5 * th) * std::cos(0.5 * ph);
    st.uv[a][3] = -std::sin(0.5 * th) * std::sin(0.5 * ph);
  }
  if (pf) {
    const int p = q->p, k = count[DH_HOLE_GROUP_A];
    if (N % 2) return fail(DH_EINVAL, name + ": the pfaffian base needs an even number of electrons");
    if (p < 1) return fail(DH_EINVAL, name + ": the pfaffian base needs p >= 1, got " + std::to_string(p));
    if (count[DH_HOLE_GROUP_B] != k)
      return fail(DH_EINVAL, name + ": the groups A and B need the same number of holes, got " + std::to_string(k) +
                                 " and " + std::to_string(count[DH_HOLE_GROUP_B]));
    const int64_t f = moore_read_flux(N, p, k + count[DH_HOLE_BOTH]);
    if (cfg->flux != f)
      return fail(DH_EINVAL, name + ": the state lives at flux 2 p (N - 1) - 1 + k + (Abelian holes) = " +
                                 std::to_string(f) + ", got " + std::to_string(cfg->flux));
    st.m_up = st.m_dn = st.n_int = 2 * p;
  } else {
    const int holes[2] = {count[DH_HOLE_BOTH] + count[DH_HOLE_UP], count[DH_HOLE_BOTH] + count[DH_HOLE_DOWN]};
    if (int rc = check_halperin(cfg, name, q->m_up, q->m_dn, q->n_inter, holes)) return rc;
    st.m_up = q->m_up;
    st.m_dn = q->m_dn;
    st.n_int = q->n_inter;
  }
  return check_lds(name + ": N = " + std::to_string(N) + " needs", quasihole_smem_bytes(N, pf, true));
}

int create_quasihole(const dh_config* cfg, const dh_quasihole* q, dh_handle** out) {
  QuasiholeState st;
  if (int rc = quasihole_state(cfg, q, "Quasihole", st)) return rc;
  dh_handle* h = analytic_handle(cfg, dh_handle::QUASIHOLE, {});
  h->trial.quasihole = st;
  *out = h;
  return DH_OK;
}

// The packed table of dh_hole_table: the spinors, then the kinds
struct HoleTable {
  double uv[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES][4];
  int kind[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES];
};

// What dh_hole_table and dh_hole_logs check: the entry (check_entry), the number of configurations,
// and every configuration as the dh_quasihole it is (quasihole_state).  Fills the table and base,
// the state of configuration 0: the weights, the base and n_holes are the same in all.
int hole_table(const dh_config* cfg, const dh_hole_configs* hc, bool args, HoleTable& tab, QuasiholeState& base) {
  if (int rc = check_entry(args && cfg && hc, cfg, "Holes: ", "Holes", DH_NETWORK_QUASIHOLE, "dh_hole_table",
                           "DH_NETWORK_QUASIHOLE", "dh_hole_configs", hc ? hc->struct_size : 0, sizeof(dh_hole_configs)))
    return rc;
  if (hc->n_configs < 1 || hc->n_configs > DH_HOLE_MAX_CONFIGS)
    return fail(DH_EINVAL, "Holes: need 1 <= n_configs <= " + std::to_string(DH_HOLE_MAX_CONFIGS) + ", got " +
                               std::to_string(hc->n_configs));
  std::memset(&tab, 0, sizeof(tab));
  for (auto& row : tab.kind)
    for (int& k : row) k = -1;
  for (int c = 0; c < hc->n_configs; ++c) {
    dh_quasihole q{};
    q.struct_size = sizeof(dh_quasihole);
    q.base = hc->base;
    q.m_up = hc->m_up;
    q.m_dn = hc->m_dn;
    q.n_inter = hc->n_inter;
    q.p = hc->p;
    q.n_holes = hc->n_holes;
    const int nh = std::min(std::max(hc->n_holes, 0), DH_QUASIHOLE_MAX_HOLES);  // the check refuses the rest
    for (int a = 0; a < nh; ++a) {
      q.kind[a] = hc->kind[c][a];
      q.holes[a][0] = hc->holes[c][a][0];
      q.holes[a][1] = hc->holes[c][a][1];
    }
    QuasiholeState st;
    if (int rc = quasihole_state(cfg, &q, "Holes: configuration " + std::to_string(c), st)) return rc;
    for (int a = 0; a < st.n_holes; ++a) {
      tab.kind[c][a] = st.kind[a];
      for (int j = 0; j < 4; ++j) tab.uv[c][a][j] = st.uv[a][j];
    }
    if (c == 0) base = st;
  }
  return DH_OK;
}

}  // namespace

int dh::create_trial(const dh_config* cfg, dh_handle** out) {
  if (cfg->network_type == DH_NETWORK_LAUGHLIN) {
    if (int rc = check_analytic(cfg, "Laughlin", 1)) return rc;
    std::vector<int> ex;
    if (int rc = laughlin_exponents(cfg, ex)) return rc;
    *out = analytic_handle(cfg, dh_handle::LAUGHLIN, ex);
    return DH_OK;
  }
  if (cfg->network_type == DH_NETWORK_JAIN) return create_jain(cfg, nullptr, 0, out);
  if (cfg->network_type == DH_NETWORK_PFAFFIAN) return create_pfaffian(cfg, out);
  if (cfg->network_type == DH_NETWORK_HALPERIN)
    return fail(DH_EINVAL, "Halperin: the exponents (m_up, m_dn, n) are arguments of dh_create_halperin, not dh_create");
  if (cfg->network_type == DH_NETWORK_QUASIHOLE)
    return fail(DH_EINVAL, "Quasihole: the base and the holes are arguments of dh_create_quasihole, not dh_create");
  return fail(DH_EINVAL, "bad network type");
}

int dh::launch_trial(dh_handle* h, const float* x, float* logpsi, float* e_l, float* obs, int nw, hipStream_t s) {
  dh_handle::Trial& t = h->trial;
  if (!t.table && !t.table_host.empty()) {
    HIP_TRY(hipMalloc(&t.table, t.table_host.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(t.table, t.table_host.data(), t.table_host.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  PROF(e_l ? PK_DET_ENERGY : PK_DET_VALUE, 0.0, e_l ? 48.0 * nw : 8.0 * nw * h->d.N);
  if (t.state == dh_handle::QUASIHOLE)
    launch_quasihole(h->d, x, t.quasihole, logpsi, e_l, obs, nw, s);
  else if (t.state == dh_handle::HALPERIN)
    launch_halperin(h->d, x, t.halperin[0], t.halperin[1], t.halperin[2], logpsi, e_l, obs, nw, s);
  else if (t.state == dh_handle::PFAFFIAN)
    launch_pfaffian(h->d, x, h->cfg.cf_flux, logpsi, e_l, obs, nw, s);
  else if (t.state == dh_handle::JAIN)
    launch_cf(h->d, x, t.table, t.cf_dense, logpsi, e_l, obs, nw, s);
  else
    launch_laughlin(h->d, x, t.table, logpsi, e_l, obs, nw, s);
  return check_launch();
}

extern "C" {
int dh_create_quasihole(const dh_config* cfg, const dh_quasihole* q, dh_handle** out) {
  const int rc = check_entry(cfg && q && out, cfg, "Quasihole: ", "Quasihole", DH_NETWORK_QUASIHOLE, "dh_create_quasihole",
                             "DH_NETWORK_QUASIHOLE", "dh_quasihole", q ? q->struct_size : 0, sizeof(dh_quasihole));
  return rc ? rc : create_quasihole(cfg, q, out);
}

size_t dh_hole_table_bytes(void) { return sizeof(HoleTable); }

int dh_hole_table(const dh_config* cfg, const dh_hole_configs* configs, void* table_host, size_t bytes) {
  HoleTable tab;
  QuasiholeState base;
  if (int rc = hole_table(cfg, configs, table_host != nullptr, tab, base)) return rc;
  if (bytes < sizeof(HoleTable)) return fail(DH_EINVAL, "Holes: table smaller than dh_hole_table_bytes");
  std::memcpy(table_host, &tab, sizeof(tab));
  return DH_OK;
}

int dh_hole_logs(const dh_config* cfg, const dh_hole_configs* configs, const float* x, int B, const void* table,
                 size_t table_bytes, double* L, void* stream) {
  HoleTable tab;  // checked and discarded: the kernel reads the caller's device copy
  QuasiholeState base;
  if (int rc = hole_table(cfg, configs, x && table && L, tab, base)) return rc;
  if (const char* e = hole_gram_error(B, configs->n_configs)) return fail(DH_EINVAL, e);
  if ((int64_t)B * (cfg->n_up + cfg->n_dn) > INT32_MAX) return fail(DH_EINVAL, "Holes: B nelec >= 2^31");
  if (table_bytes < sizeof(HoleTable)) return fail(DH_EINVAL, "Holes: table smaller than dh_hole_table_bytes");
  launch_hole_logs(x, B, cfg->n_up + cfg->n_dn, cfg->n_up, base, configs->n_configs, table, L, (hipStream_t)stream);
  return check_launch();
}

int dh_create_halperin(const dh_config* cfg, int m_up, int m_dn, int n_inter, dh_handle** out) {
  const int rc = check_entry(cfg && out, cfg, "Halperin: ", "Halperin", DH_NETWORK_HALPERIN, "dh_create_halperin",
                             "DH_NETWORK_HALPERIN");
  return rc ? rc : create_halperin(cfg, m_up, m_dn, n_inter, out);
}

int dh_create_cf(const dh_config* cfg, const int* occ, int n_occ, dh_handle** out) {
  const int rc = check_entry(cfg && out && occ, cfg, "", "Jain", DH_NETWORK_JAIN, "dh_create_cf", "DH_NETWORK_JAIN");
  return rc ? rc : create_jain(cfg, occ, n_occ, out);
}
}  // extern "C"
