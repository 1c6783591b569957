// The estimator calls of the C ABI (include/deephall_amd.h) that take no handle: they see walkers
// and log psi values only.  Histograms, monopole orbitals, dh_swap_*, dh_rdm_*, dh_pair_*, dh_spin_*,
// dh_sf_*, the hole overlap matrix, the subspace matrices, and the impurity potential with its axis
// histogram.  Every check comes before any device call.
#include <algorithm>
#include <cmath>

#include "api_internal.h"

using namespace dh;

const char* dh::hole_gram_error(int B, int K) {
  if (B < 1) return "Holes: B < 1";
  if (K < 1 || K > DH_HOLE_MAX_CONFIGS) return "Holes: n_configs outside 1..DH_HOLE_MAX_CONFIGS";
  if ((int64_t)B * K > INT32_MAX) return "Holes: B n_configs >= 2^31";
  return nullptr;
}

extern "C" {

int dh_histograms(const float* x, int B, int nelec, int density_bins, int pair_bins, float* density, float* pair,
                  void* stream) {
  if (!x || B < 1 || nelec < 1 || density_bins < 0 || pair_bins < 0 || density_bins + pair_bins < 1 ||
      density_bins + pair_bins > 8192 || (density_bins && !density) || (pair_bins && !pair))
    return fail(DH_EINVAL, "bad arguments");
  launch_histograms(x, B, nelec, density_bins, pair_bins, density, pair, (hipStream_t)stream);
  return check_launch();
}

int dh_monopole_orbitals(const float* points, int n, int flux, float* out, void* stream) {
  if (!points || !out || n < 1 || flux < 0 || flux > 126) return fail(DH_EINVAL, "bad arguments");
  launch_monopole_orbitals(points, n, flux, out, (hipStream_t)stream);
  return check_launch();
}

// ---- Renyi-2 swap estimator (swap.hip): no handle, like the histograms ----

namespace {
// the checks the four swap calls share; thetas == nullptr: the call takes no angles
const char* swap_args_error(int B, int nelec, int n_up, int n_dn, const float* thetas, int A) {
  if (B < 2) return "swap: B < 2 (no pair)";
  if (nelec < 1 || n_up < 0 || n_dn < 0 || n_up + n_dn != nelec) return "swap: n_up + n_dn != nelec or nelec < 1";
  if (A < 1 || A > kSwapMaxAngles) return "swap: A outside 1..DH_SWAP_MAX_ANGLES";
  if ((int64_t)2 * A * (B / 2) > INT32_MAX) return "swap: 2 A (B / 2) >= 2^31";
  if (((int64_t)n_up + 1) * ((int64_t)n_dn + 1) > INT32_MAX / A) return "swap: A (n_up + 1)(n_dn + 1) >= 2^31";
  for (int a = 0; thetas && a < A; ++a)
    if (thetas[a] != thetas[a]) return "swap: a theta is NaN";
  return nullptr;
}
SwapThetas swap_thetas(const float* thetas, int A) {
  SwapThetas th{};
  for (int a = 0; a < A; ++a) th.t[a] = thetas[a];
  return th;
}
}  // namespace

size_t dh_swap_workspace_bytes(int B, int A) {
  if (swap_args_error(B, 1, 1, 0, nullptr, A)) return 0;
  return align64((size_t)A * (B / 2) * sizeof(int32_t));
}

int dh_swap_classify(const float* x, int B, int nelec, int n_up, int n_dn, const float* thetas, int A,
                     int32_t* sector, int32_t* counts, void* stream) {
  if (!x || !thetas || !sector || !counts) return fail(DH_EINVAL, "swap: null pointer");
  if (const char* e = swap_args_error(B, nelec, n_up, n_dn, thetas, A)) return fail(DH_EINVAL, e);
  launch_swap_classify(x, B, nelec, n_up, swap_thetas(thetas, A), A, sector, counts, (hipStream_t)stream);
  return check_launch();
}

int dh_swap_compact(const float* x, int B, int nelec, int n_up, int n_dn, const float* thetas, int A,
                    const int32_t* sector, int32_t* start, int32_t* pair, float* xs, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (!x || !thetas || !sector || !start || !pair || !xs || !workspace) return fail(DH_EINVAL, "swap: null pointer");
  if (const char* e = swap_args_error(B, nelec, n_up, n_dn, thetas, A)) return fail(DH_EINVAL, e);
  if (workspace_bytes < dh_swap_workspace_bytes(B, A)) return fail(DH_ENOMEM, "workspace too small");
  launch_swap_compact(x, B, nelec, n_up, swap_thetas(thetas, A), A, sector, (int32_t*)workspace, start, pair, xs,
                      (hipStream_t)stream);
  return check_launch();
}

int dh_swap_reduce(const float* logpsi, const float* logpsi_s, int B, int nelec, int n_up, int n_dn, int A, int M,
                   const int32_t* pair, const int32_t* sector, const int32_t* start, double* sums, void* stream) {
  if (!logpsi || !sector || !start || !sums || (M != 0 && (!logpsi_s || !pair)))
    return fail(DH_EINVAL, "swap: null pointer");
  if (const char* e = swap_args_error(B, nelec, n_up, n_dn, nullptr, A)) return fail(DH_EINVAL, e);
  if (M < 0 || (int64_t)M > (int64_t)A * (B / 2)) return fail(DH_EINVAL, "swap: M outside 0..A (B / 2)");
  launch_swap_reduce(logpsi, logpsi_s, B, (n_up + 1) * (n_dn + 1), A, M, pair, sector, start, sums,
                     (hipStream_t)stream);
  return check_launch();
}

// ---- Landau-level-resolved one-body density matrix (rdm.hip): no handle either ----

namespace {
const char* rdm_basis_error(int flux, int levels) {
  if (levels < 1 || levels > kRdmMaxLevels) return "rdm: levels outside 1..DH_RDM_MAX_LEVELS";
  if (flux < 0 || flux > 126) return "rdm: flux outside 0..126";
  return nullptr;
}
const char* rdm_size_error(int B, int nelec, int P) {
  if (B < 1 || P < 1) return "rdm: B < 1 or P < 1";
  if (nelec < 1 || nelec > 32) return "rdm: nelec outside 1..32";
  if ((int64_t)P * B > (int64_t)1 << 30) return "rdm: P B > 2^30";
  if ((int64_t)P * B * nelec * nelec > INT32_MAX) return "rdm: P B nelec^2 >= 2^31";
  return nullptr;
}
}  // namespace

int dh_rdm_norb(int flux, int levels) { return rdm_basis_error(flux, levels) ? 0 : rdm_norb(flux, levels); }

size_t dh_rdm_workspace_bytes(int B, int nelec, int flux, int levels, int P) {
  if (rdm_basis_error(flux, levels) || rdm_size_error(B, nelec, P)) return 0;
  return align64(rdm_workspace_bytes((int64_t)P * B, flux, levels));
}

int dh_monopole_harmonics(const float* points, int n, int flux, int levels, float* out, void* stream) {
  if (!points || !out) return fail(DH_EINVAL, "rdm: null pointer");
  if (const char* e = rdm_basis_error(flux, levels)) return fail(DH_EINVAL, e);
  if (n < 1 || (int64_t)n * (flux + 2 * levels - 1) > INT32_MAX) return fail(DH_EINVAL, "rdm: n < 1 or too large");
  const double* table = nullptr;
  HIP_TRY(rdm_table(flux, levels, &table));
  launch_monopole_harmonics(points, n, flux, levels, table, out, (hipStream_t)stream);
  return check_launch();
}

int dh_rdm_displace(const float* x, const float* r_prime, int B, int nelec, int P, float* xp, void* stream) {
  if (!x || !r_prime || !xp) return fail(DH_EINVAL, "rdm: null pointer");
  if (const char* e = rdm_size_error(B, nelec, P)) return fail(DH_EINVAL, e);
  launch_rdm_displace(x, r_prime, B, nelec, P, xp, (hipStream_t)stream);
  return check_launch();
}

int dh_rdm_accumulate(const float* x, const float* r_prime, const float* logpsi, const float* logpsi_p, int B,
                      int nelec, int n_up, int flux, int levels, int P, int by_spin, double* rho, int32_t* nvalid,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !r_prime || !logpsi || !logpsi_p || !rho || !nvalid || !workspace)
    return fail(DH_EINVAL, "rdm: null pointer");
  if (const char* e = rdm_basis_error(flux, levels)) return fail(DH_EINVAL, e);
  if (const char* e = rdm_size_error(B, nelec, P)) return fail(DH_EINVAL, e);
  if (n_up < 0 || n_up > nelec) return fail(DH_EINVAL, "rdm: n_up outside 0..nelec");
  if (workspace_bytes < dh_rdm_workspace_bytes(B, nelec, flux, levels, P))
    return fail(DH_EINVAL, "rdm: workspace smaller than dh_rdm_workspace_bytes");
  const double* table = nullptr;
  HIP_TRY(rdm_table(flux, levels, &table));
  HIP_TRY(launch_rdm_accumulate(x, r_prime, logpsi, logpsi_p, B, nelec, n_up, flux, levels, P, by_spin != 0, table,
                                rho, nvalid, workspace, (hipStream_t)stream));
  return check_launch();
}

// ---- pair amplitudes (pairamp.hip): no handle either ----

namespace {
const char* pair_size_error(int B, int nelec, int P) {
  if (B < 1 || P < 1) return "pair: B < 1 or P < 1";
  if (nelec < 1 || nelec > 32) return "pair: nelec outside 1..32";
  if ((int64_t)P * B > (int64_t)1 << 30) return "pair: P B > 2^30";
  if ((int64_t)P * B * std::max(1, nelec * (nelec - 1) / 2) > INT32_MAX)
    return "pair: P B nelec (nelec - 1) / 2 >= 2^31";
  return nullptr;
}
const char* pair_flux_error(int flux) {
  return flux < 0 || flux > kPairMaxFlux ? "pair: flux outside 0..126" : nullptr;
}
}  // namespace

size_t dh_pair_workspace_bytes(int B, int nelec, int flux, int P) {
  if (pair_size_error(B, nelec, P) || pair_flux_error(flux)) return 0;
  return align64(pair_workspace_bytes((int64_t)P * B, nelec, flux));
}

int dh_pair_displace(const float* x, const float* r1, const float* r2, int B, int nelec, int P, int pair0, int pair1,
                     float* xp, void* stream) {
  if (!x || !r1 || !r2 || !xp) return fail(DH_EINVAL, "pair: null pointer");
  if (const char* e = pair_size_error(B, nelec, P)) return fail(DH_EINVAL, e);
  if (pair0 < 0 || pair1 <= pair0 || pair1 > nelec * (nelec - 1) / 2)
    return fail(DH_EINVAL, "pair: need 0 <= pair0 < pair1 <= nelec (nelec - 1) / 2");
  launch_pair_displace(x, r1, r2, B, nelec, P, pair0, pair1, xp, (hipStream_t)stream);
  return check_launch();
}

int dh_pair_kernel(const float* points, int n, int flux, double* out, void* stream) {
  if (!points || !out) return fail(DH_EINVAL, "pair: null pointer");
  if (const char* e = pair_flux_error(flux)) return fail(DH_EINVAL, e);
  if (n < 1 || (int64_t)n * (flux + 1) > INT32_MAX) return fail(DH_EINVAL, "pair: n < 1 or n (flux + 1) >= 2^31");
  launch_pair_kernel(points, n, flux, out, (hipStream_t)stream);
  return check_launch();
}

int dh_pair_accumulate(const float* x, const float* r1, const float* r2, const float* logpsi, const float* logpsi_p,
                       int B, int nelec, int n_up, int flux, int P, double* A, int32_t* nvalid, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (!x || !r1 || !r2 || !logpsi || !logpsi_p || !A || !nvalid || !workspace)
    return fail(DH_EINVAL, "pair: null pointer");
  if (const char* e = pair_size_error(B, nelec, P)) return fail(DH_EINVAL, e);
  if (const char* e = pair_flux_error(flux)) return fail(DH_EINVAL, e);
  if (n_up < 0 || n_up > nelec) return fail(DH_EINVAL, "pair: n_up outside 0..nelec");
  if (workspace_bytes < dh_pair_workspace_bytes(B, nelec, flux, P))
    return fail(DH_EINVAL, "pair: workspace smaller than dh_pair_workspace_bytes");
  HIP_TRY(launch_pair_accumulate(x, r1, r2, logpsi, logpsi_p, B, nelec, n_up, flux, P, A, nvalid, workspace,
                                 (hipStream_t)stream));
  return check_launch();
}

// ---- total-spin estimator (spin.hip): no handle either ----

namespace {
const char* spin_size_error(int B, int n_up, int n_dn) {
  if (B < 1) return "spin: B < 1";
  if (n_up < 0 || n_dn < 0 || n_up + n_dn < 1 || n_up + n_dn > 32) return "spin: n_up, n_dn < 0 or n_up + n_dn outside 1..32";
  if ((int64_t)B * n_up * n_dn > INT32_MAX) return "spin: B n_up n_dn >= 2^31";
  return nullptr;
}
const char* spin_window_error(int n_up, int n_dn, int pair0, int pair1) {
  if (pair0 < 0 || pair1 <= pair0 || pair1 > n_up * n_dn) return "spin: need 0 <= pair0 < pair1 <= n_up n_dn";
  return nullptr;
}
}  // namespace

size_t dh_spin_workspace_bytes(int B, int n_up, int n_dn) {
  if (spin_size_error(B, n_up, n_dn)) return 0;
  return align64(spin_workspace_bytes(B, n_up * n_dn));
}

int dh_spin_exchange(const float* x, int B, int nelec, int n_up, int n_dn, int pair0, int pair1, float* xs,
                     void* stream) {
  if (!x || !xs) return fail(DH_EINVAL, "spin: null pointer");
  if (const char* e = spin_size_error(B, n_up, n_dn)) return fail(DH_EINVAL, e);
  if (n_up + n_dn != nelec) return fail(DH_EINVAL, "spin: n_up + n_dn != nelec");
  if (const char* e = spin_window_error(n_up, n_dn, pair0, pair1)) return fail(DH_EINVAL, e);
  launch_spin_exchange(x, B, nelec, n_up, n_dn, pair0, pair1, xs, (hipStream_t)stream);
  return check_launch();
}

int dh_spin_ratios(const float* logpsi, const float* logpsi_s, int B, int n_up, int n_dn, int pair0, int pair1,
                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!logpsi || !logpsi_s || !workspace) return fail(DH_EINVAL, "spin: null pointer");
  if (const char* e = spin_size_error(B, n_up, n_dn)) return fail(DH_EINVAL, e);
  if (const char* e = spin_window_error(n_up, n_dn, pair0, pair1)) return fail(DH_EINVAL, e);
  if (workspace_bytes < dh_spin_workspace_bytes(B, n_up, n_dn))
    return fail(DH_ENOMEM, "spin: workspace smaller than dh_spin_workspace_bytes");
  launch_spin_ratios(logpsi, logpsi_s, B, pair0, pair1, workspace, (hipStream_t)stream);
  return check_launch();
}

int dh_spin_reduce(const float* logpsi, int B, int n_up, int n_dn, void* workspace, size_t workspace_bytes,
                   double* s2, double* pairs, double* total, int32_t* nvalid, void* stream) {
  if (!logpsi || !workspace || !s2 || !total || !nvalid) return fail(DH_EINVAL, "spin: null pointer");
  if (const char* e = spin_size_error(B, n_up, n_dn)) return fail(DH_EINVAL, e);
  if (n_up * n_dn > 0 && !pairs) return fail(DH_EINVAL, "spin: null pointer");
  if (workspace_bytes < dh_spin_workspace_bytes(B, n_up, n_dn))
    return fail(DH_ENOMEM, "spin: workspace smaller than dh_spin_workspace_bytes");
  launch_spin_reduce(logpsi, B, n_up, n_dn, workspace, s2, pairs, total, nvalid, (hipStream_t)stream);
  return check_launch();
}

// ---- static structure factor (sfactor.hip) ----

namespace {
const char* sf_error(int B, int nelec, int n_up, int lmax) {
  if (B < 1) return "sf: B < 1";
  if (nelec < 1 || nelec > 32) return "sf: nelec outside 1..32";
  if ((int64_t)B * nelec > INT32_MAX) return "sf: B nelec >= 2^31";
  if (n_up < 0 || n_up > nelec) return "sf: n_up outside 0..nelec";
  if (lmax < 0 || lmax > kSfMaxL) return "sf: lmax outside 0..DH_SF_MAX_L";
  return nullptr;
}
}  // namespace

int dh_sf_nlm(int lmax) { return lmax < 0 || lmax > kSfMaxL ? -1 : sf_nlm(lmax); }

size_t dh_sf_workspace_bytes(int B, int nelec, int lmax) {
  if (sf_error(B, nelec, 0, lmax)) return 0;
  return align64(sf_workspace_bytes(B, lmax));
}

int dh_sf_pairs(const float* x, int B, int nelec, int n_up, int lmax, double* T, void* stream) {
  if (!x || !T) return fail(DH_EINVAL, "sf: null pointer");
  if (const char* e = sf_error(B, nelec, n_up, lmax)) return fail(DH_EINVAL, e);
  launch_sf_pairs(x, B, nelec, n_up, lmax, T, (hipStream_t)stream);
  return check_launch();
}

int dh_sf_multipoles(const float* x, int B, int nelec, int n_up, int lmax, double* rho, void* stream) {
  if (!x || !rho) return fail(DH_EINVAL, "sf: null pointer");
  if (const char* e = sf_error(B, nelec, n_up, lmax)) return fail(DH_EINVAL, e);
  launch_sf_multipoles(x, B, nelec, n_up, lmax, rho, (hipStream_t)stream);
  return check_launch();
}

int dh_sf_accumulate(const float* x, int B, int nelec, int n_up, int lmax, int want_multipoles, double* pair_sums,
                     double* rho_sums, int32_t* nvalid, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !pair_sums || !nvalid || !workspace || (want_multipoles && !rho_sums))
    return fail(DH_EINVAL, "sf: null pointer");
  if (const char* e = sf_error(B, nelec, n_up, lmax)) return fail(DH_EINVAL, e);
  if (workspace_bytes < dh_sf_workspace_bytes(B, nelec, lmax))
    return fail(DH_EINVAL, "sf: workspace smaller than dh_sf_workspace_bytes");
  launch_sf_accumulate(x, B, nelec, n_up, lmax, want_multipoles != 0, pair_sums, rho_sums, nvalid, workspace,
                       (hipStream_t)stream);
  return check_launch();
}

// ---- quasihole overlap matrix (holes.hip; dh_hole_table and dh_hole_logs: api_trial.cpp) ----

size_t dh_hole_workspace_bytes(int B, int n_configs) {
  if (hole_gram_error(B, n_configs)) return 0;
  return align64(hole_workspace_bytes(B, n_configs));
}

int dh_hole_gram(const double* L, int B, int n_configs, const double* shift, double* S, int32_t* nvalid,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!L || !shift || !S || !nvalid || !workspace) return fail(DH_EINVAL, "Holes: null pointer");
  if (const char* e = hole_gram_error(B, n_configs)) return fail(DH_EINVAL, e);
  if (workspace_bytes < dh_hole_workspace_bytes(B, n_configs))
    return fail(DH_ENOMEM, "Holes: workspace smaller than dh_hole_workspace_bytes");
  launch_hole_gram(L, B, n_configs, shift, S, nvalid, workspace, (hipStream_t)stream);
  return check_launch();
}

// ---- subspace matrices S, H, T of K states (subspace.hip): no handle either ----

namespace {
const char* subspace_error(int B, int K) {
  if (B < 1) return "subspace: B < 1";
  if (K < 1 || K > kSubspaceMaxStates) return "subspace: K outside 1..DH_SUBSPACE_MAX_STATES";
  if ((int64_t)B * K > INT32_MAX) return "subspace: K B >= 2^31";
  return nullptr;
}
}  // namespace

size_t dh_subspace_workspace_bytes(int B, int K) {
  if (subspace_error(B, K)) return 0;
  return align64(subspace_workspace_bytes(B, K));
}

int dh_subspace_accumulate(const float* logs, const float* e_l, const float* ke, int B, int K, const double* shift,
                           double* out, int32_t* nvalid, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logs || !e_l || !ke || !shift || !out || !nvalid || !workspace)
    return fail(DH_EINVAL, "subspace: null pointer");
  if (const char* e = subspace_error(B, K)) return fail(DH_EINVAL, e);
  if (workspace_bytes < dh_subspace_workspace_bytes(B, K))
    return fail(DH_EINVAL, "subspace: workspace smaller than dh_subspace_workspace_bytes");
  launch_subspace_accumulate(logs, e_l, ke, B, K, shift, out, nvalid, workspace, (hipStream_t)stream);
  return check_launch();
}

// ---- impurity potential and the density around an axis (impurity.hip) ----

namespace {
const double kPi = 3.14159265358979323846;
const char* impurity_error(const dh_impurity* imp, int n) {
  if (n < 0 || n > DH_MAX_IMPURITIES) return "impurity: n_imp outside 0..DH_MAX_IMPURITIES";
  if (n > 0 && !imp) return "impurity: null array";
  for (int a = 0; a < n; ++a) {
    const dh_impurity& m = imp[a];
    if (!std::isfinite(m.theta) || !std::isfinite(m.phi) || !std::isfinite(m.strength) || !std::isfinite(m.width))
      return "impurity: a field is not finite";
    if (!(m.width > 0.0)) return "impurity: width <= 0";
    if (m.kind != DH_IMPURITY_GAUSSIAN && m.kind != DH_IMPURITY_CHARGE) return "impurity: unknown kind";
    if (m.species != DH_HOLE_BOTH && m.species != DH_HOLE_UP && m.species != DH_HOLE_DOWN)
      return "impurity: unknown species";
    if (m.theta < 0.0 || m.theta > kPi) return "impurity: theta outside [0, pi]";
  }
  return nullptr;
}
const char* impurity_size_error(int B, int n_up, int n_dn) {
  if (B < 1) return "impurity: B < 1";
  if (n_up < 0 || n_dn < 0 || n_up > 32 || n_dn > 32 || n_up + n_dn < 1 || n_up + n_dn > 32)
    return "impurity: n_up, n_dn < 0 or n_up + n_dn outside 1..32";
  if ((int64_t)B * (n_up + n_dn) > INT32_MAX) return "impurity: B nelec >= 2^31";
  return nullptr;
}
}  // namespace

int dh_impurity_check(const dh_impurity* impurities, int n_imp) {
  if (const char* e = impurity_error(impurities, n_imp)) return fail(DH_EINVAL, e);
  return DH_OK;
}

int dh_external_potential(const float* x, int B, int n_up, int n_dn, double radius, const dh_impurity* impurities,
                          int n_imp, float* e_l, float* ext, void* stream) {
  if (!x || !ext) return fail(DH_EINVAL, "impurity: null pointer");
  if (const char* e = impurity_size_error(B, n_up, n_dn)) return fail(DH_EINVAL, e);
  if (!std::isfinite(radius) || !(radius > 0.0)) return fail(DH_EINVAL, "impurity: radius not finite or <= 0");
  if (const char* e = impurity_error(impurities, n_imp)) return fail(DH_EINVAL, e);
  ImpurityTable tab{};
  tab.n = n_imp;
  for (int a = 0; a < n_imp; ++a) {
    const dh_impurity& m = impurities[a];
    double v[3];
    impurity_vector(m.theta, m.phi, v);
    tab.ax[a] = v[0], tab.ay[a] = v[1], tab.az[a] = v[2];
    tab.strength[a] = m.strength;
    const bool g = m.kind == DH_IMPURITY_GAUSSIAN;
    tab.p[a] = g ? (radius / m.width) * (radius / m.width) : 2.0 * radius * radius;
    tab.q[a] = g ? 0.0 : m.width * m.width;
    tab.kind[a] = g ? kImpurityGaussian : kImpurityCharge;
    tab.species[a] = m.species;
  }
  launch_external_potential(x, B, n_up + n_dn, n_up, tab, e_l, ext, (hipStream_t)stream);
  return check_launch();
}

int dh_axis_histogram(const float* x, int B, int n_up, int n_dn, double axis_theta, double axis_phi, int bins,
                      unsigned* counts, void* stream) {
  if (!x || !counts) return fail(DH_EINVAL, "impurity: null pointer");
  if (const char* e = impurity_size_error(B, n_up, n_dn)) return fail(DH_EINVAL, e);
  if (!std::isfinite(axis_theta) || !std::isfinite(axis_phi)) return fail(DH_EINVAL, "impurity: axis not finite");
  if (axis_theta < 0.0 || axis_theta > kPi) return fail(DH_EINVAL, "impurity: axis_theta outside [0, pi]");
  if (bins < 1 || bins > 4096) return fail(DH_EINVAL, "impurity: bins outside 1..4096");
  launch_axis_histogram(x, B, n_up + n_dn, n_up, axis_theta, axis_phi, bins, counts, (hipStream_t)stream);
  return check_launch();
}

}  // extern "C"
