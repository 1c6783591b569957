// The structure-factor calls of the C ABI (include/deephall_amd.h): dh_sf_*.  No handle: like the
// histogram, swap, rdm and spin kernels they see walkers only.  Every check comes before any device call.
#include "api_internal.h"

using namespace dh;

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

extern "C" {

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

}  // extern "C"
