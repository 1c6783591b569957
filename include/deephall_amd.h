/*
 * deephall_amd.h — C ABI of the MI355X-native DeepHall VMC inner loop.
 *
 * The reference (peterzjx/DeepHall) has no FFI: its hot path is a set of Python
 * callables transformed by JAX.  This ABI is the native drop-in underneath the
 * Python mirror of those callables (deephall_amd/), one entry point per
 * reference interface:
 *
 *   dh_create / dh_set_params   <-> make_network(system, network)
 *                                   deephall/networks/__init__.py:22-37, and the
 *                                   parameter tree of model.init (train.py:62)
 *   dh_logpsi                   <-> Psiformer.__call__ / model.apply, vmapped
 *                                   deephall/networks/psiformer.py:72-76, train.py:69,84
 *   dh_mcmc_step                <-> make_mcmc_step(...)(params, data, key, width)
 *                                   deephall/mcmc.py:105-150 (mh_update 25-64,
 *                                   sph_sampling 67-102)
 *   dh_local_energy             <-> local_energy(f, system) vmapped
 *                                   deephall/hamiltonian.py:175-212 (+ make_local_kinetic_energy 83-172,
 *                                   make_potential 63-80), loss.py:51
 *   dh_energy_stats             <-> device-local statistics of loss_and_grad
 *                                   deephall/loss.py:30-38, 66-92 (before pmean)
 *   dh_init_walkers             <-> init_guess, deephall/train.py:40-54
 *
 * Conventions
 *   - Every pointer argument except `cfg`/`out`/`offsets` is a DEVICE pointer.
 *     Buffers (including the workspace) are owned by the caller; the library
 *     owns only the handle and the packed parameter copy made by dh_set_params.
 *   - Calls are asynchronous on `stream` (a hipStream_t; NULL = default stream).
 *     One handle per device; a handle is not thread-safe.
 *   - Return 0 on success, a negative DH_E* code on error; dh_last_error()
 *     returns a thread-local message.  No C++ exception crosses the ABI.
 *     NaN walkers propagate as NaN exactly as in the reference (loss.py uses
 *     nanmean; train.py:159 aborts on a NaN energy).
 *   - Walker coordinates: float32 [B][N][2] = (theta, phi), as the reference's
 *     data[B, N, 2] (train.py:53).
 */
#ifndef DEEPHALL_AMD_H
#define DEEPHALL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK 0
#define DH_EINVAL -1   /* bad argument / shape / unsupported config */
#define DH_EHIP -2     /* HIP runtime error */
#define DH_ENOMEM -3   /* workspace too small */
#define DH_ESTATE -4   /* parameters not set */

#define DH_INTERACTION_COULOMB 0
#define DH_INTERACTION_HARMONIC 1
#define DH_NETWORK_PSIFORMER 0
#define DH_NETWORK_LAUGHLIN 1 /* networks/laughlin.py: ground state, quasihole, quasiparticle (no parameters) */
#define DH_NETWORK_JAIN 2 /* Jain composite-fermion state, two Lambda levels (no parameters): dh_create builds the
                            filled-levels ground state N = 4 Q1 + 4, dh_create_cf any occupation */
#define DH_NETWORK_PFAFFIAN 3 /* Moore-Read Pfaffian state (no parameters): N even, p = cf_flux >= 1 and
                                flux = 2 p (N - 1) - 1 exactly (nu = 1/2 at p = 1); N <= 28 by the kernel's LDS */
#define DH_NETWORK_HALPERIN 4 /* Halperin (m_up, m_dn, n) two-component state (no parameters): dh_create_halperin
                                only; dh_create refuses the type, the exponents are not dh_config fields */
#define DH_NETWORK_QUASIHOLE 5 /* pinned quasiholes on a Halperin / Laughlin or a Moore-Read base (no parameters):
                                 dh_create_quasihole only; dh_create refuses the type */
#define DH_ORBITAL_FULL 0
#define DH_ORBITAL_SPARSE 1 /* blocks.py:52-62: 8 features per (j, k) mixed into the M harmonics by
                               lll_weight; folded into the full layout when parameters are set */

/* System + Network fields of deephall/config.py:56-104 that the hot path reads.
 * The first field is the caller's sizeof(dh_config): dh_create rejects any other
 * value with DH_EINVAL, so a binding written against an older (shorter) layout fails
 * loudly instead of letting the library read past the caller's struct.  Set it with
 * DH_CONFIG_INIT or `cfg.struct_size = sizeof(dh_config)`. */
typedef struct dh_config {
  uint32_t struct_size;       /* = sizeof(dh_config) = 60 bytes        */
  int n_up, n_dn;             /* System.nspins                          */
  int flux;                   /* System.flux = 2Q                       */
  float radius;               /* System.radius; <= 0 means sqrt(Q)      */
  float interaction_strength; /* System.interaction_strength            */
  int interaction_type;       /* DH_INTERACTION_*                       */
  int num_heads;              /* PsiformerNetwork.num_heads             */
  int heads_dim;              /* PsiformerNetwork.heads_dim             */
  int num_layers;             /* PsiformerNetwork.num_layers            */
  int ndets;                  /* PsiformerNetwork.determinants          */
  int orbital_type;           /* Network.orbital, DH_ORBITAL_*          */
  int network_type;           /* Network.type, DH_NETWORK_*             */
  float excitation_lz;        /* Laughlin: System.lz_center (networks/__init__.py:26) */
  int cf_flux;                /* Laughlin: composite-fermion flux p (laughlin.py:23), >= 1 */
} dh_config;
#define DH_CONFIG_INIT {sizeof(dh_config)}

typedef struct dh_handle dh_handle;

int dh_create(const dh_config* cfg, dh_handle** out);
/* Jain state (cfg->network_type = DH_NETWORK_JAIN) with an explicit occupation: occ holds
 * [n_occ][2] ints (Lambda level n in {0, 1}, 2 m), one determinant column each in this order;
 * Q1 = flux/2 - cf_flux (N - 1) >= 0, n_occ = N, 2 m of the parity of 2 Q1, |m| <= Q1 + n,
 * no orbital twice.  The handle has no parameters and serves dh_logpsi, dh_mcmc_step,
 * dh_local_energy, dh_potential and dh_energy_stats as a Laughlin handle does. */
int dh_create_cf(const dh_config* cfg, const int* occ, int n_occ, dh_handle** out);
/* Halperin state (cfg->network_type = DH_NETWORK_HALPERIN): with w_ik = u_i v_k - u_k v_i and the
 * slots below n_up up, the rest down,
 *   log psi = sum_{i<k} c_ik log w_ik,  c_ik = m_up (both up), m_dn (both down), n_inter (one of each),
 * no determinant, no normalisation, Im log psi the principal phase.  m_up and m_dn odd and >= 1,
 * n_inter >= 0, 1 <= N <= 32, 1 <= flux <= 126, flux = m_up (n_up - 1) + n_inter n_dn if n_up > 0
 * and flux = m_dn (n_dn - 1) + n_inter n_up if n_dn > 0 (the exponent of an empty or single-electron
 * species is bound by its parity only); anything else is DH_EINVAL with a message that starts
 * "Halperin".  The handle has no parameters and serves the calls a dh_create_cf handle serves. */
int dh_create_halperin(const dh_config* cfg, int m_up, int m_dn, int n_inter, dh_handle** out);

/* Pinned quasiholes (cfg->network_type = DH_NETWORK_QUASIHOLE).  Hole a at (theta_a, phi_a) has the
 * spinor (U_a, V_a) of an electron there and s_a(i) = u_i V_a - v_i U_a, zero with electron i on it.
 *   base DH_QUASIHOLE_HALPERIN: log psi = sum_{i<k} c_ik log w_ik + sum_a sum_{i in S_a} log s_a(i),
 *     c_ik as for dh_create_halperin; S_a all electrons (DH_HOLE_BOTH), the up slots (DH_HOLE_UP) or
 *     the down slots (DH_HOLE_DOWN); with h_up / h_dn holes acting on a species, a non-empty species
 *     needs flux = m_up (n_up - 1) + n_inter n_dn + h_up = m_dn (n_dn - 1) + n_inter n_up + h_dn.
 *     Laughlin 1/m: nspins (N, 0), exponents (m, any odd, 0).
 *   base DH_QUASIHOLE_PFAFFIAN: the holes of kind DH_HOLE_GROUP_A and DH_HOLE_GROUP_B (k of each),
 *     F_i = prod_{a in A} s_a(i), G_i = prod_{b in B} s_b(i), A_ik = (F_i G_k + F_k G_i) / w_ik,
 *     log psi = log Pf(A) + 2 p sum_{i<k} log w_ik + sum_{a of DH_HOLE_BOTH} sum_i log s_a(i),
 *     N even, flux = 2 p (N - 1) - 1 + k + (number of DH_HOLE_BOTH holes); N <= 28 by the kernel's LDS;
 *     k = 0 (DH_HOLE_BOTH holes only): A_ik = 1 / w_ik, Moore-Read's own entries.
 * No normalisation, Im log psi the principal phase.  1 <= n_holes <= DH_QUASIHOLE_MAX_HOLES, angles
 * finite, 0 <= theta <= pi, flux <= 126, N <= 32; anything else is DH_EINVAL with a message that
 * starts "Quasihole", before any launch.  The handle has no parameters and serves the calls a
 * dh_create_halperin handle serves. */
#define DH_QUASIHOLE_MAX_HOLES 8
#define DH_QUASIHOLE_HALPERIN 0
#define DH_QUASIHOLE_PFAFFIAN 1
#define DH_HOLE_BOTH 0
#define DH_HOLE_UP 1
#define DH_HOLE_DOWN 2
#define DH_HOLE_GROUP_A 3
#define DH_HOLE_GROUP_B 4
typedef struct dh_quasihole {
  uint32_t struct_size;                     /* = sizeof(dh_quasihole) = 192 bytes                  */
  int base;                                 /* DH_QUASIHOLE_HALPERIN or DH_QUASIHOLE_PFAFFIAN      */
  int m_up, m_dn, n_inter;                  /* Halperin base: the exponents                        */
  int p;                                    /* Pfaffian base: 2 p vortices per electron            */
  int n_holes;
  int kind[DH_QUASIHOLE_MAX_HOLES];         /* DH_HOLE_* of hole a                                 */
  double holes[DH_QUASIHOLE_MAX_HOLES][2];  /* (theta, phi) of hole a                              */
} dh_quasihole;
int dh_create_quasihole(const dh_config* cfg, const dh_quasihole* q, dh_handle** out);
void dh_destroy(dh_handle* h);
const char* dh_last_error(void);
const char* dh_version(void);

/* Packed parameter layout.  Segment s starts at float offset
 * offsets[s] of the packed buffer (each segment 64-float aligned); segment
 * order:
 *   0                  W0        [4][D]           PsiformerLayers_0/Dense_0/kernel
 *   per layer l (8 segments, base 1+8l):
 *     +0 Wqkv [D][3D]  query|key|value kernels, columns (h, d) per block
 *     +1 bqkv [3D]
 *     +2 Wol  [D][D]   out/kernel (as [H*dh][D]) @ Dense_{2l+1}/kernel  (folded)
 *     +3 bol  [D]      out/bias @ Dense_{2l+1}/kernel
 *     +4 ln1  [2][D]   LayerNorm_{2l}: scale, bias
 *     +5 Wm   [D][D]   Dense_{2l+2}/kernel
 *     +6 bm   [D]      Dense_{2l+2}/bias
 *     +7 ln2  [2][D]   LayerNorm_{2l+1}: scale, bias
 *   1+8L     Worb [D][ld_orb]  columns ((blk*2+part)*M + m)*N*K + j*K + k,
 *                              blk = spin block, part 0 = real / 1 = imag,
 *                              zero padded to ld_orb (multiple of 128)
 *   2+8L     borb [ld_orb]
 *   3+8L     jastrow [2]       ee_par, ee_anti
 *   4+8L     W0qkv [4][3D]     W0 @ Wqkv of layer 0: the first attention projection
 *                              folded into the K=4 input map (unused if L == 0)
 * Returns the number of segments (5+8L) and writes up to `n` offsets; the
 * total float count is offsets[nseg] (written if n > nseg). */
int dh_param_layout(const dh_handle* h, size_t* offsets, int n);
/* Copy the packed parameter buffer (device pointer, `count` floats) into the
 * handle.  `count` must equal the total from dh_param_layout. */
int dh_set_params(dh_handle* h, const float* params, size_t count, void* stream);

/* Reference parameter tree, flattened (SURVEY.md Appendix B names, Flax order):
 *   0                 PsiformerLayers_0/Dense_0/kernel [4][D]
 *   per layer l (15 segments, base 1+15l):
 *     MultiHeadAttention_l/{query,key,value}/{kernel [D][H*dh], bias [H*dh]}  (+0..+5)
 *     MultiHeadAttention_l/out/{kernel [H*dh][D], bias [D]}                   (+6, +7)
 *     Dense_{2l+1}/kernel [D][D]; LayerNorm_{2l}/{scale, bias} [D]             (+8..+10)
 *     Dense_{2l+2}/{kernel [D][D], bias [D]}; LayerNorm_{2l+1}/{scale, bias}   (+11..+14)
 *   1+15L+2i, +1      Orbitals_0/featured_orbitals/DenseGeneral_i/{kernel [D][F*N*K],
 *                     bias [F*N*K]}, i < 2 * (spin blocks); F = M ("full") or 8 ("sparse")
 *   "sparse" only:    Orbitals_0/lll_weight/{kernel [8][M], bias [M]}
 *   then              Jastrow_0/ee_par [1], Jastrow_0/ee_anti [1]
 * Segments are 64-float aligned.  Returns the segment count; offsets[nseg] = total floats.
 * Parameter gradients (dh_logpsi_vjp) use the same layout. */
int dh_ref_layout(const dh_handle* h, size_t* offsets, int n);
/* Upload the reference tree (device pointer, `count` = total floats of dh_ref_layout) and
 * pack it on the device: concatenations, zero padding, and the folds Wo Wl, bo Wl,
 * W0 Wqkv (double-accumulated), transposed / split-bf16 copies.  Replaces the host
 * packing of dh_set_params; required by dh_logpsi_vjp. */
int dh_set_params_ref(dh_handle* h, const float* ref, size_t count, void* stream);

/* Parameter gradient by reverse mode (loss.py:53-64, 93-108 with jax.grad of the network):
 *   grad = sum_b ct[b][0] d Re log psi_b / dp + ct[b][1] d Im log psi_b / dp
 * ct [B][2] per-walker cotangents (dh_grad_cotangent), grad [dh_ref_layout total] f32,
 * logpsi [B][2] optional (NULL) log psi of the walkers from the same forward pass.
 * Processes walkers in chunks sized to the workspace (dh_vjp_workspace_bytes per chunk). */
size_t dh_vjp_workspace_bytes(const dh_handle* h, int batch);
int dh_logpsi_vjp(dh_handle* h, const float* x, int B, const float* ct, float* grad, float* logpsi, void* ws,
                  size_t ws_bytes, void* stream);
/* KFAC — the reference's default optimizer (deephall/optimizers/kfac.py:195-241, kfac_jax
 * Optimizer with "fisher_exact" curvature, repeated-dense Kronecker blocks, pi-adjusted
 * damping, norm constraint; restated in oracle/kfac.py).  Orbital "full" only.
 *
 * dh_kfac_layout: describes the curvature statistics buffer; returns the number of size_t
 *   values, writes up to n of them: [0] statistics floats, [1] factor-matrix floats,
 *   [2] factor slots S, [3] dense blocks nb, [4] generic (diagonal) floats, [5] dh_kfac_step
 *   workspace bytes, then per block (kernel segment, bias segment or SIZE_MAX, d_in, d_out,
 *   A slot, G slot, 1000 x fixed scale), then per slot (n, float offset).
 * dh_kfac_vjp: one forward pass over x [B][N][2] with saved activations, then
 *   (ct != NULL) the gradient of dh_logpsi_vjp into grad, and the Fisher reverse pass
 *   (cotangent sqrt(2) on Re log psi; 0 for a walker with non-finite log psi) whose layer
 *   Gram matrices A = x~^T x~ / rows, G = dy^T dy / rows and generic diagonal
 *   (sum_b tangent)^2 / B are WRITTEN to stats (this device's batch; average over devices
 *   before dh_kfac_step).  logpsi [B][2] optional.  Workspace per chunk:
 *   dh_kfac_workspace_bytes.
 * dh_kfac_step: raw = ema * raw + stats (stats may be NULL: no EMA update), then with the
 *   EMA weight `weight` (sum of ema^k): damped inverses, P g into pgrad (dh_ref_layout
 *   floats), info[0] = <P g, g>, info[1] = c = min(1, sqrt(norm_constraint / (lr^2 <P g, g>))),
 *   info[2] = lr c (device doubles), and params -= lr c P g when params != NULL. */
int dh_kfac_layout(dh_handle* h, size_t* out, int n);
size_t dh_kfac_workspace_bytes(const dh_handle* h, int batch);
int dh_kfac_vjp(dh_handle* h, const float* x, int B, const float* ct, float* grad, float* stats, float* logpsi,
                void* ws, size_t ws_bytes, void* stream);
int dh_kfac_step(dh_handle* h, float* raw, const float* stats, float ema, float weight, const float* grad,
                 float* params, float lr, float damping, float norm_constraint, float* pgrad, double* info, void* ws,
                 size_t ws_bytes, void* stream);

/* MinSR — stochastic reconfiguration solved in sample space (B x B instead of P x P):
 *   delta = O~^T (O~ O~^T + lambda I)^-1 eps~.   The library supplies the Gram matrix O O^T of the
 * per-walker gradients; the centring, the solve and the update are the caller's (optimizers.py),
 * and O~^T y is dh_logpsi_vjp with y as cotangents.  Psiformer, orbital "full", N <= 32 only.
 *
 * dh_ntk: with g_b = ct[b][0] d Re log psi_b / dp + ct[b][1] d Im log psi_b / dp over the
 *   dh_ref_layout parameters (the reference tree: Wo, bo and Wl apart, not the kernels' folded
 *   Wo Wl), T[b][b'] = <g_b, g_b'>, float32 [B][B], WRITTEN.  x, ct, logpsi as dh_logpsi_vjp.
 *   The B x P Jacobian is never formed: every dense map adds sum_{t in b, t' in b'}
 *   (x_t . x_t' + 1) (dy_t . dy_t') over the walkers' electron rows (exact-f32 MFMA, ntk.hip);
 *   the LayerNorm and Jastrow parameters add J J^T of their explicit per-walker tangents.
 *   T is exactly symmetric (the upper triangle is computed and mirrored) and two calls give
 *   bit-identical results (no atomics).  A walker whose log psi is not finite, or whose ct is
 *   zero, gets an exactly zero row and column.
 *   ONE chunk: pairs of walkers from two chunks would need both chunks' activations, so
 *   ws_bytes < dh_ntk_workspace_bytes(h, B) is DH_ENOMEM (checked, with every other argument,
 *   before any device call); "sparse" orbitals and Laughlin handles are DH_EINVAL.
 * dh_ntk_tile_walkers: walkers per Gram tile (host only; tile_walkers * N <= 128 rows, a
 *   workgroup owns one pair of tiles); 0 for a handle dh_ntk does not serve.
 * The launches are not recorded by dh_profile_* (no kernel class is theirs).
 *
 * Across ranks every rank holds all B walkers and computes a share of T:
 * dh_ntk_part: dh_ntk's arguments and checks, then DH_EINVAL unless 0 <= part < nparts (all
 *   before any device call).  T is cleared and only the entries T[b][b'], b <= b', with
 *   dh_ntk_owner(h, b, nparts) == part are accumulated; no mirror.  The forward pass, the
 *   centring and logpsi cover all B walkers, identically for every part.  The parts have
 *   disjoint support, so their sum in any order (an all-reduce) followed by dh_ntk_mirror is
 *   dh_ntk's T bit for bit; dh_ntk is part 0 of 1 and the mirror.  Workspace as dh_ntk.
 * dh_ntk_mirror: T[b'][b] = T[b][b'] for b < b', T float32 [B][B] on the device.
 * dh_ntk_owner: (walker / dh_ntk_tile_walkers(h)) % nparts (host only): the part that owns row
 *   `walker` of T — a property of the row, not of a launch's tile size, so that all additions to
 *   an entry happen on one rank in one order.  -1 for a handle dh_ntk rejects, walker < 0 or
 *   nparts < 1.  Rows are dealt out cyclically by tile: the first and the last part's share of
 *   the upper triangle differ by about 2 (nparts - 1) / (number of tiles), relative.
 *
 * dh_minsr_matrix: the matrix MinSR solves, from T float32 [M][M] symmetric, M = 2 Bg, rows
 *   (a, i) = a Bg + i over the halves a (Re | Im) and walkers i, and valid [Bg] (bytes, nonzero =
 *   the walker takes part; n = max(1, their number)):
 *     r[a,i][c] = sum_j v_j T[(a,i),(c,j)] / n,   g[a][c] = sum_i v_i r[a,i][c] / n,
 *     A[(a,i),(c,j)] = v_i v_j (T - r[a,i][c] - r[c,j][a] + g[a][c]) / n + damping [(a,i) == (c,j)]
 *   A float64 [M][M], WRITTEN once; T is read twice (row sums in double in a fixed order, then
 *   the assembly); no atomics: two calls give identical bits; A is exactly symmetric; an invalid
 *   walker's rows and columns are 0 with damping on the diagonal.  ws: 8-byte aligned device
 *   memory of dh_minsr_matrix_workspace_bytes(Bg); a null pointer is DH_EINVAL, a short workspace
 *   DH_ENOMEM, both before any device call.
 *
 * dh_ntk_jvp: the per-walker Jacobian-vector product jv[b] = <g_b, v>, float32 [B], WRITTEN, for
 *   a parameter direction v (float32, dh_ref_layout, device), in the same forward pass and
 *   reverse walk as dh_ntk_part and with its arguments: every dense map adds
 *   sum_{t in b} (x_t V + v_b) . dy_t for its slices V, v_b of v (exact-f32 MFMA on the
 *   batch-mean-centred rows, ntk.hip), the LayerNorm and Jastrow parameters their explicit rows'
 *   dot products.  T non-null: exactly what dh_ntk_part(part, nparts) writes (not mirrored).
 *   T null: no Gram products (needs part 0 of 1, else DH_EINVAL).  jv is complete for every
 *   walker on every part and does not depend on T or the part; no atomics, two calls give
 *   identical bits, and a power-of-two multiple of v gives that multiple of jv bit for bit.  A
 *   walker whose log psi is not finite, or whose ct is zero, gets jv = 0 exactly.  Handles and
 *   states refused as by dh_ntk; a null v or jv is DH_EINVAL; ws_bytes <
 *   dh_ntk_jvp_workspace_bytes(h, B) (>= dh_ntk_workspace_bytes) is DH_ENOMEM; every check
 *   precedes the first device call. */
size_t dh_ntk_jvp_workspace_bytes(const dh_handle* h, int batch);
int dh_ntk_jvp(dh_handle* h, const float* x, int B, const float* ct, const float* v, float* T, float* jv,
               float* logpsi, void* ws, size_t ws_bytes, int part, int nparts, void* stream);
size_t dh_ntk_workspace_bytes(const dh_handle* h, int batch);
int dh_ntk_tile_walkers(const dh_handle* h);
int dh_ntk(dh_handle* h, const float* x, int B, const float* ct, float* T, float* logpsi, void* ws, size_t ws_bytes,
           void* stream);
int dh_ntk_part(dh_handle* h, const float* x, int B, const float* ct, float* T, float* logpsi, void* ws,
                size_t ws_bytes, int part, int nparts, void* stream);
int dh_ntk_mirror(float* T, int B, void* stream);
int dh_ntk_owner(const dh_handle* h, int walker, int nparts);
size_t dh_minsr_matrix_workspace_bytes(int Bg);
int dh_minsr_matrix(const float* T, const unsigned char* valid, int Bg, double damping, double* A, void* ws,
                    size_t ws_bytes, void* stream);

/* Cotangents of the gradient estimator 2 nanmean(conj(d log psi) diff) (loss.py:59-64):
 * part 0 (its real part, ENERGY_GRAD): ct = 2 (Re diff, Im diff) / n;
 * part 1 (its imaginary part, SR_F_VECTOR): ct = 2 (Im diff, -Re diff) / n;
 * n = nvalid[0] (device), NaN diffs give 0. */
int dh_grad_cotangent(const float* diff, const float* nvalid, int B, int part, float* ct, void* stream);
/* optax.adam step in place (optimizers/adam.py:24-43): b1, b2, eps as optax, lr = the
 * schedule value at `step` (config.py:125-137), bias correction with step + 1; NaN
 * gradients count as 0 (loss.py:64 nan_to_num). */
int dh_adam_update(float* params, const float* grad, float* mu, float* nu, size_t n, float lr, float b1, float b2,
                   float eps, int step, void* stream);

/* GEMM arithmetic of the local-energy (2N+5 channel) pass:
 *   DH_GEMM_F32   exact-f32 MFMA (v_mfma_f32_32x32x2_f32), f32 rounding per product;
 *   DH_GEMM_X6    split-bf16 MFMA: each f32 operand split exactly into three bf16 terms,
 *                 six bf16 products per pair (dropped terms <= 2^-24 |ab|, f32 accumulate);
 *                 error at the level of the f32 GEMM (tests/test_gpu_kernels.py), 2.67x the
 *                 f32 matrix rate.
 *   DH_GEMM_X6_ALL  split-bf16 also for the log-psi / MCMC GEMMs (the two per layer that
 *                 carry a LayerNorm with it in their epilogue).  Default.
 *   DH_GEMM_X6_ALL_UNFUSED  as DH_GEMM_X6_ALL, but the local energy's channel LayerNorms run
 *                 as separate passes after their GEMMs instead of inside them (test hook for
 *                 the fused gemm_lnch kernel; same arithmetic up to f32 summation order).
 * In DH_GEMM_F32 and DH_GEMM_X6 the log-psi / MCMC passes use the exact-f32 kernels. */
#define DH_GEMM_F32 0
#define DH_GEMM_X6 1
#define DH_GEMM_X6_ALL 2
#define DH_GEMM_X6_ALL_UNFUSED 3
int dh_set_gemm_mode(dh_handle* h, int mode);

/* Workspace bytes needed to process `batch` walkers: op 0 = log psi / MCMC,
 * op 1 = local energy.  Local energy processes walkers in chunks sized to the
 * workspace it is given (at least one walker). */
size_t dh_workspace_bytes(const dh_handle* h, int batch, int op);

/* log psi for B walkers: logpsi[B][2] = (Re, Im), Im the principal phase. */
int dh_logpsi(dh_handle* h, const float* x, int B, float* logpsi, void* ws, size_t ws_bytes, void* stream);

/* `steps` Metropolis-Hastings all-electron moves on B walkers, in place.
 *   x       [B][N][2]  walkers, updated in place (the reference donates data)
 *   lp      [B]        work/out: 2 Re log psi of the current walkers (computed
 *                      here at entry, mcmc.py:142)
 *   n_accept[B] int32  out: accepted moves per walker in this call
 *   width              proposal width (MCMC.width, mcmc.py:69-70)
 *   seed, counter      counter-based RNG (Philox4x32-10): the draw for walker g
 *                      (global index = walker_offset + b), step s uses counter
 *                      (g, counter + s, electron, 0) under key seed; results do
 *                      not depend on how walkers are sharded over devices
 *   noise              NULL, or injected noise [steps][B][2N+1] floats:
 *                      normals [N], phi uniforms in [0,1) [N], accept uniform [1]
 */
int dh_mcmc_step(dh_handle* h, float* x, float* lp, int32_t* n_accept, int B, int steps, float width,
                 uint64_t seed, uint64_t counter, int64_t walker_offset, const float* noise, void* ws,
                 size_t ws_bytes, void* stream);

/* Local energy for B walkers.
 *   e_l [B][2]   E_L = KE + lambda * PE (complex)
 *   obs [B][8]   KE re, KE im, PE (already times interaction_strength),
 *                Lz, Lz^2, L^2, logpsi re, logpsi im                         */
int dh_local_energy(dh_handle* h, const float* x, int B, float* e_l, float* obs, void* ws, size_t ws_bytes,
                    void* stream);

/* Device-local energy statistics (loss.py:66-92 before the pmean).  Writes
 * out[DH_NSTATS] floats: see DH_STAT_* indices.  Any B >= 1 (quantiles by a radix
 * select, no sort).  penalties != 0 also computes the clipped Lz^2, Lz, L^2 means that
 * System.lz_penalty / l2_penalty need (loss.py:76-88); else those entries are 0. */
#define DH_NSTATS 16
#define DH_STAT_ENERGY_RE 0    /* nanmean Re E_L                     */
#define DH_STAT_ENERGY_IM 1    /* nanmean Im E_L                     */
#define DH_STAT_CLIPPED_RE 2   /* nanmean Re iqr_clip(E_L)           */
#define DH_STAT_CLIPPED_IM 3   /* nanmean Im iqr_clip(E_L)           */
#define DH_STAT_ERE2 4         /* nanmean (Re E_L)^2                 */
#define DH_STAT_KINETIC_RE 5   /* mean KE re                         */
#define DH_STAT_KINETIC_IM 6   /* mean KE im                         */
#define DH_STAT_POTENTIAL 7    /* mean PE                            */
#define DH_STAT_LZ 8           /* mean Lz                            */
#define DH_STAT_LZ2 9          /* mean Lz^2                          */
#define DH_STAT_L2 10          /* mean L^2                           */
#define DH_STAT_PMOVE 11       /* sum n_accept / (steps * B)         */
#define DH_STAT_NVALID 12      /* number of non-NaN E_L              */
#define DH_STAT_CLIPPED_LZ2 13 /* nanmean iqr_clip(Lz^2)  (penalties) */
#define DH_STAT_CLIPPED_LZ 14  /* nanmean iqr_clip(Lz)    (penalties) */
#define DH_STAT_CLIPPED_L2 15  /* nanmean iqr_clip(L^2)   (penalties) */
/* h may be NULL (E_L of a log-psi callable evaluated outside the library). */
int dh_energy_stats(dh_handle* h, const float* e_l, const float* obs, const int32_t* n_accept, int B, int steps,
                    int penalties, float* out, void* stream);

/* The clipped energy difference that weights the parameter gradient (loss.py:75-89):
 *   d = E_L - <E_L>_clip + lz_penalty ((Lz^2 - <Lz^2>_clip) - 2 lz_center (Lz - <Lz>_clip))
 *         + l2_penalty (L^2 - <L^2>_clip),    diff = iqr_clip(d)  (local quantiles)
 * with the <.>_clip means read from `stats` (device, DH_STAT_* layout, already averaged
 * over devices).  diff[B][2] (re, im; NaN where E_L is NaN); nvalid[1] = number of
 * walkers with a non-NaN diff (the nanmean count of loss.py:64).  h may be NULL. */
int dh_loss_diff(dh_handle* h, const float* e_l, const float* obs, int B, const float* stats, float lz_penalty,
                 float lz_center, float l2_penalty, float* diff, float* nvalid, void* stream);

/* Fidelity of psi with a trial state phi on walkers drawn from |psi|^2 (pretraining; not in the
 * reference).  d_b = logphi[b] - logpsi[b] (complex, inputs float32 [B][2] = (Re, Im)); a walker
 * is valid when its four floats are finite.
 * dh_fidelity_partial writes part[DH_NFID] doubles (device):
 *   m = max Re d over the valid walkers (-inf: none), S = sum_b z_b with z_b = e^{d_b - m}
 *   (re, im), S2 = sum_b |z_b|^2 = sum_b e^{2 (Re d_b - m)}, n = the number of valid walkers.
 *   Partials of shards combine with M = max m_r, S = sum S_r e^{m_r - M},
 *   S2 = sum S2_r e^{2 (m_r - M)}, n = sum n_r (shards with n_r = 0 skipped);
 *   F = |S|^2 / (n S2) estimates |<phi|psi>|^2 / (<phi|phi> <psi|psi>).
 * dh_fidelity_residual writes resid[B][2] = 1 - n z_b / S (complex division) from such a
 *   (combined) total: the weights eps_b of d(-log F)/dp = 2 Re mean(conj(d log psi_b / dp) eps_b).
 *   NaN for an invalid walker; all NaN when n = 0 or S = 0 (|S|^2 = 0 in double).
 * Double arithmetic from the subtraction on; Im d is folded into [-pi, pi] before sin / cos.
 * One workgroup reduces in a fixed order, no atomics: two calls give identical bits.  A single
 * valid walker gives F = 1 and resid = 0 exactly.  Any B >= 1; B < 1 or a null pointer is
 * DH_EINVAL before any device call. */
#define DH_NFID 5
#define DH_FID_M 0     /* max Re d over the valid walkers */
#define DH_FID_S_RE 1  /* Re sum e^{d - m}                */
#define DH_FID_S_IM 2  /* Im sum e^{d - m}                */
#define DH_FID_S2 3    /* sum e^{2 (Re d - m)}            */
#define DH_FID_N 4     /* number of valid walkers         */
int dh_fidelity_partial(const float* logpsi, const float* logphi, int B, double* part, void* stream);
int dh_fidelity_residual(const float* logpsi, const float* logphi, int B, const double* total, float* resid,
                         void* stream);

/* Overlap penalty against K frozen lower states phi_k (excited-state training; not in the
 * reference).  logpsi [B][2], logphi [K][B][2] float32 (device); the rules are dh_fidelity_*'s,
 * per state: walker b is valid for state k when its four floats there are finite, the shift is
 * m_k = max Re d_k over those walkers, the sums run in one fixed order with no atomics.
 * dh_ortho_partial writes part[K][DH_NFID] doubles in one launch, one workgroup per state; row k
 *   is bit for bit dh_fidelity_partial(logpsi, logphi[k]).  Rows of shards combine as that
 *   call's partials do, state by state.
 * dh_ortho_residual writes out[B][2] = (e_l ? e_l[b] : 0) - sum_k weight[k] (1 - n_k z_kb / S_k)
 *   from the (combined) totals total[K][DH_NFID] and weight[K] doubles (device; lambda_k F_k):
 *   double arithmetic, k ascending, the quotient as dh_fidelity_residual forms it, each product
 *   weight[k] eps_kb rounded before it is subtracted, the result rounded once to float32.  A
 *   walker invalid for any k is NaN; any k with n_k = 0, S_k = 0 or a non-finite weight makes
 *   every output NaN.  With K = 1, weight 1 and e_l NULL the output is minus dh_fidelity_residual's;
 *   with every weight 0 and every walker valid it is e_l.
 * K outside 1 .. DH_ORTHO_MAX_STATES, B < 1 or a null pointer (e_l excepted) is DH_EINVAL before
 * any device call. */
#define DH_ORTHO_MAX_STATES 16
int dh_ortho_partial(const float* logpsi, const float* logphi, int B, int K, double* part, void* stream);
int dh_ortho_residual(const float* logpsi, const float* logphi, int B, int K, const double* total,
                      const double* weight, const float* e_l, float* out, void* stream);

/* Potential energy only (make_potential, hamiltonian.py:63-80), NOT multiplied by
 * interaction_strength: pe[B]. */
int dh_potential(dh_handle* h, const float* x, int B, float* pe, void* stream);

/* ---- NetObs-style estimators (deephall/netobs_bridge/observables/NAME.py) ----------------
 * dh_histograms ADDS to density[density_bins] the counts of every electron's theta and
 * to pair[pair_bins] the 1/sin(theta_12)-weighted counts of every pair angle
 * theta_12 = arccos(r_i . r_j), i < j, both over [0, pi] with numpy's bin rule
 * (density.py:38-44, pair_corr.py:43-58; the caller applies pair_corr.py:57's scale).
 * Either count may be 0 (its pointer then unused).  Walkers x[B][nelec][2]. */
int dh_histograms(const float* x, int B, int nelec, int density_bins, int pair_bins, float* density, float* pair,
                  void* stream);
/* Lowest-Landau-level monopole harmonics Y_{Q,Q,m}, m = -Q..Q, Q = flux / 2, at n points
 * (theta, phi): out[n][flux + 1] complex (re, im), one_rdm.py:31-54 (cos theta clipped to
 * +-(1 - 1e-4) as there). */
int dh_monopole_orbitals(const float* points, int n, int flux, float* out, void* stream);

/* ---- Renyi-2 entanglement entropy of a spherical cap: the swap estimator ------------------
 * Walkers x[B][nelec][2] (theta, phi); the slots below n_up are up electrons (n_up + n_dn =
 * nelec).  P = B / 2 pairs: pair p is (R1, R2) = (walker p, walker p + P), an odd last walker
 * is ignored.  Region a of A is the cap theta < thetas[a]; thetas is a HOST array (it is
 * checked and passed by value), 1 <= A <= DH_SWAP_MAX_ANGLES.  "In the cap" is the float32
 * comparison on the stored theta.  A pair is matched at angle a when the up count and the down
 * count in the cap agree between R1 and R2; its sector is k = nA_up (n_dn + 1) + nA_dn,
 * K = (n_up + 1)(n_dn + 1) sectors.  For a matched pair R1' is R1 with the coordinates of its
 * in-cap slots, in ascending slot order within each spin, replaced by R2's in-cap coordinates
 * in ascending slot order, and R2' the mirror image (copies of the stored floats).
 *
 * dh_swap_classify  sector[A][P] = the pair's sector, -1 when unmatched; ADDS to counts[A][K]
 *                   the sector of each of the 2 P members (matched or not): their sum grows by
 *                   2 P per angle.
 * dh_swap_compact   from sector: the matched pairs in (a-major, then p) order get the rows
 *                   o = 0..M-1; start[A + 1] = the first row of every angle and start[A] = M (the
 *                   device int the caller reads); pair[o] = a P + p; xs[2 o] = R1' and
 *                   xs[2 o + 1] = R2', each [nelec][2].  pair holds A P ints and xs 2 A P rows (the
 *                   case of every pair matched); only the first M / 2 M are written.  The rows are
 *                   handed out by a prefix sum, not an atomic counter: the same on every call.
 *                   workspace: dh_swap_workspace_bytes(B, A) device bytes.
 * dh_swap_reduce    sums[A][K][2] (re, im; double) = the sum over the matched pairs of angle a in
 *                   sector k of exp(logpsi_s[2 o] + logpsi_s[2 o + 1] - logpsi[p] - logpsi[p + P]),
 *                   with logpsi[B][2] of x and logpsi_s[2 M][2] of the first 2 M rows of xs as
 *                   dh_logpsi writes them, and M as read from start[A] (0 <= M <= A P; with
 *                   M = 0 logpsi_s and pair are not read and may be null).  Double arithmetic from
 *                   the float32 logs on, a fixed summation order, no float atomics: two calls give
 *                   identical bits.  An (a, k) without a matched pair gets zeros.
 *                   Tr rho_A^2 = sum_k sums[a][k] / P.
 * Each call checks its arguments before any device call: a null pointer, B < 2, nelec < 1,
 * n_up < 0, n_dn < 0, n_up + n_dn != nelec, A out of range, a NaN theta or 2 A P >= 2^31 is
 * DH_EINVAL (dh_swap_workspace_bytes then returns 0).  No dh_handle: like the histogram
 * kernels these know nothing of the network. */
#define DH_SWAP_MAX_ANGLES 64
int dh_swap_classify(const float* x, int B, int nelec, int n_up, int n_dn, const float* thetas, int A,
                     int32_t* sector, int32_t* counts, void* stream);
int dh_swap_compact(const float* x, int B, int nelec, int n_up, int n_dn, const float* thetas, int A,
                    const int32_t* sector, int32_t* start, int32_t* pair, float* xs, void* workspace,
                    size_t workspace_bytes, void* stream);
int dh_swap_reduce(const float* logpsi, const float* logpsi_s, int B, int nelec, int n_up, int n_dn, int A, int M,
                   const int32_t* pair, const int32_t* sector, const int32_t* start, double* sums, void* stream);
size_t dh_swap_workspace_bytes(int B, int A);

/* ---- Landau-level-resolved one-body density matrix -----------------------------------------
 * Basis: the monopole harmonics Y_{Q,Q+n,m}, Q = flux / 2, of the Landau levels n = 0..levels-1,
 * m = -(Q + n)..(Q + n); level-major, m ascending inside a level:
 * norb = dh_rdm_norb(flux, levels) = levels (flux + 1) + levels (levels - 1).  The general-l
 * formula of one_rdm.py:31-51 (the reference calls it with l = Q only), cos theta clipped to
 * +-(1 - 1e-4) as there; double arithmetic.  The per-orbital constants are computed on the host,
 * once per (device, flux, levels), and stay in a device table for the life of the process.
 *
 * dh_monopole_harmonics  out[n][norb] complex float32 (re, im) at n points (theta, phi): the
 *                        format of dh_monopole_orbitals, whose flux + 1 values are the level-0 block.
 * dh_rdm_displace        xp[P][B][nelec][nelec][2]: row (p B + b) nelec + a is walker b of
 *                        x[B][nelec][2] with electron a moved to r_prime[p][b] (r_prime[P][B][2]).
 * dh_rdm_accumulate      OVERWRITES rho[S][norb][norb][2] (re, im; double; S = 2, up then down,
 *                        when by_spin, else 1) with the SUM over the kept samples (b, p) of
 *                          4 pi u_i conj(v_j),  v_j = Y_j(r_prime[p][b]),
 *                          u_i = sum_a exp(logpsi_p[(p B + b) nelec + a] - logpsi[b]) Y_i(x[b][a]),
 *                        the sum over a restricted to the slots below n_up (up) or from n_up on
 *                        (down) when by_spin.  logpsi[B][2] and logpsi_p[P B nelec][2] are float32
 *                        (re, im) as dh_logpsi writes them for x and for xp; the difference is
 *                        exponentiated in double.  A sample is dropped when any of its nelec + 1
 *                        log-amplitudes or any of its ratios is not finite; nvalid (one device
 *                        int32) = the number kept, so rho / nvalid is the estimate.  The samples
 *                        are reduced on the device in a fixed order without float atomics: two
 *                        calls on the same inputs give identical bits.  workspace:
 *                        dh_rdm_workspace_bytes(B, nelec, flux, levels, P) device bytes (sized for
 *                        S = 2).
 * Checked before any device call, DH_EINVAL otherwise (the two queries then return 0):
 * 1 <= levels <= DH_RDM_MAX_LEVELS, 0 <= flux <= 126, 1 <= nelec <= 32, 0 <= n_up <= nelec,
 * B >= 1, P >= 1, P B <= 2^30, P B nelec^2 < 2^31, non-null pointers, the workspace size. */
#define DH_RDM_MAX_LEVELS 4
int dh_rdm_norb(int flux, int levels);
size_t dh_rdm_workspace_bytes(int B, int nelec, int flux, int levels, int P);
int dh_monopole_harmonics(const float* points, int n, int flux, int levels, float* out, void* stream);
int dh_rdm_displace(const float* x, const float* r_prime, int B, int nelec, int P, float* xp, void* stream);
int dh_rdm_accumulate(const float* x, const float* r_prime, const float* logpsi, const float* logpsi_p, int B,
                      int nelec, int n_up, int flux, int levels, int P, int by_spin, double* rho, int32_t* nvalid,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- Pair amplitudes in the lowest Landau level ---------------------------------------------------
 * A_L: the mean number of electron pairs with total pair angular momentum L = 0..flux (relative
 * angular momentum m = flux - L).  Spinor of a point: u = cos(theta / 2) e^{i phi / 2},
 * v = sin(theta / 2) e^{-i phi / 2}; <p|q> = u_p conj(u_q) + v_p conj(v_q).  For (r1, r2; r1', r2')
 *   a = <1|1'><2|2'>,  b = <1|2'><2|1'>,  d = (u1 v2 - v1 u2) conj(u1' v2' - v1' u2') = a - b,
 *   (4 pi)^2 K_L = n_L d^(flux - L) p_L,   p_0 = 1, p_1 = a + b,
 *   L p_L = (2L - 1)(a + b) p_{L-1} - (L - 1) d^2 p_{L-2},
 *   n_L = (flux + 1)^2 (2L + 1) / (flux + L + 1)  C(flux, L) / C(flux + L, L):
 * the projector onto pair angular momentum L built from the orbitals Y_{Q,Q,m}, summed over M.
 * Pairs q = (i < j) in lexicographic order, nelec (nelec - 1) / 2 of them.
 *
 * dh_pair_displace    xp[pair1 - pair0][P][B][nelec][2]: row ((q - pair0) P + p) B + b is walker b of
 *                     x[B][nelec][2] with electron i at r1[p][b] and electron j at r2[p][b]
 *                     (r1, r2 [P][B][2]), for the pairs pair0 <= q < pair1; copies of the floats.
 * dh_pair_kernel      out[n][flux + 1][2] (re, im; double) = (4 pi)^2 K_L of the n quadruples
 *                     points[n][4][2] = (r1, r2, r1', r2'), by the device function the accumulation
 *                     uses; NaN for a quadruple with a non-finite coordinate.
 * dh_pair_accumulate  OVERWRITES A[3][flux + 1][2] (re, im; double; up-up, up-down, down-down by the
 *                     slots below n_up or from n_up on) with the SUM over the kept samples (b, p) and
 *                     the pairs of the class of
 *                       (4 pi)^2 K_L(x[b][i], x[b][j]; r1[p][b], r2[p][b])
 *                         exp(logpsi_p[(q P + p) B + b] - logpsi[b]).
 *                     logpsi[B][2] and logpsi_p[pairs P B][2] are float32 (re, im) as dh_logpsi
 *                     writes them for x and for all of xp; the difference is exponentiated in
 *                     double.  A sample is dropped whole when its own log, any of its pairs' logs or
 *                     any ratio is not finite; nvalid (one device int32) = the number kept, so
 *                     A / nvalid is the estimate.  A fixed order, no float atomics: two calls on
 *                     the same inputs give identical bits.  workspace:
 *                     dh_pair_workspace_bytes(B, nelec, flux, P) device bytes, 16-byte aligned.
 * Checked before any device call, DH_EINVAL otherwise (the query then returns 0): 1 <= nelec <= 32,
 * 0 <= flux <= 126, 0 <= n_up <= nelec, B >= 1, P >= 1, P B <= 2^30, P B nelec (nelec - 1) / 2 < 2^31, the pair
 * window 0 <= pair0 < pair1 <= pairs, n >= 1, n (flux + 1) < 2^31, non-null pointers, the workspace
 * size. */
size_t dh_pair_workspace_bytes(int B, int nelec, int flux, int P);
int dh_pair_displace(const float* x, const float* r1, const float* r2, int B, int nelec, int P, int pair0, int pair1,
                     float* xp, void* stream);
int dh_pair_kernel(const float* points, int n, int flux, double* out, void* stream);
int dh_pair_accumulate(const float* x, const float* r1, const float* r2, const float* logpsi, const float* logpsi_p,
                       int B, int nelec, int n_up, int flux, int P, double* A, int32_t* nvalid, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- Total spin: <S^2> by exchanging one up and one down electron ----------------------------
 * Walkers x[B][nelec][2]; the slots below n_up are up electrons (n_up + n_dn = nelec).  Pair
 * p = i n_dn + (j - n_up) of an up slot i and a down slot j, P = n_up n_dn pairs; R_p is the walker
 * with the coordinates of slots i and j exchanged (copies of the stored floats), and
 *   S^2_loc(R) = ((n_up - n_dn) / 2)^2 + nelec / 2 - sum_p psi(R_p) / psi(R).
 *
 * dh_spin_exchange  xs[(pair1 - pair0) B][nelec][2]: row (p - pair0) B + b is R_p of walker b, for
 *                   the pairs pair0 <= p < pair1 (0 <= pair0 < pair1 <= P).
 * dh_spin_ratios    stores exp(logpsi_s[(p - pair0) B + b] - logpsi[b]) of that window in the
 *                   workspace, in double from the float32 logs (re, im as dh_logpsi writes them for
 *                   x and xs); NaN where a log or the ratio is not finite.  What a pair stores does
 *                   not depend on the window it came in.
 * dh_spin_reduce    after EVERY pair has been stored: s2[B][2] (re, im; double) = S^2_loc per
 *                   walker, the pairs added in ascending p; pairs[n_up][n_dn][2], the sum of the
 *                   ratio of each pair over the valid walkers; total[2], the sum of s2 over them;
 *                   nvalid (one device int32), their number.  A walker is valid when its own log
 *                   and all its P ratios are finite; an invalid one gets s2 = NaN and enters no sum.
 *                   Double arithmetic, a fixed order, no float atomics: two calls give identical
 *                   bits, and so do one window of all pairs and one window per pair.  With P = 0
 *                   (no exchange, no ratios, pairs may be null) s2 = (nelec / 2)(nelec / 2 + 1).
 * workspace: dh_spin_workspace_bytes(B, n_up, n_dn) device bytes, 16-byte aligned, the same buffer
 * for the ratios and the reduce.  Checked before any device call, DH_EINVAL otherwise (the query
 * then returns 0): B >= 1, n_up, n_dn >= 0, 1 <= n_up + n_dn <= 32, B n_up n_dn < 2^31, the window,
 * non-null pointers; a short workspace is DH_ENOMEM.  No dh_handle, as for the swap kernels. */
size_t dh_spin_workspace_bytes(int B, int n_up, int n_dn);
int dh_spin_exchange(const float* x, int B, int nelec, int n_up, int n_dn, int pair0, int pair1, float* xs,
                     void* stream);
int dh_spin_ratios(const float* logpsi, const float* logpsi_s, int B, int n_up, int n_dn, int pair0, int pair1,
                   void* workspace, size_t workspace_bytes, void* stream);
int dh_spin_reduce(const float* logpsi, int B, int n_up, int n_dn, void* workspace, size_t workspace_bytes,
                   double* s2, double* pairs, double* total, int32_t* nvalid, void* stream);

/* ---- Static structure factor S(L) from the walkers alone ---------------------------------------
 * Walkers x[B][nelec][2] float32 (theta, phi); the slots below n_up are up electrons.  All
 * arithmetic in double.  gamma_ij is the angle between electrons i and j,
 *   cos gamma = cos th_i cos th_j + sin th_i sin th_j cos(ph_i - ph_j).
 *
 * dh_sf_pairs       T[B][3][lmax+1]: T[b][s][L] = sum over the pairs i < j of species s of
 *                   P_L(cos gamma_ij); s = 0 both up, 1 i up and j down, 2 both down.  Row L = 0 is
 *                   the pair count exactly; nothing is clamped (cos gamma = 1, -1 give 1, (-1)^L).
 * dh_sf_multipoles  rho[B][2][nlm][2] (re, im): rho[b][a][lm] = sum over the electrons of species a
 *                   (0 up, 1 down) of Y_LM(th, ph), 0 <= M <= L <= lmax, lm = L (L + 1) / 2 + M,
 *                   nlm = dh_sf_nlm(lmax) = (lmax + 1)(lmax + 2) / 2.  Orthonormal Y_LM with the
 *                   Condon-Shortley phase (Y_{L,-M} = (-1)^M conj Y_LM), by fully normalised
 *                   recurrences: no overflow at any L <= DH_SF_MAX_L, and sin^M th underflowing to 0
 *                   near a pole is the correct value.
 *                   A walker is valid when its 2 nelec coordinates are all finite; both calls write
 *                   NaN rows for an invalid one.
 * dh_sf_accumulate  pair_sums[3][lmax+1] and (want_multipoles != 0) rho_sums[2][nlm][2]: the sums of
 *                   the above over the valid walkers, and nvalid (one device int32), their number.
 *                   Nothing per walker leaves the kernel: each workgroup adds a contiguous range of
 *                   walkers in order into one partial in the workspace, a second kernel adds the
 *                   partials in order.  No float atomics: two calls give identical bits, and
 *                   pair_sums are the same bits with want_multipoles = 0, which skips the multipoles
 *                   entirely (rho_sums may then be null and is not touched).  No valid walker:
 *                   zero sums and nvalid = 0.
 * workspace: dh_sf_workspace_bytes(B, nelec, lmax) device bytes, 8-byte aligned.  Checked before any
 * device call, DH_EINVAL otherwise (dh_sf_nlm then returns -1, dh_sf_workspace_bytes 0): B >= 1,
 * 1 <= nelec <= 32, B nelec < 2^31, 0 <= n_up <= nelec, 0 <= lmax <= DH_SF_MAX_L, non-null
 * pointers, the workspace size.  No dh_handle, as for the swap kernels. */
#define DH_SF_MAX_L 64
int dh_sf_nlm(int lmax);
size_t dh_sf_workspace_bytes(int B, int nelec, int lmax);
int dh_sf_pairs(const float* x, int B, int nelec, int n_up, int lmax, double* T, void* stream);
int dh_sf_multipoles(const float* x, int B, int nelec, int n_up, int lmax, double* rho, void* stream);
int dh_sf_accumulate(const float* x, int B, int nelec, int n_up, int lmax, int want_multipoles, double* pair_sums,
                     double* rho_sums, int32_t* nvalid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Quasihole overlap matrix: K configurations of the pinned holes on the same walkers -------
 * A configuration is one setting of the holes of a dh_quasihole state: n_holes points and kinds.
 * All K configurations share the base, the exponents, p and n_holes, and each passes the checks of
 * dh_create_quasihole against the same dh_config, so all live at the same flux; the kinds may
 * differ between configurations (the pairings of the Pfaffian base).
 *
 * dh_hole_table  checks cfg and configs and fills the packed table on the host (no device call):
 *                uv[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES][4] double (Re U, Im U, Re V, Im V,
 *                the spinors a dh_create_quasihole handle holds; zero where unused), then
 *                kind[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES] int (-1 where unused):
 *                dh_hole_table_bytes() bytes.  The caller copies it to device memory it owns.
 * dh_hole_logs   L[B][n_configs][2] (re, im; double) = log psi_c(R_b) for walkers x[B][nelec][2]
 *                float32 and the device copy of the table made from the same cfg and configs (both
 *                are checked again, on the host); Im reduced as dh_logpsi reduces it.  L[b][c]
 *                rounded to float32 is dh_logpsi of a dh_create_quasihole handle with configuration
 *                c, bit for bit.  One workgroup per walker walks the configurations: the electrons'
 *                spinors and the pair part are formed once per walker.
 * dh_hole_gram   with r[b][c] = exp(L[b][c] - L[b][0] - shift[c]), shift[n_configs] real (device,
 *                zeros allowed): S[n_configs][n_configs][2] (re, im; double), S[c][c'] = sum over
 *                the valid walkers of conj(r[b][c]) r[b][c'], and nvalid (one device int32), their
 *                number.  A walker with a non-finite entry of L, or a ratio that overflows, is
 *                dropped.  Double arithmetic, a fixed order, no float atomics: two calls give
 *                identical bits.
 * workspace (dh_hole_gram): dh_hole_workspace_bytes(B, n_configs) device bytes, 16-byte aligned.
 * Checked before any device call, DH_EINVAL with a message that starts "Holes:" otherwise (the
 * workspace query then returns 0): non-null pointers, the struct sizes, 1 <= n_configs <=
 * DH_HOLE_MAX_CONFIGS, every configuration, B >= 1, B n_configs < 2^31, the table and workspace
 * sizes (a short workspace is DH_ENOMEM). */
#define DH_HOLE_MAX_CONFIGS 16
typedef struct dh_hole_configs {
  uint32_t struct_size;                     /* = sizeof(dh_hole_configs) = 2592 bytes             */
  int base;                                 /* DH_QUASIHOLE_HALPERIN or DH_QUASIHOLE_PFAFFIAN      */
  int m_up, m_dn, n_inter;                  /* Halperin base: the exponents                        */
  int p;                                    /* Pfaffian base: 2 p vortices per electron            */
  int n_holes;                              /* holes of every configuration                        */
  int n_configs;
  int kind[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES];       /* DH_HOLE_* of hole a of config c */
  double holes[DH_HOLE_MAX_CONFIGS][DH_QUASIHOLE_MAX_HOLES][2]; /* its (theta, phi)               */
} dh_hole_configs;
size_t dh_hole_table_bytes(void);
int dh_hole_table(const dh_config* cfg, const dh_hole_configs* configs, void* table_host, size_t bytes);
size_t dh_hole_workspace_bytes(int B, int n_configs);
int dh_hole_logs(const dh_config* cfg, const dh_hole_configs* configs, const float* x, int B, const void* table,
                 size_t table_bytes, double* L, void* stream);
int dh_hole_gram(const double* L, int B, int n_configs, const double* shift, double* S, int32_t* nvalid,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- Subspace matrices: overlap, Hamiltonian and kinetic energy of K states (subspace.hip) -----
 * K wavefunctions on one set of B walkers, stacked by state c = 0 .. K - 1, state 0 the one the
 * walkers sample.  All three inputs are float32 (re, im) pairs as dh_local_energy writes them:
 *   logs[K][B][2]  log|psi_c| and arg psi_c    (obs columns 6, 7)
 *   e_l[K][B][2]   the local energy of psi_c   (e_l)
 *   ke[K][B][2]    its kinetic part            (obs columns 0, 1)
 * and shift[K] is real (device, double, zeros allowed), as dh_hole_gram takes it.  With
 * r_c(b) = exp(logs[c][b] - logs[0][b] - shift[c]), out[3][K][K][2] (re, im; double) holds
 *   out[0] = S[c][c'] = sum_b conj(r_c) r_c'
 *   out[1] = H[c][c'] = sum_b conj(r_c) r_c' e_l[c'][b]     (the operator acts on the ket)
 *   out[2] = T[c][c'] = sum_b conj(r_c) r_c' ke[c'][b]
 * over the valid walkers, and nvalid (one device int32) is their number.  A walker is valid when
 * its 6 K inputs and its K ratios are all finite; an invalid one is dropped from every entry.
 * Everything after the subtraction of the logs is double, the sums run in an order that depends on
 * B and K alone, and there are no float atomics: two calls give identical bits.  H and T are not
 * Hermitian on a finite sample; the caller Hermitises them.
 * workspace: dh_subspace_workspace_bytes(B, K) device bytes, 16-byte aligned.  Checked before any
 * device call, DH_EINVAL with a message that starts "subspace:" otherwise (the workspace query
 * then returns 0): non-null pointers, B >= 1, 1 <= K <= DH_SUBSPACE_MAX_STATES, K B < 2^31, the
 * workspace size.  No dh_handle, as for the swap kernels. */
#define DH_SUBSPACE_MAX_STATES 32
size_t dh_subspace_workspace_bytes(int B, int K);
int dh_subspace_accumulate(const float* logs, const float* e_l, const float* ke, int B, int K, const double* shift,
                           double* out, int32_t* nvalid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Impurity potential and the density around an axis (impurity.hip): no handle -------------
 * Walkers x[B][nelec][2] float32 (theta, phi), nelec = n_up + n_dn, the slots below n_up up.  All
 * arithmetic in double on the upcast angles.  With R = radius, u = r_i . r_a the cosine of the
 * angle between electron i and impurity a, and the squared chord c^2 = 2 R^2 (1 - u):
 *   DH_IMPURITY_GAUSSIAN  U_a = strength exp(-c^2 / (2 width^2))
 *   DH_IMPURITY_CHARGE    U_a = strength / sqrt(c^2 + width^2)   (a point charge at height width)
 * species: DH_HOLE_BOTH, DH_HOLE_UP or DH_HOLE_DOWN, the electrons the impurity acts on.
 *
 * dh_impurity_check       the checks of the array alone, no device call: 0 <= n_imp <=
 *                         DH_MAX_IMPURITIES, non-null when n_imp > 0, every field finite, width > 0,
 *                         a known kind and species, 0 <= theta <= pi.
 * dh_external_potential   ext[b] (float32) = sum_a sum_{i in species(a)} U_a(r_i); when e_l
 *                         (dh_local_energy's [B][2]) is not null also e_l[b][0] = (float)((double)
 *                         e_l[b][0] + the sum), e_l[b][1] untouched.  The impurities are a host array and
 *                         reach the kernel by value; no device memory is allocated.  A fixed order and
 *                         no float atomics: a walker's value is the same bits alone and in any batch.  A
 *                         walker with a non-finite coordinate gives NaN in ext and in e_l[b][0].
 * dh_axis_histogram       adds to counts[2][bins] (device, unsigned; row 0 up, row 1 down) the
 *                         electrons by u = r_i . a, a the axis (axis_theta, axis_phi): bins of equal
 *                         area, bin k is 1 - 2 (k + 1) / bins < u <= 1 - 2 k / bins, the last one
 *                         closed at u = -1; NaN is dropped.  Integer atomics: two calls give the
 *                         same bits.  The caller zeroes counts.
 * Checked before any device call, DH_EINVAL with a message that starts "impurity:" otherwise:
 * non-null pointers, B >= 1, n_up, n_dn >= 0, 1 <= nelec <= 32, B nelec < 2^31, radius finite and
 * > 0, the impurities as dh_impurity_check, the axis finite with 0 <= axis_theta <= pi,
 * 1 <= bins <= 4096. */
#define DH_MAX_IMPURITIES 8
#define DH_IMPURITY_GAUSSIAN 0
#define DH_IMPURITY_CHARGE 1
typedef struct dh_impurity {
  double theta, phi, strength, width;
  int kind, species;
} dh_impurity;
int dh_impurity_check(const dh_impurity* impurities, int n_imp);
int dh_external_potential(const float* x, int B, int n_up, int n_dn, double radius, const dh_impurity* impurities,
                          int n_imp, float* e_l, float* ext, void* stream);
int dh_axis_histogram(const float* x, int B, int n_up, int n_dn, double axis_theta, double axis_phi, int bins,
                      unsigned* counts, void* stream);

/* ---- log psi supplied by the caller: the arbitrary-callable boundary ---------------------
 * The reference's make_mcmc_step(batch_network, ...) (mcmc.py:105-150) and
 * make_local_kinetic_energy(f, Q, r) (hamiltonian.py:83-172) accept ANY log psi.  For one
 * that is not a network of this library the caller evaluates log psi (and, for the energy,
 * its derivatives) itself; these entry points do the rest on the device.
 *
 * MCMC with the same random streams as dh_mcmc_step (so a caller-evaluated network walks
 * exactly as the native one):
 *   dh_mh_init     lp[b] = 2 Re logpsi[b][0], n_accept[b] = 0           (mcmc.py:142)
 *   dh_mh_propose  x2 = sph_sampling(x) for step `step` = counter + s    (mcmc.py:67-102)
 *   dh_mh_accept   accept/select with logpsi2[B][2] = log psi(x2) (re, im): x, lp, n_accept
 *                  updated where 2 Re log psi(x2) - lp > log U             (mcmc.py:25-64)
 * noise: NULL or this step's injected [B][2N+1] (dh_mcmc_step layout).
 *
 * dh_kinetic_from_derivatives: KE (complex) and Lz, Lz^2, L^2 from x[B][N][2], the complex
 * first derivatives grad[B][N][2][2] (d/dtheta, d/dphi; re, im) and complex Hessian
 * hess[B][N][2][N][2][2] of log psi, all double; Q monopole strength, r radius; nelec <= 256.
 * Out: ke[B][2] (re, im), mom[B][3] (Lz, Lz^2, L^2). */
int dh_mh_init(const float* logpsi, float* lp, int32_t* n_accept, int B, void* stream);
int dh_mh_propose(const float* x, float* x2, int B, int nelec, float width, uint64_t seed, uint64_t step,
                  int64_t walker_offset, const float* noise, void* stream);
int dh_mh_accept(float* x, const float* x2, float* lp, const float* logpsi2, int32_t* n_accept, int B, int nelec,
                 uint64_t seed, uint64_t step, int64_t walker_offset, const float* noise, void* stream);
int dh_kinetic_from_derivatives(const double* x, const double* grad, const double* hess, int B, int nelec, double Q,
                                double r, float* ke, float* mom, void* stream);

/* Kernel timing with HIP events on the launch stream (bench / roofline).
 * dh_profile_enable(h, 1) starts recording every kernel launch of this handle;
 * dh_profile_read fills out[k*4 + {0,1,2,3}] = {launches, total ms, algorithmic
 * FLOPs, algorithmic bytes} for kernel class k (returns the number of classes):
 *   0 GEMM  1 attention  2 LayerNorm  3 input  4 det (log psi)  5 det (energy)
 *   6 MCMC proposal/accept; 7-10 = classes 0-3 launched with 2N+5 channels
 *   (local energy); 11 = layer 1 of the local energy in one launch (gemm_lnch MODE 2:
 *   LayerNorms, tanh and three 32-deep products).  out holds 4 * 12 doubles.
 *   Synchronises on the recorded events.
 *   A class is timed by events around its launches, so while recording is on a log-psi pass
 *   launches the value kernel (class 4) on its own even where it would otherwise run as the tail
 *   of the last chain launch (dh_debug_det_in_chain); the results are bit-identical. */
int dh_profile_enable(dh_handle* h, int on);
int dh_profile_read(dh_handle* h, double* out, int reset);

/* Test hooks: run the network trunk + orbital map only and leave the
 * activations in the workspace (trunk output at float offset 0, orbital
 * features F [rows][ld_orb] at float offset dh_debug_f_offset).
 * Where the pass maps no F over its rows (dh_debug_route field 10 = 0: op 1 of the
 * envelope-first configs, one determinant of one spin block at N = 10, 20), nothing is run:
 * dh_debug_trunk returns DH_EINVAL and dh_debug_f_offset returns (size_t)-1, as it does for a
 * null handle or B < 1. */
int dh_debug_trunk(dh_handle* h, const float* x, int B, int op, void* ws, size_t ws_bytes, void* stream);
size_t dh_debug_f_offset(const dh_handle* h, int B, int op);
/* Test hook: the envelope leaves of det.hip's env_leaf (e0, d/dtheta, d/dphi / sin theta,
 * Laplace-Beltrami, d2/dtheta2 as re / im pairs: 10 floats) of n (theta, phi) pairs thph[n][2]
 * for every harmonic p < M (norm 1, the kernels' gauge kappa = env_gauge(cos theta)) into
 * out[n][M][10]; sq = 1: integer powers by squaring (the production form), 0: powf. */
int dh_debug_env_leaf(const float* thph, int n, int M, int sq, float* out, void* stream);
/* Test hook: one launch of GEMM kernel variant `variant`:
 * Y = X W (+ bias on rows r % C == 0) (+ R).  X must hold round_up(rows, 256) rows.
 * Valid codes: the register-staged tiles 0 .. 11 but 3 (production: 9, 10; -1 = 0), and the
 * NT kernels 100 .. 107, three-stage 110, 111, 114 .. 117 (production: 104, 106, 107) and
 * persistent 120 .. 126 (production: 120, 125; whole tiles written, Y padded to 256 rows and
 * 256 columns).
 * With a code >= 100, W is the TRANSPOSED weight Wt[n][k] (row stride ldw) holding
 * round_up(ncols, 256) rows, and K % 32 == 0.  Any other code: DH_EINVAL, checked before any
 * pointer is used. */
int dh_debug_gemm(int variant, const float* X, int ldx, const float* W, int ldw, const float* bias, const float* R,
                  int ldr, float* Y, int ldy, int rows, int ncols, int K, int C, void* stream);

/* Test hook: the log-psi GEMM with the LayerNorm fused into its epilogue (D = 256):
 * h = LN(h + X Wt^T + bias) (mode 0) or LN(h + tanh(X Wt^T + bias)) (mode 1), in place;
 * Wt[256][K] transposed weight (row stride ldw), ln = gamma[256] | beta[256];
 * bm = rows per workgroup (32, 64, 96; 0 = automatic).  X, h hold round_up(rows, 96) rows. */
int dh_debug_gemm_ln(int mode, int bm, const float* X, int ldx, const float* Wt, int ldw, const float* bias,
                     const float* ln, float* h, int rows, int K, void* stream);

/* Split-bf16 form of dh_debug_gemm_ln (weight as the planes of dh_debug_split_planes,
 * ldp >= dh_debug_x6_plane_rows(256)); nw = tile form: 1 = 96 rows x (3 x 4 waves),
 * 2 = 64 rows x (2 x 4 waves), 8 = 128 rows x (4 x 4 waves), 3 / 4 = 96 / 128 rows of
 * whole-row waves, 0 = choose (among 1, 2, 8).  Any other nw:
 * DH_EINVAL, checked before any pointer is used. */
int dh_debug_gemm_x6_ln(int mode, int nw, const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias,
                        const float* ln, float* h, int rows, int K, void* stream);
/* Chained log-psi layer tail (gemm_x6.hip chain_x6_kernel; D = K = 256, rows padded to 768):
 * h1 = LN1(h + X1 W1 + b1); h = LN2(h1 + tanh(h1 W2 + b2)); Y3 = h W3 + b3 when Wp3. */
int dh_debug_chain_x6(const float* X1, const uint16_t* Wp1, int ldp1, const float* b1, const float* ln1,
                      const uint16_t* Wp2, int ldp2, const float* b2, const float* ln2, const uint16_t* Wp3,
                      int ldp3, const float* b3, int n3, float* Y3, int ldy3, float* h, int rows, void* stream);

/* Fused channel GEMM + channel LayerNorm (gemm_lnch.hip; D = K = 256, N <= 6): in place over
 * h [ne * (2N + 5)][256], mode 0: h = LN_ch(h + X W + b), mode 1: h = LN_ch(h + tanh_ch(h W + b))
 * (X ignored); geo [ne][4] = (sin th, cos th, sin ph, cos ph) of the walkers' electrons. */
int dh_debug_gemm_lnch(int N, int mode, const float* X, const uint16_t* Wp, int ldp, const float* bias,
                       const float* ln, const float* geo, float* h, int ne, void* stream);

/* Test hooks of the split-bf16 GEMM (gemm_x6.hip): the transposed weight Wt[ncols][K]
 * is split into three bf16 planes Wp[3][ldp][K] (ldp = dh_debug_x6_plane_rows(ncols),
 * uint16 bit patterns), then Y = X Wt^T (+ bias on rows r % C == 0) (+ R) with
 * K % 32 == 0 and X holding round_up(rows, 256) rows.  The codes production picks: 44, 46
 * (gemm_x6d, 128 x 192 and 256 x 128 tiles), 52, 56, 57, 58 (gemm_x6q, 256 x 128 / 256 / 192 /
 * 160), 76, 77 (gemm_x6m, 256 x 256 / 192), -1 = automatic.  Kept beside them for comparison:
 * 40, 41, 43, 45, 60, 61, 62 (gemm_x6d), 50, 51 (gemm_x6q), 79 .. 83, 90 (gemm_x6m).  Any other
 * code: DH_EINVAL, checked before any pointer is used.
 * dh_debug_gemm_x6_choice: the code the automatic choice takes for (rows, ncols); host only. */
int dh_debug_gemm_x6_choice(int rows, int ncols);
/* Test hook: which launches make up one pass of B walkers (op 0: log psi, 1 channel; op 1: the
 * local energy, 2N+5 channels, one chunk) in the handle's GEMM mode (dh_set_gemm_mode; no
 * parameters needed).  Host only: no device call.  Writes min(n, 12) ints to out and returns 12:
 *   0 dense GEMM family: 0 exact-f32 W, 1 exact-f32 W^T (NT), 2 split-bf16
 *   1 the input kernel writes h0 = f W0     2 ... and layer 1's q|k|v     3 it writes the geometry
 *     only, and is skipped when the MCMC proposal already wrote that
 *   4 form of layer 1, 5 of every later layer: 0 GEMM, LayerNorm, GEMM, LayerNorm; 1 two GEMMs
 *     with the LayerNorm in the epilogue; 2 chain (both and the next linear map in one launch);
 *     3 chain with layer 1's attention in its prologue; 4 gemm_lnch pair (channel rows, GEMM +
 *     LayerNorm per launch); 5 gemm_lnch whole layer; 6 layer1_ch (whole layer, N = 10, 20)
 *   6 layer 1's attention forms q|k|v from the features     7 layer 1's residual h0 is formed in
 *     its first map's epilogue / LayerNorm     8 that map contracts the o~ rows with U (K = 32)
 *   9 layers >= 2: a q|k|v GEMM precedes attention (a chained layer's last pass wrote it)
 *  10 orbital map: 0 none (envelope first), 1 a GEMM, 2 the last chain launch
 *  11 determinant stage: 0 value kernel (op 0), 1 direct from F, 2 precontracted PhiC,
 *     3 envelope first (PhiC from h, no F)
 * DH_EINVAL (negative) for a Laughlin handle or B < 1. */
int dh_debug_route(const dh_handle* h, int B, int op, int* out, int n);
/* Test hooks of the determinant tail: where a log-psi pass ends in a chain launch that maps the
 * orbitals (route fields 5 = 2, 10 = 2) and the value kernel would put two walkers on a wave
 * (N = 6 at 2Q = 15), that launch runs the value kernel's work as its tail on orbital rows still in
 * the CU (gemm_x6.hip), and no value kernel is launched; bit-identical results.
 * dh_debug_set_det_in_chain(0) makes every later pass of the process launch the value kernel on
 * its own instead (1: the default); it returns the previous setting.
 * dh_debug_det_in_chain: 1 if a pass of B walkers (op as dh_debug_route) carries the tail under
 * the current setting, else 0 (a pass run while dh_profile_enable records launches the value
 * kernel on its own all the same); host only; DH_EINVAL (negative) as dh_debug_route. */
int dh_debug_set_det_in_chain(int on);
int dh_debug_det_in_chain(const dh_handle* h, int B, int op);
int dh_debug_x6_plane_rows(int ncols);
int dh_debug_split_planes(const float* Wt, int ldw, int ncols, int K, uint16_t* Wp, void* stream);
int dh_debug_gemm_x6(int variant, const float* X, int ldx, const uint16_t* Wp, int ldp, const float* bias,
                     const float* R, int ldr, float* Y, int ldy, int rows, int ncols, int K, int C, void* stream);

/* init_guess with the device RNG: theta = arccos U(-1,1), phi = U(-pi,pi). */
int dh_init_walkers(dh_handle* h, float* x, int B, uint64_t seed, int64_t walker_offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPHALL_AMD_H */
