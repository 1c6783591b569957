"""ctypes binding of the C ABI declared in include/deephall_amd.h.

The HIP library is the only compute path: if it is missing this module raises —
there is no CPU / PyTorch fallback.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "_lib" / "libdeephall_amd.so"

DH_NSTATS = 16
STAT_NAMES = [
    "energy_re",
    "energy_im",
    "clipped_re",
    "clipped_im",
    "ere2",
    "kinetic_re",
    "kinetic_im",
    "potential",
    "angular_momentum_z",
    "angular_momentum_z_square",
    "angular_momentum_square",
    "pmove",
    "nvalid",
    "clipped_lz2",
    "clipped_lz",
    "clipped_l2",
]

EXPORTS = [
    "dh_create",
    "dh_create_cf",
    "dh_destroy",
    "dh_last_error",
    "dh_version",
    "dh_param_layout",
    "dh_set_params",
    "dh_workspace_bytes",
    "dh_set_gemm_mode",
    "dh_logpsi",
    "dh_mcmc_step",
    "dh_local_energy",
    "dh_energy_stats",
    "dh_loss_diff",
    "dh_init_walkers",
    "dh_potential",
    "dh_histograms",
    "dh_monopole_orbitals",
    "dh_mh_init",
    "dh_mh_propose",
    "dh_mh_accept",
    "dh_kinetic_from_derivatives",
    "dh_debug_trunk",
    "dh_debug_gemm",
    "dh_debug_gemm_ln",
    "dh_debug_gemm_x6_ln",
    "dh_debug_chain_x6",
    "dh_debug_gemm_lnch",
    "dh_debug_set_lnch_form",
    "dh_debug_x6_plane_rows",
    "dh_debug_split_planes",
    "dh_debug_gemm_x6",
    "dh_debug_gemm_x6_choice",
    "dh_debug_route",
    "dh_debug_set_det_in_chain",
    "dh_debug_det_in_chain",
    "dh_ref_layout",
    "dh_set_params_ref",
    "dh_vjp_workspace_bytes",
    "dh_logpsi_vjp",
    "dh_grad_cotangent",
    "dh_adam_update",
    "dh_profile_enable",
    "dh_profile_read",
    "dh_debug_f_offset",
    "dh_debug_env_leaf",
    "dh_kfac_layout",
    "dh_kfac_workspace_bytes",
    "dh_kfac_vjp",
    "dh_kfac_step",
    "dh_ntk_workspace_bytes",
    "dh_ntk_tile_walkers",
    "dh_ntk",
    "dh_ntk_part",
    "dh_ntk_mirror",
    "dh_ntk_owner",
    "dh_minsr_matrix_workspace_bytes",
    "dh_minsr_matrix",
    "dh_ntk_jvp_workspace_bytes",
    "dh_ntk_jvp",
    "dh_fidelity_partial",
    "dh_fidelity_residual",
    "dh_ortho_partial",
    "dh_ortho_residual",
    "dh_swap_classify",
    "dh_swap_compact",
    "dh_swap_reduce",
    "dh_swap_workspace_bytes",
    "dh_rdm_norb",
    "dh_rdm_workspace_bytes",
    "dh_monopole_harmonics",
    "dh_rdm_displace",
    "dh_rdm_accumulate",
    "dh_create_halperin",
    "dh_spin_workspace_bytes",
    "dh_spin_exchange",
    "dh_spin_ratios",
    "dh_spin_reduce",
    "dh_sf_nlm",
    "dh_sf_workspace_bytes",
    "dh_sf_pairs",
    "dh_sf_multipoles",
    "dh_sf_accumulate",
    "dh_create_quasihole",
    "dh_hole_table_bytes",
    "dh_hole_table",
    "dh_hole_workspace_bytes",
    "dh_hole_logs",
    "dh_hole_gram",
    "dh_impurity_check",
    "dh_external_potential",
    "dh_axis_histogram",
    "dh_pair_workspace_bytes",
    "dh_pair_displace",
    "dh_pair_kernel",
    "dh_pair_accumulate",
    "dh_subspace_workspace_bytes",
    "dh_subspace_accumulate",
]

DH_QUASIHOLE_MAX_HOLES = 8
DH_HOLE_MAX_CONFIGS = 16
QUASIHOLE_BASES = {"halperin": 0, "pfaffian": 1}  # DH_QUASIHOLE_*
HOLE_KINDS = {"both": 0, "up": 1, "down": 2, "A": 3, "B": 4}  # DH_HOLE_*

DH_MAX_IMPURITIES = 8
IMPURITY_KINDS = {"gaussian": 0, "charge": 1}  # DH_IMPURITY_*
IMPURITY_SPECIES = {"both": 0, "up": 1, "down": 2}  # DH_HOLE_BOTH, DH_HOLE_UP, DH_HOLE_DOWN
DH_AXIS_MAX_BINS = 4096

DH_SWAP_MAX_ANGLES = 64
DH_RDM_MAX_LEVELS = 4
DH_SF_MAX_L = 64
DH_SUBSPACE_MAX_STATES = 32

DH_NFID = 5  # dh_fidelity_partial: m, S re, S im, S2, n
DH_ORTHO_MAX_STATES = 16


PROF_KINDS = ["gemm", "attention", "layernorm", "input", "det_value", "det_energy", "mcmc",
              "gemm_ch", "attention_ch", "layernorm_ch", "input_ch", "layer1_ch"]


class DhConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_up", C.c_int),
        ("n_dn", C.c_int),
        ("flux", C.c_int),
        ("radius", C.c_float),
        ("interaction_strength", C.c_float),
        ("interaction_type", C.c_int),
        ("num_heads", C.c_int),
        ("heads_dim", C.c_int),
        ("num_layers", C.c_int),
        ("ndets", C.c_int),
        ("orbital_type", C.c_int),
        ("network_type", C.c_int),
        ("excitation_lz", C.c_float),
        ("cf_flux", C.c_int),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(DhConfig)


class DhQuasihole(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", C.c_int),
        ("m_up", C.c_int),
        ("m_dn", C.c_int),
        ("n_inter", C.c_int),
        ("p", C.c_int),
        ("n_holes", C.c_int),
        ("kind", C.c_int * DH_QUASIHOLE_MAX_HOLES),
        ("holes", (C.c_double * 2) * DH_QUASIHOLE_MAX_HOLES),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(DhQuasihole)


class DhHoleConfigs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("base", C.c_int),
        ("m_up", C.c_int),
        ("m_dn", C.c_int),
        ("n_inter", C.c_int),
        ("p", C.c_int),
        ("n_holes", C.c_int),
        ("n_configs", C.c_int),
        ("kind", (C.c_int * DH_QUASIHOLE_MAX_HOLES) * DH_HOLE_MAX_CONFIGS),
        ("holes", ((C.c_double * 2) * DH_QUASIHOLE_MAX_HOLES) * DH_HOLE_MAX_CONFIGS),
    ]

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(DhHoleConfigs)


class DhImpurity(C.Structure):
    _fields_ = [
        ("theta", C.c_double),
        ("phi", C.c_double),
        ("strength", C.c_double),
        ("width", C.c_double),
        ("kind", C.c_int),
        ("species", C.c_int),
    ]


_lib = None


def load(path: Path | str | None = None):
    """Load (once) and return the HIP library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # DH_LIB_PATH: an alternative build of the same library (A/B timing tools only)
    p = Path(path) if path else Path(os.environ.get("DH_LIB_PATH") or LIB_PATH)
    if not p.exists():
        raise RuntimeError(
            f"deephall_amd HIP library not found at {p}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)."
        )
    lib = C.CDLL(str(p))
    vp, sz, i32, u64, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_int64
    lib.dh_create.argtypes = [C.POINTER(DhConfig), C.POINTER(vp)]
    lib.dh_create.restype = i32
    lib.dh_create_cf.argtypes = [C.POINTER(DhConfig), C.POINTER(C.c_int), i32, C.POINTER(vp)]
    lib.dh_create_cf.restype = i32
    lib.dh_destroy.argtypes = [vp]
    lib.dh_destroy.restype = None
    lib.dh_last_error.restype = C.c_char_p
    lib.dh_version.restype = C.c_char_p
    lib.dh_param_layout.argtypes = [vp, C.POINTER(sz), i32]
    lib.dh_param_layout.restype = i32
    lib.dh_set_params.argtypes = [vp, vp, sz, vp]
    lib.dh_set_params.restype = i32
    lib.dh_workspace_bytes.argtypes = [vp, i32, i32]
    lib.dh_workspace_bytes.restype = sz
    lib.dh_set_gemm_mode.argtypes = [vp, i32]
    lib.dh_set_gemm_mode.restype = i32
    lib.dh_logpsi.argtypes = [vp, vp, i32, vp, vp, sz, vp]
    lib.dh_logpsi.restype = i32
    lib.dh_mcmc_step.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, u64, u64, i64, vp, vp, sz, vp]
    lib.dh_mcmc_step.restype = i32
    lib.dh_local_energy.argtypes = [vp, vp, i32, vp, vp, vp, sz, vp]
    lib.dh_local_energy.restype = i32
    lib.dh_energy_stats.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    lib.dh_energy_stats.restype = i32
    f32 = C.c_float
    lib.dh_loss_diff.argtypes = [vp, vp, vp, i32, vp, f32, f32, f32, vp, vp, vp]
    lib.dh_loss_diff.restype = i32
    lib.dh_init_walkers.argtypes = [vp, vp, i32, u64, i64, vp]
    lib.dh_init_walkers.restype = i32
    lib.dh_potential.argtypes = [vp, vp, i32, vp, vp]
    lib.dh_potential.restype = i32
    lib.dh_histograms.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    lib.dh_histograms.restype = i32
    lib.dh_monopole_orbitals.argtypes = [vp, i32, i32, vp, vp]
    lib.dh_monopole_orbitals.restype = i32
    lib.dh_debug_trunk.argtypes = [vp, vp, i32, i32, vp, sz, vp]
    lib.dh_debug_trunk.restype = i32
    lib.dh_debug_f_offset.argtypes = [vp, i32, i32]
    lib.dh_debug_f_offset.restype = sz
    lib.dh_debug_env_leaf.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dh_debug_env_leaf.restype = i32
    lib.dh_debug_gemm.argtypes = [i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
    lib.dh_debug_gemm.restype = i32
    lib.dh_debug_gemm_ln.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp]
    lib.dh_debug_gemm_ln.restype = i32
    lib.dh_debug_gemm_x6_ln.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp]
    lib.dh_debug_gemm_x6_ln.restype = i32
    lib.dh_debug_chain_x6.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, i32, vp, i32, vp]
    lib.dh_debug_chain_x6.restype = i32
    lib.dh_debug_gemm_lnch.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    lib.dh_debug_gemm_lnch.restype = i32
    lib.dh_debug_set_lnch_form.argtypes = [i32]
    lib.dh_debug_set_lnch_form.restype = i32
    lib.dh_debug_x6_plane_rows.argtypes = [i32]
    lib.dh_debug_x6_plane_rows.restype = i32
    lib.dh_debug_split_planes.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dh_debug_split_planes.restype = i32
    lib.dh_debug_gemm_x6.argtypes = [i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
    lib.dh_debug_gemm_x6.restype = i32
    lib.dh_debug_gemm_x6_choice.argtypes = [i32, i32]
    lib.dh_debug_gemm_x6_choice.restype = i32
    lib.dh_debug_route.argtypes = [vp, i32, i32, C.POINTER(i32), i32]
    lib.dh_debug_route.restype = i32
    lib.dh_debug_set_det_in_chain.argtypes = [i32]
    lib.dh_debug_set_det_in_chain.restype = i32
    lib.dh_debug_det_in_chain.argtypes = [vp, i32, i32]
    lib.dh_debug_det_in_chain.restype = i32
    lib.dh_ref_layout.argtypes = [vp, C.POINTER(sz), i32]
    lib.dh_ref_layout.restype = i32
    lib.dh_set_params_ref.argtypes = [vp, vp, sz, vp]
    lib.dh_set_params_ref.restype = i32
    lib.dh_vjp_workspace_bytes.argtypes = [vp, i32]
    lib.dh_vjp_workspace_bytes.restype = sz
    lib.dh_logpsi_vjp.argtypes = [vp, vp, i32, vp, vp, vp, vp, sz, vp]
    lib.dh_logpsi_vjp.restype = i32
    lib.dh_kfac_layout.argtypes = [vp, C.POINTER(sz), i32]
    lib.dh_kfac_layout.restype = i32
    lib.dh_kfac_workspace_bytes.argtypes = [vp, i32]
    lib.dh_kfac_workspace_bytes.restype = sz
    lib.dh_kfac_vjp.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.dh_kfac_vjp.restype = i32
    lib.dh_kfac_step.argtypes = [vp, vp, vp, f32, f32, vp, vp, f32, f32, f32, vp, vp, vp, sz, vp]
    lib.dh_kfac_step.restype = i32
    lib.dh_ntk_workspace_bytes.argtypes = [vp, i32]
    lib.dh_ntk_workspace_bytes.restype = sz
    lib.dh_ntk_tile_walkers.argtypes = [vp]
    lib.dh_ntk_tile_walkers.restype = i32
    lib.dh_ntk.argtypes = [vp, vp, i32, vp, vp, vp, vp, sz, vp]
    lib.dh_ntk.restype = i32
    lib.dh_ntk_part.argtypes = [vp, vp, i32, vp, vp, vp, vp, sz, i32, i32, vp]
    lib.dh_ntk_part.restype = i32
    lib.dh_ntk_mirror.argtypes = [vp, i32, vp]
    lib.dh_ntk_mirror.restype = i32
    lib.dh_ntk_owner.argtypes = [vp, i32, i32]
    lib.dh_ntk_owner.restype = i32
    lib.dh_minsr_matrix_workspace_bytes.argtypes = [i32]
    lib.dh_minsr_matrix_workspace_bytes.restype = sz
    lib.dh_minsr_matrix.argtypes = [vp, vp, i32, C.c_double, vp, vp, sz, vp]
    lib.dh_minsr_matrix.restype = i32
    lib.dh_ntk_jvp_workspace_bytes.argtypes = [vp, i32]
    lib.dh_ntk_jvp_workspace_bytes.restype = sz
    lib.dh_ntk_jvp.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, sz, i32, i32, vp]
    lib.dh_ntk_jvp.restype = i32
    lib.dh_fidelity_partial.argtypes = [vp, vp, i32, vp, vp]
    lib.dh_fidelity_partial.restype = i32
    lib.dh_fidelity_residual.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.dh_fidelity_residual.restype = i32
    lib.dh_ortho_partial.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.dh_ortho_partial.restype = i32
    lib.dh_ortho_residual.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.dh_ortho_residual.restype = i32
    pf = C.POINTER(C.c_float)  # the cap angles: a host array
    lib.dh_swap_classify.argtypes = [vp, i32, i32, i32, i32, pf, i32, vp, vp, vp]
    lib.dh_swap_classify.restype = i32
    lib.dh_swap_compact.argtypes = [vp, i32, i32, i32, i32, pf, i32, vp, vp, vp, vp, vp, sz, vp]
    lib.dh_swap_compact.restype = i32
    lib.dh_swap_reduce.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.dh_swap_reduce.restype = i32
    lib.dh_swap_workspace_bytes.argtypes = [i32, i32]
    lib.dh_swap_workspace_bytes.restype = sz
    lib.dh_rdm_norb.argtypes = [i32, i32]
    lib.dh_rdm_norb.restype = i32
    lib.dh_rdm_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.dh_rdm_workspace_bytes.restype = sz
    lib.dh_monopole_harmonics.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dh_monopole_harmonics.restype = i32
    lib.dh_rdm_displace.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.dh_rdm_displace.restype = i32
    lib.dh_rdm_accumulate.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]
    lib.dh_rdm_accumulate.restype = i32
    lib.dh_pair_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.dh_pair_workspace_bytes.restype = sz
    lib.dh_pair_displace.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    lib.dh_pair_displace.restype = i32
    lib.dh_pair_kernel.argtypes = [vp, i32, i32, vp, vp]
    lib.dh_pair_kernel.restype = i32
    lib.dh_pair_accumulate.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]
    lib.dh_pair_accumulate.restype = i32
    lib.dh_create_halperin.argtypes = [C.POINTER(DhConfig), i32, i32, i32, C.POINTER(vp)]
    lib.dh_create_halperin.restype = i32
    lib.dh_create_quasihole.argtypes = [C.POINTER(DhConfig), C.POINTER(DhQuasihole), C.POINTER(vp)]
    lib.dh_create_quasihole.restype = i32
    lib.dh_hole_table_bytes.argtypes = []
    lib.dh_hole_table_bytes.restype = sz
    lib.dh_hole_table.argtypes = [C.POINTER(DhConfig), C.POINTER(DhHoleConfigs), vp, sz]
    lib.dh_hole_table.restype = i32
    lib.dh_hole_workspace_bytes.argtypes = [i32, i32]
    lib.dh_hole_workspace_bytes.restype = sz
    lib.dh_hole_logs.argtypes = [C.POINTER(DhConfig), C.POINTER(DhHoleConfigs), vp, i32, vp, sz, vp, vp]
    lib.dh_hole_logs.restype = i32
    lib.dh_hole_gram.argtypes = [vp, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.dh_hole_gram.restype = i32
    lib.dh_subspace_workspace_bytes.argtypes = [i32, i32]
    lib.dh_subspace_workspace_bytes.restype = sz
    lib.dh_subspace_accumulate.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.dh_subspace_accumulate.restype = i32
    pi = C.POINTER(DhImpurity)  # the impurities: a host array
    lib.dh_impurity_check.argtypes = [pi, i32]
    lib.dh_impurity_check.restype = i32
    lib.dh_external_potential.argtypes = [vp, i32, i32, i32, C.c_double, pi, i32, vp, vp, vp]
    lib.dh_external_potential.restype = i32
    lib.dh_axis_histogram.argtypes = [vp, i32, i32, i32, C.c_double, C.c_double, i32, vp, vp]
    lib.dh_axis_histogram.restype = i32
    lib.dh_spin_workspace_bytes.argtypes = [i32, i32, i32]
    lib.dh_spin_workspace_bytes.restype = sz
    lib.dh_spin_exchange.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.dh_spin_exchange.restype = i32
    lib.dh_spin_ratios.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]
    lib.dh_spin_ratios.restype = i32
    lib.dh_spin_reduce.argtypes = [vp, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]
    lib.dh_spin_reduce.restype = i32
    lib.dh_sf_nlm.argtypes = [i32]
    lib.dh_sf_nlm.restype = i32
    lib.dh_sf_workspace_bytes.argtypes = [i32, i32, i32]
    lib.dh_sf_workspace_bytes.restype = sz
    lib.dh_sf_pairs.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.dh_sf_pairs.restype = i32
    lib.dh_sf_multipoles.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.dh_sf_multipoles.restype = i32
    lib.dh_sf_accumulate.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.dh_sf_accumulate.restype = i32
    lib.dh_grad_cotangent.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.dh_grad_cotangent.restype = i32
    lib.dh_adam_update.argtypes = [vp, vp, vp, vp, sz, f32, f32, f32, f32, i32, vp]
    lib.dh_adam_update.restype = i32
    lib.dh_mh_init.argtypes = [vp, vp, vp, i32, vp]
    lib.dh_mh_init.restype = i32
    lib.dh_mh_propose.argtypes = [vp, vp, i32, i32, f32, u64, u64, i64, vp, vp]
    lib.dh_mh_propose.restype = i32
    lib.dh_mh_accept.argtypes = [vp, vp, vp, vp, vp, i32, i32, u64, u64, i64, vp, vp]
    lib.dh_mh_accept.restype = i32
    lib.dh_kinetic_from_derivatives.argtypes = [vp, vp, vp, i32, i32, C.c_double, C.c_double, vp, vp, vp]
    lib.dh_kinetic_from_derivatives.restype = i32
    lib.dh_profile_enable.argtypes = [vp, i32]
    lib.dh_profile_enable.restype = i32
    lib.dh_profile_read.argtypes = [vp, C.POINTER(C.c_double), i32]
    lib.dh_profile_read.restype = i32
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().dh_last_error().decode(errors="replace")
        raise RuntimeError(f"deephall_amd error {rc}: {msg}")
