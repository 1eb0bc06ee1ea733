"""ctypes binding of ``libfemo_hip.so`` (include/femo_hip.h).

The product has no CPU fallback: if the shared library is missing, or a compute
entry point is called without a HIP device, an exception is raised -- nothing is
silently routed elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FEMO_LIB") or os.path.join(_HERE, "csrc", "libfemo_hip.so")    # FEMO_LIB: another build of the library (A/B measurements)

c_i64 = C.c_int64
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_f64p = C.POINTER(C.c_double)
H = C.c_void_p  # opaque handle

ABI_VERSION = 10            # include/femo_hip.h FEMO_ABI_VERSION
MESH_INFO_COUNT = 12
MESH_INFO_KEYS = ("tdim", "n_vert", "n_rows", "n_cell", "nnz", "sell_entries", "max_rowlen",
                  "max_valence", "n_slices", "visit_entries", "regular_slices", "short_slices")

PDE_POISSON = 0
PDE_NL_POISSON = 1
PDE_MASS = 2
PDE_EB_BEAM = 3
J_L2_TRACKING = 0
ELAST_SIMP = 0
ELAST_RAMP = 1
ELAST_INFO_KEYS = ("dim", "n_dof", "nnz", "sell_entries", "spmv_bytes")
ELAST_PC = {"jacobi": 0, "multilevel": 1}
ELAST_MAX_COLS = 8                # FEMO_ELAST_MAX_COLS: load cases of one batched product / solve
ELAST_MASS_LAWS = {"linear": 0, "du_olhoff": 1}    # FEMO_ELAST_MASS_LINEAR, FEMO_ELAST_MASS_DU_OLHOFF
ELAST_THERMAL_PRODUCTS = {"N": 0, "T_rho": 1, "T_temp": 2}    # FEMO_ELAST_THERMAL_N, _T_RHO, _T_TEMP
ELAST_PC_INFO_COUNT = 16          # [levels, lattice bytes, block builds, last build us, nodes per level ...]


class SolverOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_it", C.c_int32),
                ("zero_guess", C.c_int32), ("check_every", C.c_int32), ("pc", C.c_int32), ("atol_pc", C.c_double)]


class NewmarkParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("c_m", C.c_double), ("c_k", C.c_double)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32),
                ("residual_norm", C.c_double), ("pc_residual_norm", C.c_double), ("pc_rhs_norm", C.c_double),
                ("rhs_norm", C.c_double),
                ("solve_ms", C.c_double), ("spmv_ms", C.c_double),
                ("spmv_samples", C.c_int32), ("loop_allreduces", C.c_int32)]


class EigOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("pcg_rtol", C.c_double), ("max_outer", C.c_int32), ("pcg_max_it", C.c_int32),
                ("pc", C.c_int32), ("reserved", C.c_int32)]


class EigInfo(C.Structure):
    _fields_ = [("outer_iterations", C.c_int32), ("pcg_iterations", C.c_int32), ("converged", C.c_int32),
                ("reserved", C.c_int32), ("residual", C.c_double * ELAST_MAX_COLS), ("solve_ms", C.c_double)]


MMA_MAX_M = 8                     # FEMO_MMA_MAX_M: general constraints of one MMA handle


class MmaParams(C.Structure):
    _fields_ = [("move", C.c_double), ("sub_tol", C.c_double), ("c", C.c_double * MMA_MAX_M), ("d", C.c_double * MMA_MAX_M)]


class MmaInfo(C.Structure):
    _fields_ = [("converged", C.c_int32), ("step", C.c_int32), ("stages", C.c_int32), ("newton_steps", C.c_int32),
                ("halvings", C.c_int32), ("blocking_copies", C.c_int32), ("residual_max", C.c_double), ("max_dx", C.c_double),
                ("max_dx_rel", C.c_double), ("update_ms", C.c_double), ("lam", C.c_double * MMA_MAX_M), ("y", C.c_double * MMA_MAX_M)]


PROJECT_FIXED, PROJECT_VOLUME = 0, 1     # FEMO_PROJECT_FIXED / FEMO_PROJECT_VOLUME


class ProjectInfo(C.Structure):
    _fields_ = [("eta", C.c_double), ("vol_in", C.c_double), ("vol_out", C.c_double), ("s_v", C.c_double), ("ms", C.c_double),
                ("flat", C.c_int32), ("mode", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32)]


class HostStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("h2d_pinned", "h2d_pinned_bytes", "h2d_staged", "h2d_staged_bytes",
                                         "h2d_skipped", "h2d_skipped_bytes", "h2d_as_d2d", "h2d_as_d2d_bytes",
                                         "d2h_pinned", "d2h_pinned_bytes", "d2h_staged", "d2h_staged_bytes",
                                         "d2h_async", "d2h_async_bytes", "d2h_device_sum", "d2h_device_sum_bytes",
                                         "h2d_deferred", "h2d_deferred_bytes",
                                         # appended with femo_mesh_head_info: a build without it leaves the field at 0 (the
                                         # library fills the struct it knows; engine.host_stats reports the field only when bound)
                                         "h2d_chunks",
                                         # appended with femo_vec_get_host_promised_ex: the pool's own bookkeeping
                                         "pool_fresh", "pool_fresh_us", "pool_free_deferred", "pool_free_waited",
                                         "pool_free_waited_us")]


# name -> (restype, argtypes); every symbol include/femo_hip.h declares
PROTOTYPES = {
    "femo_last_error": (C.c_char_p, []),
    "femo_abi_version": (C.c_int, []),
    "femo_host_sync_stats": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
    "femo_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "femo_ctx_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(H)]),
    "femo_ctx_destroy": (C.c_int, [H]),
    "femo_ctx_sync": (C.c_int, [H]),
    "femo_ctx_stream": (C.c_void_p, [H]),
    "femo_vec_create": (C.c_int, [H, c_i64, C.POINTER(H)]),
    "femo_vec_wrap": (C.c_int, [H, C.c_void_p, c_i64, C.POINTER(H)]),
    "femo_vec_destroy": (C.c_int, [H]),
    "femo_vec_size": (c_i64, [H]),
    "femo_vec_device_ptr": (C.c_void_p, [H]),
    "femo_vec_device_ptr_const": (C.c_void_p, [H]),
    "femo_vec_set_host": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_get_host": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_add_to_host": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_get_host_async": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_get_host_promised": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_get_host_promised_ex": (C.c_int, [H, C.c_void_p, c_i64, C.c_int]),
    "femo_host_forget": (C.c_int, [C.c_void_p]),
    "femo_range_plan_host": (C.c_int, [c_i64, c_i64, C.c_int, c_i64, c_i64, c_i64, C.POINTER(c_i64), c_i64]),
    "femo_vec_set_host_deferred": (C.c_int, [H, C.c_void_p, c_i64]),
    "femo_vec_await_upload": (C.c_int, [H]),
    "femo_host_wait": (C.c_int, [C.c_void_p]),
    "femo_host_sync": (C.c_int, []),
    "femo_host_alloc": (C.c_int, [c_i64, C.POINTER(C.c_void_p)]),
    "femo_host_free": (C.c_int, [C.c_void_p]),
    "femo_host_trim": (C.c_int, []),
    "femo_host_register": (C.c_int, [C.c_void_p, c_i64]),
    "femo_host_unregister": (C.c_int, [C.c_void_p]),
    "femo_host_touch": (C.c_int, [C.c_void_p]),
    "femo_host_fill": (C.c_int, [C.c_void_p, c_i64, C.c_double]),
    "femo_host_is_pinned": (C.c_int, [C.c_void_p, c_i64]),
    "femo_host_threads": (C.c_int, []),
    "femo_host_copy": (C.c_int, [C.c_void_p, C.c_void_p, c_i64]),
    "femo_host_axpby": (C.c_int, [c_i64, C.c_double, C.c_void_p, C.c_double, C.c_void_p]),
    "femo_host_get_stats": (C.c_int, [C.POINTER(HostStats)]),
    "femo_host_reset_stats": (C.c_int, []),
    "femo_vec_fill": (C.c_int, [H, C.c_double]),
    "femo_vec_copy": (C.c_int, [H, H]),
    "femo_vec_axpy": (C.c_int, [H, C.c_double, H]),
    "femo_vec_dot": (C.c_int, [H, H, c_i64, c_f64p]),
    "femo_vec_dots": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i64, c_f64p]),
    "femo_vec_dots_rhs": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_i64, c_f64p, H, H]),
    "femo_mat_identity_solve": (C.c_int, [H, H, H]),
    "femo_mat_identity_solve_flag": (C.c_int, [H, H, H]),
    "femo_vec_axpy_if": (C.c_int, [H, C.c_double, H]),
    "femo_newton_rhs_linear_if": (C.c_int, [H, H, H, H, H]),
    "femo_ctx_newton_flag_info": (C.c_int, [H, c_i64p, C.c_int]),
    "femo_mesh_create": (C.c_int, [H, C.c_int, c_i64, c_i64, C.c_void_p, c_i64, C.c_void_p, C.POINTER(H)]),
    "femo_mesh_destroy": (C.c_int, [H]),
    "femo_mesh_info": (C.c_int, [H, c_i64p]),
    "femo_mesh_set_boundary_facets": (C.c_int, [H, C.c_void_p]),
    "femo_pc_plan_host": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                          C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_emu_group_create": (C.c_int, [C.c_int, C.POINTER(H)]),
    "femo_emu_group_destroy": (C.c_int, [H]),
    "femo_comm_emulate": (C.c_int, [H, H, C.c_int]),
    "femo_comm_model": (C.c_int, [H, C.c_int, C.c_int]),
    "femo_comm_stats": (C.c_int, [H, C.POINTER(C.c_int64), C.c_int]),
    "femo_mesh_pcg_info": (C.c_int, [H, C.POINTER(C.c_int64), C.c_int]),
    "femo_mesh_head_info": (C.c_int, [H, C.POINTER(C.c_int64), C.c_int]),
    "femo_mesh_tail_info": (C.c_int, [H, C.POINTER(C.c_int64), C.c_int]),
    "femo_mat_compact_info": (C.c_int, [H, C.POINTER(C.c_int64), C.c_int]),
    "femo_mat_spmv_scaled": (C.c_int, [H, C.c_int, H, H, c_f64p, C.POINTER(C.c_int)]),
    "femo_mat_import_csr": (C.c_int, [H, C.c_void_p]),
    # Reissner-Mindlin shell
    "femo_shell_create": (C.c_int, [H, c_i64, C.c_void_p, c_i64, C.c_void_p, c_i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(H)]),
    "femo_shell_destroy": (C.c_int, [H]),
    "femo_shell_pc_create": (C.c_int, [H, C.c_int, c_i64, C.c_int, C.c_void_p] + [C.c_void_p] * 11),
    "femo_shell_pc_coarse": (C.c_int, [H, C.c_int, C.c_void_p, c_i64] + [C.c_void_p] * 6),
    "femo_shell_pc_coarse_matrix": (C.c_int, [H, H, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(c_i64)]),
    "femo_shell_pc_hermite": (C.c_int, [H] + [C.c_void_p] * 11),
    "femo_shell_pc_info": (C.c_int, [H, C.POINTER(C.c_int32)]),
    "femo_shell_pc_block_items": (C.c_int, [H, C.c_int64] + [C.c_void_p] * 4),
    "femo_shell_pc_weights": (C.c_int, [H, C.c_double, C.c_double]),
    "femo_shell_pc_apply": (C.c_int, [H, H, C.c_void_p, H, H]),
    "femo_shell_pnorm_stress": (C.c_int, [H, C.c_double, C.c_double, H, H, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.POINTER(C.c_double), C.c_int, H, H]),
    "femo_shell_vm_rhs": (C.c_int, [H, C.c_double, C.c_double, H, H, C.c_double, H, H]),
    "femo_shell_p1_mass": (C.c_int, [H, H, H]),
    "femo_shell_ndof": (c_i64, [H]),
    "femo_shell_nnz": (c_i64, [H]),
    "femo_shell_assemble": (C.c_int, [H, C.c_double, C.c_double, H, H]),
    "femo_shell_matvec": (C.c_int, [H, H, C.c_void_p, H, H]),
    "femo_shell_load": (C.c_int, [H, H, C.c_double, C.c_int, H]),
    "femo_shell_load_T": (C.c_int, [H, H, C.c_double, C.c_int, H]),
    "femo_shell_dform_dh": (C.c_int, [H, C.c_double, C.c_double, H, H, H, C.c_int, H, C.POINTER(C.c_double)]),
    "femo_shell_compliance": (C.c_int, [H, H, C.POINTER(C.c_double), C.c_int, H]),
    "femo_shell_mass": (C.c_int, [H, C.c_double, H, C.POINTER(C.c_double), C.c_int, H]),
    "femo_shell_compliance_dx": (C.c_int, [H, H, H, C.POINTER(C.c_double), C.c_int, H]),
    "femo_shell_regularization": (C.c_int, [H, C.c_int, H, C.POINTER(C.c_double), C.c_int, H]),
    "femo_shell_hpower": (C.c_int, [H, C.c_double, C.c_double, H, C.POINTER(C.c_double), C.c_int, H]),
    "femo_shell_set_penalty": (C.c_int, [H, c_i64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_shell_penalty_add": (C.c_int, [H, H]),
    "femo_shell_penalty_apply": (C.c_int, [H, H, H, C.c_int, H]),
    "femo_shell_inertia_apply": (C.c_int, [H, C.c_double, H, H, C.c_int, H]),
    "femo_shell_inertia_dh": (C.c_int, [H, C.c_double, H, H, H, C.c_int, H]),
    "femo_shell_inertia_dh_fwd": (C.c_int, [H, C.c_double, H, H, H, C.c_int, H]),
    "femo_shell_dform_dh_fwd": (C.c_int, [H, C.c_double, C.c_double, H, H, H, C.c_int, H]),
    "femo_shell_solve": (C.c_int, [H, H, C.c_void_p, H, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_shell_set_partition": (C.c_int, [H, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_shell_set_owned_cells": (C.c_int, [H, C.c_void_p]),
    "femo_shell_halo": (C.c_int, [H, H]),
    "femo_shell_mask_unowned": (C.c_int, [H, H]),
    "femo_mesh_set_global": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64]),
    "femo_mesh_pc_info": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "femo_mesh_pattern_csr": (C.c_int, [H, C.c_void_p, C.c_void_p]),
    "femo_topology_build_host": (C.c_int, [C.c_int, c_i64, c_i64, c_i64, C.c_void_p, c_i64p, C.c_void_p, C.c_void_p]),
    "femo_bc_create": (C.c_int, [H, c_i64, C.c_void_p, C.c_void_p, C.POINTER(H)]),
    "femo_bc_destroy": (C.c_int, [H]),
    "femo_assemble_residual": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, H]),
    "femo_mat_create": (C.c_int, [H, C.POINTER(H)]),
    "femo_mat_destroy": (C.c_int, [H]),
    "femo_assemble_jacobian": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, H, H]),
    "femo_assemble_dRdf": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H]),
    "femo_assemble_system": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, H, H, H, H]),
    "femo_bc_apply_rhs": (C.c_int, [H, H, H]),
    "femo_newton_rhs": (C.c_int, [H, H, H, H, H]),
    "femo_newton_rhs_linear": (C.c_int, [H, H, H, H, H]),
    "femo_mat_spmv": (C.c_int, [H, C.c_int, H, H]),
    "femo_dRdf_apply": (C.c_int, [H, H, C.c_int, H, H, C.c_int]),
    "femo_assemble_dRdf_cell": (C.c_int, [H, C.c_int, C.c_void_p, H]),
    "femo_dRdf_cell_apply": (C.c_int, [H, H, C.c_int, H, H, C.c_int]),
    "femo_dRdf_cell_apply_T_add_to_host": (C.c_int, [H, H, H, H, C.c_void_p, c_i64]),
    "femo_mat_export_csr": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_mat_diagonal": (C.c_int, [H, H]),
    "femo_mat_prescale": (C.c_int, [H]),
    "femo_solve_cg": (C.c_int, [H, C.c_int, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_mat_pc_apply": (C.c_int, [H, H, H]),
    "femo_solve_bicgstab": (C.c_int, [H, C.c_int, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_functional_value": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, c_f64p]),
    "femo_functional_grad_u": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, H]),
    "femo_functional_grad_f": (C.c_int, [H, C.c_int, C.c_void_p, H, H, H, H]),
    "femo_cell_expression": (C.c_int, [H, C.c_int, C.c_void_p, H, H]),
    "femo_vec_pointwise_divide": (C.c_int, [H, H, H, c_i64]),
    "femo_bench_spmv": (C.c_int, [H, H, H, C.c_int, c_f64p]),
    "femo_comm_unique_id": (C.c_int, [C.c_char_p]),
    "femo_comm_init": (C.c_int, [H, C.c_char_p, C.c_int, C.c_int]),
    "femo_comm_rank": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "femo_mesh_set_halo": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_halo_exchange": (C.c_int, [H, H]),
    "femo_mesh_halo_direct_export": (C.c_int, [H, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "femo_mesh_halo_direct_connect": (C.c_int, [H, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_mesh_halo_direct_selftest": (C.c_int, [H, C.POINTER(C.c_int)]),
    "femo_mesh_halo_direct_enable": (C.c_int, [H, C.c_int]),
    "femo_mesh_halo_direct_info": (C.c_int, [H, C.POINTER(C.c_int64)]),
    "femo_allreduce_sum": (C.c_int, [H, c_f64p, C.c_int]),
    # SIMP topology optimisation: vector CG1 elasticity and the DG0 density filter
    "femo_elast_create": (C.c_int, [H, C.c_double, C.c_double, C.POINTER(H)]),
    "femo_elast_destroy": (C.c_int, [H]),
    "femo_elast_info": (C.c_int, [H, c_i64p]),
    "femo_elast_set_fixed": (C.c_int, [H, C.c_void_p]),
    "femo_elast_set_springs": (C.c_int, [H, C.c_void_p]),
    "femo_elast_set_facets": (C.c_int, [H, c_i64, C.c_void_p]),
    "femo_elast_assemble": (C.c_int, [H, C.c_int, H]),
    "femo_elast_apply": (C.c_int, [H, C.c_int, C.c_double, H, C.c_double, H, H]),
    "femo_elast_load": (C.c_int, [H, c_f64p, H]),
    "femo_elast_drho": (C.c_int, [H, C.c_int, C.c_int, H, H, H, H, C.c_int]),
    "femo_elast_pnorm_stress": (C.c_int, [H, H, H, C.c_double, C.c_double, C.c_double, C.c_double, c_f64p, H, H, C.c_int]),
    "femo_elast_von_mises": (C.c_int, [H, H, H, C.c_double, H]),
    "femo_elast_solve": (C.c_int, [H, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_elast_apply_multi": (C.c_int, [H, C.c_int, C.c_int, C.c_double, H, C.c_double, H, H]),
    "femo_elast_solve_multi": (C.c_int, [H, C.c_int, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_elast_drho_multi": (C.c_int, [H, C.c_int, C.c_int, C.c_int, H, H, H, H, C.c_int]),
    "femo_elast_pnorm_stress_multi": (C.c_int, [H, C.c_int, H, H, c_f64p, c_f64p, C.c_double, C.c_double, C.c_double, c_f64p,
                                                H, H, C.c_int]),
    "femo_elast_von_mises_multi": (C.c_int, [H, C.c_int, H, H, c_f64p, C.c_double, C.c_int, H]),
    "femo_elast_pnorm_disp_multi": (C.c_int, [H, C.c_int, H, H, c_f64p, c_f64p, C.c_double, C.c_double, c_f64p, H, C.c_int]),
    "femo_elast_body_apply": (C.c_int, [H, C.c_int, c_f64p, C.c_int, C.c_double, H, H, C.c_int, H, C.c_int]),
    "femo_elast_thermal_apply": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_f64p, C.c_double, H, H, C.c_double, C.c_double,
                                           C.c_double, H, H, C.c_int, H, C.c_int]),
    "femo_elast_mass_apply_multi": (C.c_int, [H, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, H, H, H]),
    "femo_elast_block_gram": (C.c_int, [H, C.c_int, H, C.c_int, H, c_f64p]),
    "femo_elast_block_rotate": (C.c_int, [H, C.c_int, c_f64p, H, H]),
    "femo_elast_eig_drho": (C.c_int, [H, C.c_int, C.c_int, C.c_double, C.c_int, H, H, c_f64p, c_f64p, H, C.c_int]),
    "femo_elast_eigs": (C.c_int, [H, C.c_int, C.c_double, H, C.c_int, C.c_int, H, C.POINTER(EigOpts), c_f64p,
                                  C.POINTER(EigInfo)]),
    "femo_elast_geom_stress": (C.c_int, [H, C.c_int, H, H]),
    "femo_elast_geom_stress_get": (C.c_int, [H, H]),
    "femo_elast_geom_apply_multi": (C.c_int, [H, C.c_int, C.c_int, C.c_double, H, H]),
    "femo_elast_buckle_du": (C.c_int, [H, C.c_int, C.c_int, H, H, c_f64p, H]),
    "femo_elast_buckle_drho": (C.c_int, [H, C.c_int, C.c_int, H, H, H, c_f64p, c_f64p, H, C.c_int]),
    "femo_elast_buckle": (C.c_int, [H, C.c_int, H, H, C.c_int, C.c_int, H, C.POINTER(EigOpts), c_f64p, C.POINTER(EigInfo)]),
    "femo_elast_mass_assemble": (C.c_int, [H, C.c_int, C.c_double, H]),
    "femo_elast_dyn_apply_multi": (C.c_int, [H, C.c_int, C.c_int, c_f64p, C.c_double, H, C.c_double, H, H]),
    "femo_elast_dyn_solve_multi": (C.c_int, [H, C.c_int, c_f64p, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_elast_cdyn_apply_multi": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_f64p, c_f64p, c_f64p, C.c_double, H, C.c_double, H, H]),
    "femo_elast_cdyn_solve_multi": (C.c_int, [H, C.c_int, C.c_int, c_f64p, c_f64p, c_f64p, H, H, C.POINTER(SolverOpts),
                                              C.POINTER(SolveInfo)]),
    "femo_elast_mass_drho_multi": (C.c_int, [H, C.c_int, C.c_double, C.c_int, C.c_int, c_f64p, H, H, H, H, C.c_int]),
    "femo_elast_newmark_rhs": (C.c_int, [H, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, H, H, H]),
    "femo_elast_newmark_march": (C.c_int, [H, C.POINTER(NewmarkParams), C.c_int, C.c_int, H, H, c_f64p, H, C.POINTER(SolverOpts),
                                           C.c_int, C.POINTER(SolveInfo), C.POINTER(C.c_int32)]),
    "femo_elast_newmark_apply": (C.c_int, [H, C.POINTER(NewmarkParams), C.c_int, C.c_int, C.c_int, H, H]),
    "femo_elast_newmark_drho": (C.c_int, [H, C.POINTER(NewmarkParams), C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                          C.c_int, H, H, H, H, C.c_int]),
    "femo_elast_newmark_dots": (C.c_int, [H, C.c_int, H, H, c_f64p]),
    "femo_elast_newmark_outer": (C.c_int, [H, C.c_int, c_f64p, H, H]),
    "femo_elast_export_csr": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_elast_pc_setup": (C.c_int, [H, C.c_double]),
    "femo_elast_pc_info": (C.c_int, [H, c_i64p]),
    "femo_elast_pc_export_level": (C.c_int, [H, C.c_int, C.c_void_p]),
    "femo_elast_pc_apply": (C.c_int, [H, H, H]),
    "femo_elast_bench_spmv": (C.c_int, [H, H, H, C.c_int, c_f64p]),
    "femo_filter_create": (C.c_int, [H, C.c_int, c_i64, C.c_void_p, C.c_double, C.POINTER(H)]),
    "femo_filter_destroy": (C.c_int, [H]),
    "femo_filter_nnz": (C.c_int, [H, c_i64p]),
    "femo_filter_apply": (C.c_int, [H, C.c_int, H, H]),
    "femo_filter_export_csr": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # Helmholtz (PDE) density filter (csrc/pde_filter.hip)
    "femo_pde_filter_create": (C.c_int, [H, C.c_double, C.c_int, C.POINTER(H)]),
    "femo_pde_filter_destroy": (C.c_int, [H]),
    "femo_pde_filter_apply": (C.c_int, [H, C.c_int, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_pde_filter_set": (C.c_int, [H, C.c_double, C.c_int]),
    "femo_pde_filter_export_csr": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p]),
    "femo_pde_filter_bytes": (C.c_int, [H, c_i64p]),
    "femo_pde_filter_project": (C.c_int, [H, H, H, H, H, C.POINTER(ProjectInfo)]),
    # heat conduction with a penalised conductivity (csrc/conduction.hip)
    "femo_cond_create": (C.c_int, [H, C.POINTER(H)]),
    "femo_cond_destroy": (C.c_int, [H]),
    "femo_cond_assemble": (C.c_int, [H, C.c_int, C.c_double, C.c_double, H, H]),
    "femo_cond_apply": (C.c_int, [H, C.c_int, H, H]),
    "femo_cond_lift": (C.c_int, [H, H, H, H, H]),
    "femo_cond_solve": (C.c_int, [H, H, H, C.POINTER(SolverOpts), C.POINTER(SolveInfo)]),
    "femo_cond_pc_apply": (C.c_int, [H, H, H]),
    "femo_cond_pc_info": (C.c_int, [H, C.c_void_p, C.c_int]),
    "femo_cond_pc_export_level": (C.c_int, [H, C.c_int, C.c_void_p]),
    "femo_cond_drho": (C.c_int, [H, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, H, H, H, H, C.c_int]),
    "femo_cond_export_csr": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # Method of Moving Asymptotes (csrc/mma.hip)
    "femo_mma_create": (C.c_int, [H, c_i64, C.c_int, H, H, C.POINTER(MmaParams), C.POINTER(H)]),
    "femo_mma_update": (C.c_int, [H, H, C.c_double, H, c_f64p, H, C.POINTER(MmaInfo)]),
    "femo_mma_reset": (C.c_int, [H]),
    "femo_mma_destroy": (C.c_int, [H]),
    "femo_mma_get": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p]),
    "femo_mma_solve_subproblem": (C.c_int, [H] + [C.c_void_p] * 11 + [C.POINTER(MmaInfo)]),
    # Heaviside projection, passive cells, volume-preserving threshold (csrc/project.hip)
    "femo_project_create": (C.c_int, [H, c_i64, C.c_void_p, c_i64, C.c_void_p, c_i64, C.c_void_p, C.c_double, C.c_double,
                                      C.c_double, C.c_int, C.POINTER(H)]),
    "femo_project_destroy": (C.c_int, [H]),
    "femo_project_set": (C.c_int, [H, C.c_double, C.c_double, C.c_int]),
    "femo_project_forward": (C.c_int, [H, H, H, C.POINTER(ProjectInfo)]),
    "femo_filter_project": (C.c_int, [H, H, H, H, H, C.POINTER(ProjectInfo)]),
    "femo_project_reverse": (C.c_int, [H, H, H, H]),
    "femo_project_tangent": (C.c_int, [H, H, H, H]),
    "femo_project_grayness": (C.c_int, [H, H, C.POINTER(C.c_double)]),
}


# test-only entry points that an older build selected through FEMO_LIB (A/B measurements against a parent commit) may lack:
# they stay unbound there and their wrappers raise
# (and Newton's flagged passes: without them utils_hip takes the plain entry points, as under FEMO_NEWTON_FLAG=0; the
# streamed tail and results on demand: without them the product + add_to_host and the eager asynchronous copy-out)
OPTIONAL = frozenset({"femo_mesh_pcg_info", "femo_mesh_head_info", "femo_mat_identity_solve_flag", "femo_vec_axpy_if",
                      "femo_newton_rhs_linear_if", "femo_ctx_newton_flag_info", "femo_mesh_tail_info",
                      "femo_dRdf_cell_apply_T_add_to_host", "femo_vec_get_host_promised", "femo_host_forget",
                      "femo_vec_get_host_promised_ex", "femo_range_plan_host",
                      "femo_mat_compact_info", "femo_mat_spmv_scaled", "femo_mat_import_csr"})


class FemoError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libfemo_hip.so and bind every prototype.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FemoError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C femo_amd/csrc`).  femo_amd has no CPU fallback.")
    # A context drives three HIP streams (compute, copies, neighbour exchange) and RCCL adds its own.  The HIP runtime maps
    # streams onto GPU_MAX_HW_QUEUES hardware queues (default 4): streams that SHARE a queue serialise -- a copy stream's wait
    # for a 60 MB PCIe transfer then holds up the compute stream behind it (round 6: measured on the model rank of the
    # scaling model, whose process keeps two contexts alive: 2.4 ms of a 12.5 ms cycle).  Ask for 8 unless the user has set
    # the variable; it is read when the HIP runtime initialises, i.e. before the first HIP call of the process.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        if name in OPTIONAL and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if lib.femo_abi_version() != ABI_VERSION:
        raise FemoError("libfemo_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().femo_last_error()
        raise FemoError(msg.decode() if msg else f"libfemo_hip error {rc}")


def device_count() -> int:
    n = C.c_int(0)
    rc = load().femo_device_count(C.byref(n))
    return n.value if rc == 0 else 0
