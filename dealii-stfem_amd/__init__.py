"""dealii-stfem_amd: MI355X-native matrix-free space-time operator apply.

Python is only a thin ctypes veneer over the C-ABI in include/stfem.h (libstfem_hip.so, built
from csrc/ by `make -C dealii-stfem_amd/csrc`).  The classes keep the reference's names
(`MatrixFreeOperator`, `SystemMatrix`, include/operators.h:967-1191, 517-663) so tests and
bench.py read like the reference's callers.  There is NO CPU fallback: if the HIP library is
missing or no GPU is present, construction raises.

Import with  importlib.import_module("dealii-stfem_amd")  (the hyphen is the package name the
build contract prescribes).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstfem_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem.h")

CGP, DG = 0, 1


class StfemError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().stfem_strerror(status).decode()
        why = lib().stfem_last_error().decode()
        super().__init__(f"{what}: {msg} ({status})" + (f" [{why}]" if why else ""))


def build(force=False):
    """Compile libstfem_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


class _MeshDesc(C.Structure):
    _fields_ = [("ncell", C.c_int32 * 3), ("vertices", C.POINTER(C.c_double)),
                ("lower", C.c_double * 3), ("upper", C.c_double * 3),
                ("dirichlet_mask", C.c_int32), ("device", C.c_int32)]


class _SpaceDesc(C.Structure):
    _fields_ = [("degree", C.c_int32), ("n_q_points_1d", C.c_int32), ("n_components", C.c_int32),
                ("precision", C.c_int32)]


class _StokesSpaceDesc(C.Structure):
    _fields_ = [("velocity_degree", C.c_int32), ("pressure_space", C.c_int32), ("viscosity", C.c_double),
                ("reserved", C.c_int32 * 4)]


class _StokesVankaSpaceDesc(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("block_variable", C.POINTER(C.c_int32)), ("Alpha", C.POINTER(C.c_double)),
                ("Beta", C.POINTER(C.c_double)), ("reserved", C.c_int32 * 4)]


class _StokesVankaLinearisedSpaceDesc(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("block_variable", C.POINTER(C.c_int32)), ("Alpha", C.POINTER(C.c_double)),
                ("Beta", C.POINTER(C.c_double)), ("mode", C.c_int32), ("lin_blocks", C.POINTER(C.c_void_p)),
                ("reserved", C.c_int32 * 4)]


_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
_lib = None

# every symbol include/stfem.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "stfem_ctx_create": (C.c_int, [C.POINTER(_MeshDesc), C.POINTER(_SpaceDesc), C.POINTER(_vp)]),
    "stfem_ctx_destroy": (None, [_vp]),
    "stfem_n_dofs": (C.c_int64, [_vp]),
    "stfem_n_cells": (C.c_int64, [_vp]),
    "stfem_is_cartesian": (C.c_int, [_vp]),
    "stfem_ctx_precision": (C.c_int, [_vp]),
    "stfem_set_coefficient": (C.c_int, [_vp, C.c_int, C.c_int, _dp]),
    "stfem_vector_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "stfem_vector_wrap": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    "stfem_vector_rebind": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "stfem_vector_destroy": (None, [_vp]),
    "stfem_vector_n_blocks": (C.c_int, [_vp]),
    "stfem_vector_block": (_vp, [_vp, C.c_int]),
    "stfem_vector_upload": (C.c_int, [_vp, C.POINTER(_dp)]),
    "stfem_vector_download": (C.c_int, [_vp, C.POINTER(_dp)]),
    "stfem_st_vmult": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "stfem_space_vmult": (C.c_int, [_vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    "stfem_diagonal": (C.c_int, [_vp, C.c_double, C.c_double, _vp, _vp]),
    "stfem_tensorproduct_add": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _vp, _vp, _vp]),
    "stfem_dot": (C.c_int, [_vp, _vp, _vp, C.c_int64, _dp, _vp]),
    "stfem_trace_push": (None, [C.c_char_p]),
    "stfem_trace_pop": (None, []),
    "stfem_multi_dot": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _vp, C.c_int64, _dp, _vp]),
    "stfem_multi_axpy": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(_vp), _vp, _vp]),
    "stfem_orthogonalize": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _vp, C.c_int64, _dp, _dp, _dp, _vp]),
    "stfem_diagonal_inverse": (C.c_int, [_vp, C.c_double, C.c_double, _vp, _vp]),
    "stfem_st_diagonal": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, _vp, _vp]),
    "stfem_plane_pack": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "stfem_plane_unpack": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp]),
    "stfem_n_dofs_1d": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "stfem_comm_get_unique_id": (C.c_int, [_vp]),
    "stfem_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "stfem_comm_destroy": (None, [_vp]),
    "stfem_comm_available": (C.c_int, []),
    "stfem_comm_rccl_count": (C.c_int, [_vp]),
    "stfem_comm_rank": (C.c_int, [_vp]),
    "stfem_comm_size": (C.c_int, [_vp]),
    "stfem_comm_last_error": (C.c_char_p, []),
    "stfem_ghost_update": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "stfem_halo_begin": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "stfem_neighbour_exchange": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "stfem_halo_end": (C.c_int, [_vp, _vp, _vp, _vp]),
    "stfem_halo_begin_split": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "stfem_planes_move": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "stfem_dot_global": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _dp, _vp]),
    "stfem_support_points": (C.c_int, [_vp, _dp]),
    "stfem_quadrature_points": (C.c_int, [_vp, C.c_int, _dp]),
    "stfem_integrate_rhs": (C.c_int, [_vp, C.c_int, _dp, _vp, C.c_int, _vp]),
    "stfem_integrate_difference": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _dp, _dp, _dp, _vp]),
    "stfem_integrate_rhs_product": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double, _vp, C.c_int, _vp]),
    "stfem_integrate_difference_product": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, _dp, _vp]),
    "stfem_vector_axpby": (C.c_int, [_vp, C.c_double, _vp, C.c_double, _vp, _vp]),
    "stfem_vector_set_zero": (C.c_int, [_vp, _vp, _vp]),
    "stfem_axpby_many": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64), C.c_double, C.POINTER(_vp), C.c_double, C.POINTER(_vp), _vp]),
    "stfem_driver_last_error": (C.c_char_p, []),
    "stfem_gauss_rule": (C.c_int, [C.c_int, _dp, _dp]),
    "stfem_fe_time_points": (C.c_int, [C.c_int, C.c_int, _dp]),
    "stfem_time_prolongation_matrix": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int32)]),
    "stfem_time_restriction_matrix": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int32)]),
    "stfem_time_projection_matrix": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int32)]),
    "stfem_time_evaluation_matrix": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int32)]),
    "stfem_poly_mg_sequence": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stfem_mg_sequence": (C.c_int, [C.c_int] * 5 + [C.c_char] + [C.c_int] * 4 + [C.c_char_p, C.POINTER(C.c_int32)]),
    "stfem_precondition_stmg_types": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "stfem_transfer_create": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "stfem_transfer_create_partitioned": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "stfem_transfer_destroy": (None, [_vp]),
    "stfem_transfer_prolongate": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "stfem_transfer_restrict": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "stfem_transfer_interpolate": (C.c_int, [_vp, _vp, _vp, _vp]),
    "stfem_transfer_last_error": (C.c_char_p, []),
    "stfem_transfer_last_path": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "stfem_transfer_line_matrices": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "stfem_vector_convert": (C.c_int, [_vp, _vp, _vp]),
    "stfem_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "stfem_stream_destroy": (None, [_vp]),
    "stfem_stream_synchronize": (C.c_int, [_vp]),
    "stfem_graph_begin": (C.c_int, [_vp]),
    "stfem_graph_end": (C.c_int, [_vp, C.POINTER(_vp)]),
    "stfem_graph_launch": (C.c_int, [_vp, _vp]),
    "stfem_graph_destroy": (None, [_vp]),
    "stfem_vanka_create": (C.c_int, [_vp, C.c_int, _dp, _dp, C.POINTER(_vp)]),
    "stfem_vanka_create_partitioned": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_int, C.POINTER(_vp)]),
    "stfem_vanka_create_partitioned_general": (C.c_int, [_vp, _vp, C.c_int, _dp, _dp, C.c_int, C.POINTER(_vp)]),
    "stfem_vanka_destroy": (None, [_vp]),
    "stfem_vanka_n_classes": (C.c_int, [_vp]),
    "stfem_vanka_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "stfem_vanka_setup_batches": (C.c_int, [_vp]),
    "stfem_vanka_vmult": (C.c_int, [_vp, _vp, _vp, _vp]),
    "stfem_vanka_step": (C.c_int, [_vp, _vp, C.c_double, C.c_int, _vp, _vp]),
    "stfem_vanka_last_error": (C.c_char_p, []),
    "stfem_fe_time_weights": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp, _dp]),
    "stfem_fe_time_weights_wave": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_int,
                                             _dp, _dp, _dp, _dp, _dp]),
    "stfem_mesh_vertices": (C.c_int, [C.POINTER(C.c_int32), _dp, _dp, C.c_double, C.c_uint64,
                                      C.c_int32, C.c_int32, _dp]),
    "stfem_coefficient_per_cell": (C.c_int, [C.POINTER(C.c_int32), _dp, C.c_double, C.c_double,
                                             C.c_double, C.c_double, C.POINTER(C.c_int32), _dp,
                                             _dp, _dp]),
    "stfem_stokes_create": (C.c_int, [C.POINTER(_MeshDesc), C.c_int, C.c_double, C.POINTER(_vp)]),
    "stfem_stokes_create_ex": (C.c_int, [C.POINTER(_MeshDesc), C.c_int, C.c_int, C.c_double, C.POINTER(_vp)]),
    "stfem_stokes_destroy": (None, [_vp]),
    "stfem_stokes_n_velocity_dofs": (C.c_int64, [_vp]),
    "stfem_stokes_n_pressure_dofs": (C.c_int64, [_vp]),
    "stfem_stokes_vector_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "stfem_stokes_vector_destroy": (None, [_vp, _vp]),
    "stfem_stokes_vector_upload": (C.c_int, [_vp, C.c_int, _vp, _dp]),
    "stfem_stokes_vector_download": (C.c_int, [_vp, C.c_int, _vp, _dp]),
    "stfem_stokes_vmult": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "stfem_stokes_mass_vmult": (C.c_int, [_vp, _vp, _vp, _vp]),
    "stfem_stokes_st_vmult": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(_vp),
                                        C.POINTER(_vp), _vp]),
    "stfem_stokes_st_vmult_slice_add": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(_vp),
                                                  _vp, _vp, _vp]),
    "stfem_stokes_vmult_convection": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "stfem_stokes_st_vmult_convection": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(_vp),
                                                   C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "stfem_stokes_st_vmult_slice_add_convection": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.POINTER(_vp),
                                                             _vp, _vp, _vp, _vp]),
    "stfem_stokes_last_hip_error": (C.c_char_p, []),
    "stfem_stokes_last_sweep_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "stfem_stokes_set_weak_boundaries": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double]),
    "stfem_stokes_n_face_points": (C.c_int64, [_vp]),
    "stfem_stokes_face_points": (C.c_int, [_vp, _dp]),
    "stfem_stokes_nitsche_rhs": (C.c_int, [_vp, _dp, _vp, _vp, _vp]),
    "stfem_stokes_set_cip": (C.c_int, [_vp, C.c_double, C.c_int]),
    "stfem_stokes_cip_add": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, _vp]),
    "stfem_stokes_set_cip_neighbours": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "stfem_stokes_cip_ghost_size": (C.c_int64, [_vp]),
    "stfem_stokes_cip_ghost_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "stfem_stokes_cip_ghost_destroy": (None, [_vp, _vp]),
    "stfem_stokes_cip_pack": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "stfem_stokes_cip_add_slab": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "stfem_stokes_cip_bind_ghosts": (C.c_int, [_vp, _vp, _vp, _vp]),
    "stfem_stokes_pressure_ctx": (C.c_int, [_vp, C.POINTER(_vp)]),
    "stfem_stokes_pressure_mean_vectors": (C.c_int, [_vp, _dp, _dp, _dp]),
    "stfem_stokes_pressure_quadrature_points": (C.c_int, [_vp, C.c_int, _dp]),
    "stfem_stokes_pressure_difference": (C.c_int, [_vp, C.c_int, _vp, _dp, _dp, _vp]),
    "stfem_stokes_divergence": (C.c_int, [_vp, _vp, _vp, _dp, _vp]),
    "stfem_stokes_drag_lift_n_items": (C.c_int64, [_vp, C.c_int]),
    "stfem_stokes_drag_lift": (C.c_int, [_vp, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp), _vp, _dp, _vp]),
    "stfem_stokes_dgp_prolongate": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "stfem_stokes_dgp_restrict": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "stfem_stokes_vanka_create": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int32), _dp, _dp, C.POINTER(_vp)]),
    "stfem_stokes_vanka_create_linearised": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int32), _dp, _dp, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    "stfem_stokes_vanka_create_linearised_partitioned": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_int32), _dp, _dp, C.c_int, C.POINTER(_vp),
                                                         C.c_double, C.c_int, C.c_int, C.POINTER(_vp)]),
    "stfem_stokes_vanka_create_linearised_cip": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int32), _dp, _dp, C.c_int, C.POINTER(_vp), C.c_double,
                                                 C.POINTER(_vp)]),
    "stfem_stokes_vanka_update": (C.c_int, [_vp, C.POINTER(_vp)]),
    "stfem_stokes_vanka_destroy": (None, [_vp]),
    "stfem_stokes_vanka_n_classes": (C.c_int, [_vp]),
    "stfem_stokes_vanka_setup_batches": (C.c_int, [_vp]),
    "stfem_stokes_vanka_vmult": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "stfem_stokes_vanka_step": (C.c_int, [_vp, C.POINTER(_vp), C.c_double, C.c_int, C.POINTER(_vp), _vp]),
    "stfem_stokes_vanka_last_error": (C.c_char_p, []),
    "stfem_strerror": (C.c_char_p, [C.c_int]),
    "stfem_last_error": (C.c_char_p, []),
    "stfem_last_hip_error": (C.c_char_p, []),
    "stfem_last_kernel_name": (C.c_char_p, [_vp]),
    "stfem_last_sweep_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "stfem_last_tile_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

# every symbol the companion header include/stfem_stokes_space.h declares (tests/test_stokes_space_header_cpu.py)
SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_space.h")
SPACE_SIGNATURES = {
    "stfem_stokes_create_space": (C.c_int, [C.POINTER(_MeshDesc), C.POINTER(_StokesSpaceDesc), C.POINTER(_vp)]),
    "stfem_stokes_last_cell_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

# every symbol the companion header include/stfem_stokes_vanka_space.h declares (tests/test_stokes_vanka_space_header_cpu.py)
VANKA_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_vanka_space.h")
VANKA_SPACE_SIGNATURES = {
    "stfem_stokes_vanka_create_space": (C.c_int, [_vp, C.POINTER(_StokesVankaSpaceDesc), C.POINTER(_vp)]),
}

# every symbol the companion header include/stfem_stokes_convection_space.h declares (tests/test_stokes_convection_space_header_cpu.py)
CONVECTION_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_convection_space.h")
CONVECTION_SPACE_SIGNATURES = {
    "stfem_stokes_vmult_convection_space": SIGNATURES["stfem_stokes_vmult_convection"],
    "stfem_stokes_st_vmult_convection_space": SIGNATURES["stfem_stokes_st_vmult_convection"],
    "stfem_stokes_st_vmult_slice_add_convection_space": SIGNATURES["stfem_stokes_st_vmult_slice_add_convection"],
    "stfem_stokes_last_convection_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

# every symbol the companion header include/stfem_stokes_vanka_linearised_space.h declares
# (tests/test_stokes_vanka_linearised_space_header_cpu.py)
VANKA_LINEARISED_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_vanka_linearised_space.h")
VANKA_LINEARISED_SPACE_SIGNATURES = {
    "stfem_stokes_vanka_create_linearised_space": (C.c_int, [_vp, C.POINTER(_StokesVankaLinearisedSpaceDesc), C.POINTER(_vp)]),
}

# every symbol the companion header include/stfem_stokes_pressure_space.h declares (tests/test_stokes_pressure_space_header_cpu.py)
PRESSURE_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_pressure_space.h")
PRESSURE_SPACE_SIGNATURES = {
    "stfem_stokes_get_space": (C.c_int, [_vp, C.POINTER(_StokesSpaceDesc)]),
    "stfem_stokes_pressure_ctx_space": SIGNATURES["stfem_stokes_pressure_ctx"],
    "stfem_stokes_pressure_mean_vectors_space": SIGNATURES["stfem_stokes_pressure_mean_vectors"],
    "stfem_stokes_pressure_quadrature_points_space": SIGNATURES["stfem_stokes_pressure_quadrature_points"],
    "stfem_stokes_pressure_difference_space": SIGNATURES["stfem_stokes_pressure_difference"],
    "stfem_stokes_dgp_prolongate_space": SIGNATURES["stfem_stokes_dgp_prolongate"],
    "stfem_stokes_dgp_restrict_space": SIGNATURES["stfem_stokes_dgp_restrict"],
    "stfem_stokes_divergence_space": SIGNATURES["stfem_stokes_divergence"],
    "stfem_stokes_last_divergence_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

# every symbol the companion header include/stfem_stokes_boundary_space.h declares (tests/test_stokes_boundary_space_header_cpu.py)
BOUNDARY_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_boundary_space.h")
BOUNDARY_SPACE_SIGNATURES = {
    "stfem_stokes_set_weak_boundaries_space": SIGNATURES["stfem_stokes_set_weak_boundaries"],
    "stfem_stokes_n_face_points_space": SIGNATURES["stfem_stokes_n_face_points"],
    "stfem_stokes_face_points_space": SIGNATURES["stfem_stokes_face_points"],
    "stfem_stokes_nitsche_rhs_space": SIGNATURES["stfem_stokes_nitsche_rhs"],
    "stfem_stokes_last_face_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

# every symbol the companion header include/stfem_stokes_cip_space.h declares (tests/test_stokes_cip_space_header_cpu.py)
CIP_SPACE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "stfem_stokes_cip_space.h")
CIP_SPACE_SIGNATURES = {
    "stfem_stokes_set_cip_space": SIGNATURES["stfem_stokes_set_cip"],
    "stfem_stokes_cip_add_space": SIGNATURES["stfem_stokes_cip_add"],
    "stfem_stokes_last_cip_plan": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}


def lib():
    """Loads the HIP library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C dealii-stfem_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(os.environ.get("STFEM_LIB", LIB_PATH))  # STFEM_LIB: experiment builds only
        for name, (res, args) in (list(SIGNATURES.items()) + list(SPACE_SIGNATURES.items()) + list(VANKA_SPACE_SIGNATURES.items()) +
                                  list(CONVECTION_SPACE_SIGNATURES.items()) + list(VANKA_LINEARISED_SPACE_SIGNATURES.items()) +
                                  list(PRESSURE_SPACE_SIGNATURES.items()) + list(BOUNDARY_SPACE_SIGNATURES.items()) +
                                  list(CIP_SPACE_SIGNATURES.items())):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(_dp)


def _check(status, what):
    if status != 0:
        raise StfemError(status, what)


# --------------------------------------------------------------------------- host helpers


def _time_transfer(fn, *args):
    dims = (C.c_int32 * 2)()
    _check(fn(*args, None, dims), fn.__name__)
    out = np.zeros((dims[0], dims[1]))
    _check(fn(*args, _p(out), dims), fn.__name__)
    return out


def get_time_prolongation_matrix(ttype, r, n_timesteps_at_once=2):
    """fe_time.h:805-849"""
    return _time_transfer(lib().stfem_time_prolongation_matrix, ttype, r, n_timesteps_at_once)


def get_time_restriction_matrix(ttype, r, n_timesteps_at_once=2):
    """fe_time.h:851-898"""
    return _time_transfer(lib().stfem_time_restriction_matrix, ttype, r, n_timesteps_at_once)


def get_time_projection_matrix(ttype, r_src, r_dst, n_timesteps_at_once=1):
    """fe_time.h:749-803"""
    return _time_transfer(lib().stfem_time_projection_matrix, ttype, r_src, r_dst, n_timesteps_at_once)


def get_time_evaluation_matrix(ttype, r, samples_per_interval):
    """fe_time.h:308-326 for the basis of get_time_basis(ttype, r): [samples_per_interval, r + 1], the temporal basis at
    s / (samples_per_interval - 1).  For cG the first column belongs to the step's initial value."""
    return _time_transfer(lib().stfem_time_evaluation_matrix, ttype, r, samples_per_interval)


def get_fe_time_weights(ttype, r, time_step_size=1.0, n_timesteps_at_once=1):
    """fe_time.h:351-409 -> (Alpha, Beta, Gamma, Zeta)."""
    nb = (r if ttype == CGP else r + 1) * n_timesteps_at_once
    A = np.zeros((nb, nb)); B = np.zeros((nb, nb)); G = np.zeros((nb, 1)); Z = np.zeros((nb, 1))
    rc = lib().stfem_fe_time_weights(ttype, r, time_step_size, n_timesteps_at_once,
                                     _p(A), _p(B), _p(G), _p(Z))
    if rc != nb:
        raise StfemError(rc, "stfem_fe_time_weights")
    return A, B, G, Z


def get_fe_time_weights_wave(ttype, r, time_step_size=1.0, n_timesteps_at_once=1):
    """fe_time.h:157-305 -> (Alpha_lhs, Beta_lhs, rhs_uK, rhs_uM, rhs_vM)."""
    nb = (r if ttype == CGP else r + 1) * n_timesteps_at_once
    A = np.zeros((nb, nb)); B = np.zeros((nb, nb))
    v = [np.zeros((nb, 1)) for _ in range(3)]
    rc = lib().stfem_fe_time_weights_wave(ttype, r, time_step_size, n_timesteps_at_once,
                                          _p(A), _p(B), _p(v[0]), _p(v[1]), _p(v[2]))
    if rc != nb:
        raise StfemError(rc, "stfem_fe_time_weights_wave")
    return A, B, v[0], v[1], v[2]


def mesh_vertices(global_ncell, lower=(0, 0, 0), upper=(1, 1, 1), distort=0.0, seed=5489,
                  z_range=None):
    """Structured vertex grid of a z-slab [z0, z1) of cells of the global mesh."""
    gn = (C.c_int32 * 3)(*global_ncell)
    z0, z1 = z_range if z_range else (0, global_ncell[2])
    lo = np.array(lower, dtype=np.float64); up = np.array(upper, dtype=np.float64)
    out = np.zeros(((global_ncell[0] + 1) * (global_ncell[1] + 1) * (z1 - z0 + 1), 3))
    _check(lib().stfem_mesh_vertices(gn, _p(lo), _p(up), distort, seed, z0, z1, _p(out)),
           "stfem_mesh_vertices")
    return out


def coefficient_per_cell(ncell, vertices, c1=1.0, c2=9.0, c3=16.0, distort_coeff=0.0,
                         subdivisions=(1, 1, 1), lower=(0, 0, 0), upper=(1, 1, 1)):
    nc = (C.c_int32 * 3)(*ncell); sub = (C.c_int32 * 3)(*subdivisions)
    lo = np.array(lower, dtype=np.float64); up = np.array(upper, dtype=np.float64)
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    out = np.zeros(int(np.prod(ncell)))
    _check(lib().stfem_coefficient_per_cell(nc, _p(v), c1, c2, c3, distort_coeff, sub, _p(lo),
                                            _p(up), _p(out)), "stfem_coefficient_per_cell")
    return out


# --------------------------------------------------------------------------- device objects


class BlockVector:
    """LinearAlgebra::distributed::BlockVector stand-in: n_blocks device arrays (types.h:19-23)."""

    def __init__(self, ctx, n_blocks=None, device_ptrs=None):
        self.ctx = ctx
        h = _vp()
        if device_ptrs is not None:
            arr = (_vp * len(device_ptrs))(*device_ptrs)
            _check(lib().stfem_vector_wrap(ctx._h, len(device_ptrs), arr, C.byref(h)),
                   "stfem_vector_wrap")
            self.n_blocks = len(device_ptrs)
        else:
            _check(lib().stfem_vector_create(ctx._h, n_blocks, C.byref(h)), "stfem_vector_create")
            self.n_blocks = n_blocks
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.stfem_vector_destroy(self._h)
            self._h = None

    def rebind(self, device_ptrs):
        """Points a view (made with device_ptrs=...) at other device arrays without reallocating."""
        arr = (_vp * len(device_ptrs))(*device_ptrs)
        _check(lib().stfem_vector_rebind(self._h, len(device_ptrs), arr), "stfem_vector_rebind")
        self.n_blocks = len(device_ptrs)
        return self

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        assert host.shape == (self.n_blocks, self.ctx.n_dofs)
        ptrs = (_dp * self.n_blocks)(*[_p(host[b]) for b in range(self.n_blocks)])
        _check(lib().stfem_vector_upload(self._h, ptrs), "stfem_vector_upload")
        return self

    def download(self):
        out = np.zeros((self.n_blocks, self.ctx.n_dofs))
        ptrs = (_dp * self.n_blocks)(*[_p(out[b]) for b in range(self.n_blocks)])
        _check(lib().stfem_vector_download(self._h, ptrs), "stfem_vector_download")
        return out

    def block_ptr(self, b):
        return lib().stfem_vector_block(self._h, b)


class MatrixFreeOperator:
    """Context = MatrixFree + MatrixFreeOperator state of one rank (operators.h:967-1191)."""

    def __init__(self, degree, ncell, vertices=None, lower=(0, 0, 0), upper=(1, 1, 1),
                 dirichlet_mask=63, device=0, mass_matrix_scaling=0.0, laplace_matrix_scaling=0.0,
                 number="double"):
        self.degree = degree
        self.ncell = tuple(int(v) for v in ncell)
        self.mass_matrix_scaling = mass_matrix_scaling
        self.laplace_matrix_scaling = laplace_matrix_scaling
        m = _MeshDesc()
        m.ncell[:] = self.ncell
        self._verts = None
        if vertices is not None:
            self._verts = np.ascontiguousarray(vertices, dtype=np.float64)
            assert self._verts.size == 3 * np.prod([n + 1 for n in self.ncell])
            m.vertices = _p(self._verts)
        m.lower[:] = lower
        m.upper[:] = upper
        m.dirichlet_mask = dirichlet_mask
        m.device = device
        assert number in ("double", "float")  # the operator's Number template argument
        self.number = number
        s = _SpaceDesc(degree, degree + 1, 1, 1 if number == "float" else 0)
        h = _vp()
        _check(lib().stfem_ctx_create(C.byref(m), C.byref(s), C.byref(h)), "stfem_ctx_create")
        self._h = h
        self.n_dofs = lib().stfem_n_dofs(h)
        self.n_cells = lib().stfem_n_cells(h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.stfem_ctx_destroy(self._h)
            self._h = None

    def m(self):
        return self.n_dofs

    @property
    def is_cartesian(self):
        return bool(lib().stfem_is_cartesian(self._h))

    def evaluate_coefficient(self, values, which=1):
        """operators.h:1060-1087.  values: None | (n_cells,) | (n_cells, nq^3)."""
        if values is None:
            _check(lib().stfem_set_coefficient(self._h, which, 0, None), "stfem_set_coefficient")
            return
        v = np.ascontiguousarray(values, dtype=np.float64)
        layout = 1 if v.size == self.n_cells else 2
        assert v.size in (self.n_cells, self.n_cells * (self.degree + 1) ** 3)
        _check(lib().stfem_set_coefficient(self._h, which, layout, _p(v)), "stfem_set_coefficient")

    def initialize_dof_vector(self, n_blocks=1):
        return BlockVector(self, n_blocks)

    def vmult(self, dst, src, stream=None):
        _check(lib().stfem_space_vmult(self._h, self.mass_matrix_scaling,
                                       self.laplace_matrix_scaling, dst._h, src._h, stream),
               "stfem_space_vmult")

    def compute_diagonal(self, mass=None, laplace=None, stream=None):
        d = BlockVector(self, 1)
        _check(lib().stfem_diagonal(self._h,
                                    self.mass_matrix_scaling if mass is None else mass,
                                    self.laplace_matrix_scaling if laplace is None else laplace,
                                    d._h, stream), "stfem_diagonal")
        return d

    def get_matrix_diagonal(self, stream=None):
        """operators.h:1035-1039"""
        return self.compute_diagonal(stream=stream)

    def get_matrix_diagonal_inverse(self, stream=None):
        """operators.h:1041-1045, 1106-1109: 1/d where |d| > sqrt(eps), 1 elsewhere."""
        d = BlockVector(self, 1)
        _check(lib().stfem_diagonal_inverse(self._h, self.mass_matrix_scaling, self.laplace_matrix_scaling,
                                            d._h, stream), "stfem_diagonal_inverse")
        return d

    @property
    def last_kernel_name(self):
        return lib().stfem_last_kernel_name(self._h).decode()

    @property
    def last_sweep_plan(self):
        """(tiles, workgroups launched) of the last pencil-sweep launch; (0, 0) after another kernel variant"""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_last_sweep_plan(self._h, out), "stfem_last_sweep_plan")
        return tuple(out)

    @property
    def last_tile_plan(self):
        """(x-tiles, y-tiles, z-chunks, cell layers of the longest chunk) of the last tile-sweep launch; zeros after another
        kernel variant"""
        out = (C.c_int32 * 4)()
        _check(lib().stfem_last_tile_plan(self._h, out), "stfem_last_tile_plan")
        return tuple(out)


class PreconditionVanka:
    """stmg.h:619-907: cell-patch additive-Schwarz smoother of Alpha (x) K + Beta (x) M on one context."""

    def __init__(self, ctx, Alpha, Beta, neighbour_mask=0, extended=None):
        """neighbour_mask: faces (bits as dirichlet_mask) behind which another rank holds the next cells; extended: on general
        meshes the context of the slab plus one ghost cell layer per such face (stfem_vanka_create_partitioned_general)"""
        self.ctx = ctx
        A = np.ascontiguousarray(Alpha, dtype=np.float64)
        B = np.ascontiguousarray(Beta, dtype=np.float64)
        assert A.shape == B.shape and A.shape[0] == A.shape[1]
        h = _vp()
        if extended is not None:
            _check(lib().stfem_vanka_create_partitioned_general(ctx._h, extended._h, A.shape[0], _p(A), _p(B), neighbour_mask, C.byref(h)),
                   "stfem_vanka_create_partitioned_general")
        else:
            _check(lib().stfem_vanka_create_partitioned(ctx._h, A.shape[0], _p(A), _p(B), neighbour_mask, C.byref(h)),
                   "stfem_vanka_create")
        self._h, self.n_blocks = h, A.shape[0]

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.stfem_vanka_destroy(self._h)
            self._h = None

    @property
    def n_classes(self):
        return lib().stfem_vanka_n_classes(self._h)

    @property
    def plan(self):
        """(row tiles per workgroup, parts per cell block)"""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_vanka_plan(self._h, out), "stfem_vanka_plan")
        return tuple(out)

    @property
    def setup_batches(self):
        """batches of cell layers the device set-up of the per-cell blocks took (0: class blocks, host set-up)"""
        return lib().stfem_vanka_setup_batches(self._h)

    def vmult(self, dst, src, stream=None):
        _check(lib().stfem_vanka_vmult(self._h, dst._h, src._h, stream), "stfem_vanka_vmult")

    smooth = vmult  # stmg.h:881-885

    def step(self, dst, omega, accumulate, src, stream=None):
        """dst = (dst if accumulate else 0) + omega * vmult(src): the relaxation step around the smoother (stmg.h:1199-1238)"""
        _check(lib().stfem_vanka_step(self._h, dst._h, omega, int(bool(accumulate)), src._h, stream), "stfem_vanka_step")


class SystemMatrix:
    """operators.h:517-663: A = Alpha (x) K + Beta (x) M on one context."""

    def __init__(self, ctx, Alpha, Beta):
        self.ctx = ctx
        self.Alpha = np.ascontiguousarray(Alpha, dtype=np.float64)
        self.Beta = np.ascontiguousarray(Beta, dtype=np.float64)
        assert self.Alpha.shape == self.Beta.shape and self.Alpha.ndim == 2

    def m(self):
        return self.Alpha.shape[0] * self.ctx.n_dofs

    def initialize_dof_vector(self):
        return BlockVector(self.ctx, self.Alpha.shape[0])

    def _apply(self, dst, src, transpose, add, stream):
        nr, nc = self.Alpha.shape
        _check(lib().stfem_st_vmult(self.ctx._h, nr, nc, _p(self.Alpha), _p(self.Beta),
                                    int(transpose), int(add), dst._h, src._h, stream),
               "stfem_st_vmult")

    def vmult(self, dst, src, stream=None):
        self._apply(dst, src, False, False, stream)

    def Tvmult(self, dst, src, stream=None):
        self._apply(dst, src, True, False, stream)

    def vmult_slice(self, dst, src, stream=None):
        assert self.Alpha.shape[1] == 1
        self._apply(dst, src, False, False, stream)

    def vmult_slice_add(self, dst, src, stream=None):
        assert self.Alpha.shape[1] == 1
        self._apply(dst, src, False, True, stream)

    def _diagonal(self, inverse, stream):
        n = self.Alpha.shape[0]
        assert self.Alpha.shape == (n, n)
        d = BlockVector(self.ctx, n)
        _check(lib().stfem_st_diagonal(self.ctx._h, n, _p(self.Alpha), _p(self.Beta), int(inverse), d._h, stream),
               "stfem_st_diagonal")
        return d

    def get_matrix_diagonal(self, stream=None):
        """operators.h:613-623: block i = Alpha(i,i) diag K + Beta(i,i) diag M."""
        return self._diagonal(False, stream)

    def get_matrix_diagonal_inverse(self, stream=None):
        """operators.h:625-637, as the reference combines it: 1/Alpha(i,i) (diag K)^-1 + 1/Beta(i,i) (diag M)^-1."""
        return self._diagonal(True, stream)


def tensorproduct_add(ctx, c, A, b, stream=None):
    """operators.h:238-250: c_i += A(i,j) b_j, skipping exact zeros."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    _check(lib().stfem_tensorproduct_add(ctx._h, A.shape[0], A.shape[1], _p(A), c._h, b._h,
                                         stream), "stfem_tensorproduct_add")


def dot(ctx, a, b, n_own=0, stream=None):
    out = C.c_double(0.0)
    _check(lib().stfem_dot(ctx._h, a._h, b._h, n_own, C.byref(out), stream), "stfem_dot")
    return out.value


def multi_dot(ctx, vs, w, n_own=0, stream=None):
    """[<v_i, w>]: the inner products of a Gram-Schmidt step in one pass over w per eight vectors (deterministic reductions)"""
    k = len(vs)
    out = np.zeros(k)
    arr = (_vp * k)(*[v._h for v in vs])
    _check(lib().stfem_multi_dot(ctx._h, k, arr, w._h, n_own, _p(out), stream), "stfem_multi_dot")
    return out


def multi_axpy(ctx, coef, xs, y, stream=None):
    """y += sum_i coef_i x_i"""
    k = len(xs)
    c = np.ascontiguousarray(coef, dtype=np.float64)
    assert c.size == k
    arr = (_vp * k)(*[v._h for v in xs])
    _check(lib().stfem_multi_axpy(ctx._h, k, _p(c), arr, y._h, stream), "stfem_multi_axpy")


def orthogonalize(ctx, vs, w, n_own=0, stream=None):
    """one classical Gram-Schmidt pass on the device: returns (h = V^T w, <w, w> after w -= V h, <w, w> before)"""
    k = len(vs)
    h = np.zeros(k)
    n2, b2 = C.c_double(0.0), C.c_double(0.0)
    arr = (_vp * k)(*[v._h for v in vs])
    _check(lib().stfem_orthogonalize(ctx._h, k, arr, w._h, n_own, _p(h), C.byref(b2), C.byref(n2), stream), "stfem_orthogonalize")
    return h, n2.value, b2.value


# ------------------------------------------------------------------ space-time multigrid (8 f-2)

def get_poly_mg_sequence(k_max, k_min, sequence_type="decrease_by_one"):
    """fe_time.cc:40-56; coarsest degree first"""
    kind = {"bisect": 0, "decrease_by_one": 1, "go_to_one": 2}[sequence_type]
    n = C.c_int32(0)
    _check(lib().stfem_poly_mg_sequence(k_max, k_min, kind, None, C.byref(n)), "stfem_poly_mg_sequence")
    out = (C.c_int32 * n.value)()
    _check(lib().stfem_poly_mg_sequence(k_max, k_min, kind, out, C.byref(n)), "stfem_poly_mg_sequence")
    return list(out)


def get_mg_sequence(n_sp_lvl, k_seq, p_seq=(), n_timesteps_at_once=1, n_timesteps_at_once_min=1, lower_lvl="k",
                    coarsening_type="space_and_time", time_before_space=False, use_p_multigrid_space=False,
                    zip_from_back=True):
    """fe_time.cc:58-124 -> string over 't' (tau), 'k', 'h', 'p' (MGType), coarsest transfer first"""
    ct = {"space_or_time": 0, "space_and_time": 1}[coarsening_type]
    args = (n_sp_lvl, len(k_seq), len(p_seq), n_timesteps_at_once, n_timesteps_at_once_min, lower_lvl.encode(), ct,
            int(time_before_space), int(use_p_multigrid_space), int(zip_from_back))
    n = C.c_int32(0)
    _check(lib().stfem_mg_sequence(*args, None, C.byref(n)), "stfem_mg_sequence")
    buf = C.create_string_buffer(n.value + 1)
    _check(lib().stfem_mg_sequence(*args, buf, C.byref(n)), "stfem_mg_sequence")
    return buf.raw[:n.value].decode()


def get_precondition_stmg_types(mg_type_level, coarsening_type="space_and_time", time_before_space=False, smoother=1):
    """fe_time.cc:126-150: smoother id per level (0 = identity, 1 = relaxation, 2 = Chebyshev)"""
    ct = {"space_or_time": 0, "space_and_time": 1}[coarsening_type]
    out = (C.c_int32 * (len(mg_type_level) + 1))()
    _check(lib().stfem_precondition_stmg_types(mg_type_level.encode(), len(mg_type_level), ct, int(time_before_space),
                                               smoother, out), "stfem_precondition_stmg_types")
    return list(out)


class MGTwoLevelTransfer:
    """deal.II MGTwoLevelTransfer between two contexts as MGTwoLevelBlockTransfer uses it (stmg.h:38-110)."""

    def __init__(self, fine, coarse, neighbour_mask=0):
        """neighbour_mask: 16 = a slab below, 32 = a slab above (z-slab partition)"""
        self.fine, self.coarse = fine, coarse
        h = _vp()
        _check(lib().stfem_transfer_create_partitioned(fine._h, coarse._h, neighbour_mask, C.byref(h)), "stfem_transfer_create")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.stfem_transfer_destroy(self._h)
            self._h = None

    def prolongate_and_add(self, dst, src, stream=None):
        _check(lib().stfem_transfer_prolongate(self._h, dst._h, src._h, 1, stream), "stfem_transfer_prolongate")

    def prolongate(self, dst, src, stream=None):
        _check(lib().stfem_transfer_prolongate(self._h, dst._h, src._h, 0, stream), "stfem_transfer_prolongate")

    def restrict_and_add(self, dst, src, stream=None):
        _check(lib().stfem_transfer_restrict(self._h, dst._h, src._h, 1, stream), "stfem_transfer_restrict")

    def restrict(self, dst, src, stream=None):
        _check(lib().stfem_transfer_restrict(self._h, dst._h, src._h, 0, stream), "stfem_transfer_restrict")

    def interpolate(self, dst, src, stream=None):
        _check(lib().stfem_transfer_interpolate(self._h, dst._h, src._h, stream), "stfem_transfer_interpolate")

    @property
    def last_path(self):
        """(fused y-z kernel in the last prolongation, coarse cells one thread marched through in the last restriction along y, along z)"""
        out = (C.c_int32 * 3)()
        _check(lib().stfem_transfer_last_path(self._h, out), "stfem_transfer_last_path")
        return tuple(out)


def transfer_line_matrices(ncell_fine, degree_fine, ncell_coarse, degree_coarse):
    """(P [n_f x n_c], I [n_c x n_f]): the 1D factors of a space transfer, without constraints"""
    n_f, n_c = degree_fine * ncell_fine + 1, degree_coarse * ncell_coarse + 1
    P, I = np.zeros((n_f, n_c)), np.zeros((n_c, n_f))
    _check(lib().stfem_transfer_line_matrices(ncell_fine, degree_fine, ncell_coarse, degree_coarse, _p(P), _p(I)),
           "stfem_transfer_line_matrices")
    return P, I


def vector_convert(dst, src, stream=None):
    """dst = src across contexts of different precision (stmg.h:1330-1343)"""
    _check(lib().stfem_vector_convert(dst._h, src._h, stream), "stfem_vector_convert")


# ------------------------------------------------------- around the operator: load vectors, error norms (8 f-3)

def support_points(ctx):
    """[n_dofs, 3]: the nodes in the order of the vectors (VectorTools::interpolate = evaluate + upload)"""
    out = np.zeros((ctx.n_dofs, 3))
    _check(lib().stfem_support_points(ctx._h, _p(out)), "stfem_support_points")
    return out


def quadrature_points(ctx, nq):
    """[n_cells, nq^3, 3]: the points of QGauss(nq)^3, q = qx + nq (qy + nq qz)"""
    out = np.zeros((ctx.n_cells, max(int(nq), 0) ** 3, 3))
    _check(lib().stfem_quadrature_points(ctx._h, nq, _p(out) if out.size else None), "stfem_quadrature_points")
    return out


def _points_array(ctx, nq, values, per_point, what):
    if values is None:
        return None, None
    a = np.ascontiguousarray(values, dtype=np.float64)
    if 1 <= nq <= 8:  # other nq: the library reports the error
        assert a.size == ctx.n_cells * nq ** 3 * per_point, what
    return a, _p(a)


def integrate_rhs(ctx, nq, f, dst, block=0, stream=None):
    """block `block` of dst = (f, phi_i) with QGauss(nq), f [n_cells, nq^3] at quadrature_points; constrained rows 0"""
    a, ptr = _points_array(ctx, nq, f, 1, "f")
    _check(lib().stfem_integrate_rhs(ctx._h, nq, ptr, dst._h, block, stream), "stfem_integrate_rhs")


def integrate_rhs_product(ctx, nq, amplitude, frequency, dst, block=0, stream=None):
    """the same with f(x) = amplitude * prod_d sin(2 pi frequency x_d) evaluated on the device"""
    _check(lib().stfem_integrate_rhs_product(ctx._h, nq, amplitude, frequency, dst._h, block, stream), "stfem_integrate_rhs_product")


def integrate_difference(ctx, nq, u, block, exact, exact_grad=None, stream=None):
    """(sum JxW (u_h - u)^2, max |u_h - u|, sum JxW |grad u_h - grad u|^2) of block `block` of u; exact [n_cells, nq^3],
    exact_grad [n_cells, nq^3, 3] or None (third entry 0)"""
    e, pe = _points_array(ctx, nq, exact, 1, "exact")
    g, pg = _points_array(ctx, nq, exact_grad, 3, "exact_grad")
    out = np.zeros(3)
    _check(lib().stfem_integrate_difference(ctx._h, nq, u._h, block, pe, pg, _p(out), stream), "stfem_integrate_difference")
    return out


def integrate_difference_product(ctx, nq, u, block, amplitude, frequency, stream=None):
    """the same against amplitude * prod_d sin(2 pi frequency x_d) and its gradient, evaluated on the device"""
    out = np.zeros(3)
    _check(lib().stfem_integrate_difference_product(ctx._h, nq, u._h, block, amplitude, frequency, _p(out), stream), "stfem_integrate_difference_product")
    return out


def vector_axpby(ctx, a, x, b, y, stream=None):
    """y = a x + b y on every block; a zero factor means "not read"; x and y may be the same vector"""
    _check(lib().stfem_vector_axpby(ctx._h, a, x._h, b, y._h, stream), "stfem_vector_axpby")


def vector_set_zero(ctx, y, stream=None):
    _check(lib().stfem_vector_set_zero(ctx._h, y._h, stream), "stfem_vector_set_zero")


def gauss_rule(n):
    """QGauss(n) on [0, 1] -> (points, weights)"""
    x, w = np.zeros(max(int(n), 1)), np.zeros(max(int(n), 1))
    _check(lib().stfem_gauss_rule(n, _p(x), _p(w)), "stfem_gauss_rule")
    return x, w


def fe_time_points(ttype, r):
    """support points of the temporal basis (fe_time.cc:152-161): Gauss-Lobatto for cG(r), right Gauss-Radau for dG(r)"""
    x = np.zeros(max(int(r), 0) + 1)
    _check(lib().stfem_fe_time_points(ttype, r, _p(x)), "stfem_fe_time_points")
    return x


# ------------------------------------------------------------------------------- Stokes (8a-14)

def stokes_block_index(n_timedofs, timestep, variable, timedof, variable_major=True):
    """BlockSlice::index (reference include/fe_time.h:956-967), two variables."""
    if variable_major:
        return timestep * (2 * n_timedofs) + variable * n_timedofs + timedof
    return timestep * (2 * n_timedofs) + timedof * 2 + variable


def get_fe_time_weights_stokes(type_, r, time_step_size, n_timesteps_at_once=1):
    """Alpha, Beta, Gamma, Zeta of get_fe_time_weights_stokes (fe_time.h:1242-1285): the scalar matrices
    of get_fe_time_weights scattered into the (variable, time dof) block structure.  The
    pressure-pressure block of Alpha stays empty, Beta only couples velocity with velocity; the
    right-hand-side matrices Gamma, Zeta act on the velocity rows, and for cG Gamma on the pressure
    rows as well (fe_time.h:1275-1282)."""
    A, B, G, Z = get_fe_time_weights(type_, r, time_step_size, n_timesteps_at_once)
    n = A.shape[0]
    nt = n // n_timesteps_at_once
    Alpha = np.zeros((2 * n, 2 * n)); Beta = np.zeros((2 * n, 2 * n))
    Gamma = np.zeros((2 * n, G.shape[1])); Zeta = np.zeros((2 * n, Z.shape[1]))
    idx = lambda v, k: stokes_block_index(nt, k // nt, v, k % nt)  # noqa: E731
    for a in range(n):
        for b in range(n):
            for iv in range(2):
                for jv in range(2):
                    if not (iv == 1 and jv == 1):
                        Alpha[idx(iv, a), idx(jv, b)] = A[a, b]
            Beta[idx(0, a), idx(0, b)] = B[a, b]
        Gamma[idx(0, a), :] = G[a, :]
        Zeta[idx(0, a), :] = Z[a, :]
        if type_ == CGP:
            Gamma[idx(1, a), :] = G[a, :]
    return Alpha, Beta, Gamma, Zeta


def _face_mask(faces):
    """bit mask of a set of boundary ids 0..5 (face 2 d + s); an int is taken as the mask itself"""
    if isinstance(faces, (int, np.integer)):
        return int(faces)
    return sum(1 << int(f) for f in set(faces))


# The Navier-Stokes modes of StokesMatrixFreeOperator (OperatorMode::form / jacobian, operators.h:1288-1297): the `mode` of vmult,
# st_vmult and st_vmult_slice_add; 0 is the linear operator
CONVECTION_NONE, CONVECTION_FORM, CONVECTION_JACOBIAN = 0, 1, 2
# Whose velocity weighs the CIP interior-face term (StokesMatrixFreeOperator.set_cip): the source of the vmult (the reference's
# behaviour: cubic in the source), or - with a convection mode - the linearisation velocity (linear in the source)
CIP_WEIGHT_SOURCE, CIP_WEIGHT_LINEARISATION = 0, 1


class StokesMatrixFreeOperator:
    """StokesMatrixFreeOperator + SystemMatrixStokes of the reference (include/operators.h:1193-1575,
    666-868) for the cell loop, FE_Q(2)^3 x FE_Q(1).  Vectors are device pointers (e.g.
    torch.Tensor.data_ptr()): velocity 3 * n_velocity doubles (component-major), pressure n_pressure.
    vmult / st_vmult / st_vmult_slice_add take the convection mode (CONVECTION_FORM / CONVECTION_JACOBIAN) and the linearisation
    velocity `lin` that the reference's set_data hands in; with the defaults they are the linear operator.  delta0 != 0 adds the
    CIP interior-face stabilisation (operators.h:1605-1633) to all of them, see set_cip.  with_degree(3, ...): FE_Q(3)^3 x FE_Q(2) /
    FE_DGP(2), the linear cell operator with the convection modes (cell term), weak (Nitsche) faces of the linear operator through
    set_weak_boundaries_space (no mode then), the CIP term through set_cip_space / cip_add_space, StokesPreconditionVanka.for_space
    over it, the pressure space helpers and divergence_space."""

    def __init__(self, ncell, vertices=None, lower=(0, 0, 0), upper=(1, 1, 1), dirichlet_mask=63,
                 viscosity=1.0, velocity_degree=2, device=0, weak_boundary_ids=(), outflow_boundary_ids=(),
                 penalty1=20.0, penalty2=10.0, dg_pressure=False, delta0=0.0, cip_weight=CIP_WEIGHT_SOURCE, _space=None):
        """weak_boundary_ids / outflow_boundary_ids: boundary ids 0..5 (face 2 d + s) as in the reference's constructor
        (operators.h:1206-1211); penalty1 / penalty2: its Nitsche penalties (gamma1 = viscosity penalty1, gamma2 = penalty2)."""
        m = _MeshDesc()
        self.ncell = tuple(int(v) for v in ncell)
        m.ncell[:] = self.ncell
        self._verts = None
        if vertices is not None:
            self._verts = np.ascontiguousarray(vertices, dtype=np.float64)
            m.vertices = _p(self._verts)
        m.lower[:] = lower
        m.upper[:] = upper
        m.dirichlet_mask = dirichlet_mask
        m.device = device
        h = _vp()
        # dg_pressure: FE_DGP(degree - 1) instead of FE_Q(degree - 1) (the reference's dGPressure, tests/tp_03stokes.cc:83-86)
        if _space is None:  # the keyword velocity_degree: stfem_stokes_create_ex, which builds degree 2 alone
            _check(lib().stfem_stokes_create_ex(C.byref(m), velocity_degree, 1 if dg_pressure else 0, viscosity, C.byref(h)),
                   "stfem_stokes_create")
        else:               # with_degree: the constructor by descriptor
            sd = _StokesSpaceDesc()
            sd.velocity_degree, sd.pressure_space, sd.viscosity = int(_space[0]), 1 if dg_pressure else 0, float(viscosity)
            sd.reserved[:] = _space[1]
            _check(lib().stfem_stokes_create_space(C.byref(m), C.byref(sd), C.byref(h)), "stfem_stokes_create_space")
            velocity_degree = int(_space[0])
        self.velocity_degree = velocity_degree
        # with_degree: vmult / st_vmult / st_vmult_slice_add with lin= / mode= go through the _space entries (stfem_stokes_convection_space.h)
        self._space_entries = _space is not None
        self._h = h
        self.n_velocity = lib().stfem_stokes_n_velocity_dofs(h)
        self.n_pressure = lib().stfem_stokes_n_pressure_dofs(h)
        self.weak_mask = sum(1 << int(f) for f in set(weak_boundary_ids))
        self.outflow_mask = sum(1 << int(f) for f in set(outflow_boundary_ids))
        if self.weak_mask or self.outflow_mask:
            _check(lib().stfem_stokes_set_weak_boundaries(h, self.weak_mask, self.outflow_mask, penalty1, penalty2),
                   "stfem_stokes_set_weak_boundaries")
        self.delta0, self.cip_weight = 0.0, CIP_WEIGHT_SOURCE
        if delta0 != 0.0 or cip_weight != CIP_WEIGHT_SOURCE:
            self.set_cip(delta0, cip_weight)

    @classmethod
    def with_degree(cls, velocity_degree, ncell, reserved=(0, 0, 0, 0), **keywords):
        """The operator through stfem_stokes_create_space; the keywords of the constructor except velocity_degree.  Degree 2: the
        operator of the constructor, bit for bit.  Degree 3: FE_Q(3)^3 x FE_Q(2), or FE_DGP(2) with dg_pressure (ten DoFs per cell),
        QGauss(4) - the pair of the reference's time degree 2 - with the cell operator alone: vmult, mass_vmult, st_vmult, st_Tvmult,
        st_vmult_slice_add, with the convection modes (lin=, mode=: the cell term); its smoother is StokesPreconditionVanka.for_space,
        over the linear operator.  Weak / outflow ids as keywords, delta0 != 0 and everything else raise StfemError with status -2 and the
        reason; the weak faces of a degree-3 operator are set with set_weak_boundaries_space afterwards, its CIP term with set_cip_space.
        An operator made here sends lin= / mode= through the _space entries of include/stfem_stokes_convection_space.h, and
        pressure_mean_vectors, pressure_quadrature_points, pressure_difference, pressure_ctx and (between two such operators)
        stokes_dgp_prolongate / stokes_dgp_restrict through those of include/stfem_stokes_pressure_space.h (at degree 2 the entries of
        the constructor's operator, bit for bit).  divergence_space is the divergence at either degree; divergence stays the entry of
        stfem.h, which refuses degree 3.  On z-slabs (each slab an operator of its own, its interface faces 4 / 5 left out of the
        strong mask, the weak set and the outflow set; the interface planes hold partial sums) a degree-3 operator is held against
        the whole mesh for vmult, the modes without weak faces, st_vmult, st_vmult_slice_add, st_Tvmult, mass_vmult, nitsche_rhs_space,
        divergence_space and the CIP term without the interface faces (tests/test_gpu_stokes_q3_slabs.py); set_cip_neighbours, the
        partitioned Vanka blocks, StokesSpaces::set_partition of the C++ mirror and GMGStokes are still missing there."""
        assert "velocity_degree" not in keywords and "_space" not in keywords
        return cls(ncell, _space=(velocity_degree, tuple(int(v) for v in reserved)), **keywords)

    def last_cell_plan(self):
        """(workgroups, longest run of cells per wave - per half-wave at degree 2) of the last colour launch of the cell kernel, at
        either degree; the environment variable STFEM_STOKES_Q3_WORKGROUPS, read at every launch, caps the workgroups of the colour
        launches of the cell kernel at either degree.  A context that has not launched the cell kernel raises status -2."""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_stokes_last_cell_plan(self._h, out), "stfem_stokes_last_cell_plan")
        return tuple(out)

    def last_convection_plan(self):
        """(workgroups, longest run of cells per wave - per half-wave at degree 2) of the last convection colour launch;
        STFEM_STOKES_Q3_WORKGROUPS caps the workgroups of those launches too, at either degree.  A context that has launched no convection kernel
        raises status -2."""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_stokes_last_convection_plan(self._h, out), "stfem_stokes_last_convection_plan")
        return tuple(out)

    def set_cip(self, delta0, weight=CIP_WEIGHT_SOURCE):
        """The CIP gradient-jump term sum_F int_F delta0 h_F^2 / 2^3.5 (w.n)^2 [d_n u].[d_n v] on the interior faces in every later
        vmult / st_vmult / st_vmult_slice_add (not mass_vmult; the Vanka blocks take a delta0 of their own, StokesPreconditionVanka).  weight: CIP_WEIGHT_SOURCE (w = the source, as
        the reference has it) or CIP_WEIGHT_LINEARISATION (w = `lin` where a convection mode is given).  delta0 = 0: no launch."""
        _check(lib().stfem_stokes_set_cip(self._h, float(delta0), int(weight)), "stfem_stokes_set_cip")
        self.delta0, self.cip_weight = float(delta0), int(weight)

    def cip_add(self, dst_u, src_u, weight_u, delta0, stream=None):
        """dst_u += C(weight_u; src_u): the CIP term by itself with the given delta0, independent of set_cip"""
        dst_u, src_u, weight_u = (getattr(v, "ptr", v) for v in (dst_u, src_u, weight_u))
        _check(lib().stfem_stokes_cip_add(self._h, dst_u, src_u, weight_u, float(delta0), stream), "stfem_stokes_cip_add")

    def set_cip_space(self, delta0, weight=CIP_WEIGHT_SOURCE):
        """set_cip through stfem_stokes_set_cip_space (include/stfem_stokes_cip_space.h): either velocity degree; at degree 2 the setter
        behind set_cip, bit for bit.  At degree 3 the term is sum_F int_F delta0 h_F^2 / 3^3.5 (w.n)^2 [d_n u].[d_n v] at the 4 x 4 Gauss
        points of the interior faces, added last by every later vmult / st_vmult / st_vmult_slice_add, with or without a convection mode
        (not by mass_vmult; the Vanka blocks of a degree-3 operator do not take the term)."""
        _check(lib().stfem_stokes_set_cip_space(self._h, float(delta0), int(weight)), "stfem_stokes_set_cip_space")
        self.delta0, self.cip_weight = float(delta0), int(weight)

    def cip_add_space(self, dst_u, src_u, weight_u, delta0, stream=None):
        """cip_add through stfem_stokes_cip_add_space: dst_u += C(weight_u; src_u) at either velocity degree, independent of set_cip_space"""
        dst_u, src_u, weight_u = (getattr(v, "ptr", v) for v in (dst_u, src_u, weight_u))
        _check(lib().stfem_stokes_cip_add_space(self._h, dst_u, src_u, weight_u, float(delta0), stream), "stfem_stokes_cip_add_space")

    def last_cip_plan(self):
        """(workgroups, passes of the grid-stride loop: the longest run of cells per wave - per half-wave at degree 2) of the last CIP
        colour launch; the environment variable STFEM_STOKES_CIP_WORKGROUPS, read at every launch, caps the workgroups of those
        launches.  A context that has not launched the CIP kernel raises status -2."""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_stokes_last_cip_plan(self._h, out), "stfem_stokes_last_cip_plan")
        return tuple(out)

    def set_cip_neighbours(self, neighbour_mask, lower_vertices=None, upper_vertices=None):
        """This operator is a z-slab with a slab below (bit 4) and / or above (bit 5): the CIP term treats the interface faces as
        interior.  lower / upper_vertices: [(ncx + 1)(ncy + 1)][3], the vertex plane one cell layer beyond the interface (general
        meshes; None on a box).  Mask 0: the state of an operator that never had neighbours."""
        lo, up = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (lower_vertices, upper_vertices))
        plane = (self.ncell[0] + 1) * (self.ncell[1] + 1) * 3
        assert all(v is None or v.size == plane for v in (lo, up))
        _check(lib().stfem_stokes_set_cip_neighbours(self._h, int(neighbour_mask), None if lo is None else _p(lo),
                                                     None if up is None else _p(up)), "stfem_stokes_set_cip_neighbours")
        self.cip_neighbours = int(neighbour_mask)

    @property
    def cip_ghost_size(self):
        """doubles of one side's ghost planes: 3 components, 2 planes"""
        return int(lib().stfem_stokes_cip_ghost_size(self._h))

    def cip_ghost_vector(self):
        """a zeroed device array of cip_ghost_size doubles (object with .ptr, .size, free()); freeing it drops its bindings"""
        return StokesCipGhost(self)

    def cip_pack(self, src_u, side, out, stream=None):
        """out <- what the neighbour on `side` (0 lower, 1 upper) needs of src_u: this slab's two DoF planes next to that interface
        plane, 0 on the DoFs this operator constrains strongly; out: cip_ghost_size doubles on the device"""
        _check(lib().stfem_stokes_cip_pack(self._h, getattr(src_u, "ptr", src_u), int(side), getattr(out, "ptr", out), stream),
               "stfem_stokes_cip_pack")

    def cip_add_slab(self, dst_u, src_u, weight_u, delta0, lower_ghost=None, upper_ghost=None, stream=None):
        """cip_add with the interface faces of set_cip_neighbours: lower / upper_ghost are the neighbours' cip_pack results (None for
        a side without neighbour); the interface planes of dst_u receive partial sums"""
        dst_u, src_u, weight_u, lower_ghost, upper_ghost = (getattr(v, "ptr", v) for v in (dst_u, src_u, weight_u, lower_ghost, upper_ghost))
        _check(lib().stfem_stokes_cip_add_slab(self._h, dst_u, src_u, weight_u, float(delta0), lower_ghost, upper_ghost, stream),
               "stfem_stokes_cip_add_slab")

    def cip_bind_ghosts(self, src_u, lower_ghost=None, upper_ghost=None):
        """The ghost planes that vmult / st_vmult / st_vmult_slice_add read for the velocity source src_u (looked up by its pointer)
        once set_cip and set_cip_neighbours are in force; None, None unbinds"""
        src_u, lower_ghost, upper_ghost = (getattr(v, "ptr", v) for v in (src_u, lower_ghost, upper_ghost))
        _check(lib().stfem_stokes_cip_bind_ghosts(self._h, src_u, lower_ghost, upper_ghost), "stfem_stokes_cip_bind_ghosts")

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.stfem_stokes_destroy(self._h)
            self._h = None

    def face_points(self):
        """quadrature points of the weak faces [point][3], where the Dirichlet function is evaluated (operators.h:1911-1914)"""
        n = lib().stfem_stokes_n_face_points(self._h)
        if n < 0:
            raise StfemError(int(n), "stfem_stokes_n_face_points")
        out = np.zeros((n, 3))
        _check(lib().stfem_stokes_face_points(self._h, _p(out)), "stfem_stokes_face_points")
        return out

    def set_weak_boundaries_space(self, weak_boundary_ids, outflow_boundary_ids=(), penalty1=20.0, penalty2=10.0):
        """The weak (Nitsche) / outflow faces through stfem_stokes_set_weak_boundaries_space (include/stfem_stokes_boundary_space.h):
        either velocity degree; at degree 2 the setter behind the constructor's keywords, bit for bit.  Every later vmult / st_vmult /
        st_Tvmult / st_vmult_slice_add of the linear operator includes the face launches, and StokesPreconditionVanka.for_space over
        this operator builds blocks with the Nitsche terms.  At degree 3 with weak faces a convection mode (lin= / mode=) and the
        linearised blocks raise status -2: the inflow term of the faces is not built there."""
        weak = sum(1 << int(f) for f in set(weak_boundary_ids))
        outflow = sum(1 << int(f) for f in set(outflow_boundary_ids))
        _check(lib().stfem_stokes_set_weak_boundaries_space(self._h, weak, outflow, float(penalty1), float(penalty2)),
               "stfem_stokes_set_weak_boundaries_space")
        self.weak_mask, self.outflow_mask = weak, outflow

    def n_face_points_space(self):
        """number of face quadrature points of the weak faces, (degree + 1)^2 per face cell (stfem_stokes_n_face_points_space)"""
        n = lib().stfem_stokes_n_face_points_space(self._h)
        if n < 0:
            raise StfemError(int(n), "stfem_stokes_n_face_points_space")
        return int(n)

    def face_points_space(self):
        """face_points through stfem_stokes_face_points_space: either velocity degree, QGauss(degree + 1) on the faces"""
        out = np.zeros((self.n_face_points_space(), 3))
        _check(lib().stfem_stokes_face_points_space(self._h, _p(out)), "stfem_stokes_face_points_space")
        return out

    def nitsche_rhs_space(self, g, dst_u, dst_p, stream=None):
        """nitsche_rhs through stfem_stokes_nitsche_rhs_space: either velocity degree; g at face_points_space(), in its order"""
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert g.shape == (self.n_face_points_space(), 3)
        _check(lib().stfem_stokes_nitsche_rhs_space(self._h, _p(g), getattr(dst_u, "ptr", dst_u), getattr(dst_p, "ptr", dst_p), stream),
               "stfem_stokes_nitsche_rhs_space")

    def last_face_plan(self):
        """(workgroups, longest run of boundary cells per wave - per half-wave at degree 2) of the last boundary colour launch; the
        environment variable STFEM_STOKES_FACE_WORKGROUPS, read at every launch, caps the workgroups of those launches.  A context that
        has not launched the boundary kernel raises status -2."""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_stokes_last_face_plan(self._h, out), "stfem_stokes_last_face_plan")
        return tuple(out)

    def nitsche_rhs(self, g_at_face_points, dst_u, dst_p, stream=None):
        """StokesNitscheMatrixFreeOperator::vmult(dst) (operators.h:1833-1849): dst += boundary functional of the Dirichlet data"""
        g = np.ascontiguousarray(g_at_face_points, dtype=np.float64)
        assert g.shape == (lib().stfem_stokes_n_face_points(self._h), 3)
        _check(lib().stfem_stokes_nitsche_rhs(self._h, _p(g), getattr(dst_u, "ptr", dst_u), getattr(dst_p, "ptr", dst_p), stream),
               "stfem_stokes_nitsche_rhs")

    def initialize_dof_vector(self, variable, host=None):
        """Device vector of `variable` (0 velocity, 1 pressure) as a StokesVector; optionally filled."""
        return StokesVector(self, variable, host)

    def vmult(self, dst_u, dst_p, src_u, src_p, stream=None, lin=None, mode=0):
        dst_u, dst_p, src_u, src_p = (getattr(v, "ptr", v) for v in (dst_u, dst_p, src_u, src_p))
        if mode == 0 and lin is None:
            _check(lib().stfem_stokes_vmult(self._h, dst_u, dst_p, src_u, src_p, stream), "stfem_stokes_vmult")
            return
        args = (self._h, int(mode), dst_u, dst_p, src_u, src_p, getattr(lin, "ptr", lin), stream)
        if self._space_entries:
            _check(lib().stfem_stokes_vmult_convection_space(*args), "stfem_stokes_vmult_convection_space")
        else:
            _check(lib().stfem_stokes_vmult_convection(*args), "stfem_stokes_vmult_convection")

    @property
    def last_sweep_plan(self):
        """(tiles, workgroups launched, gradient added by the sweep itself) of the last vmult's velocity sweep (tiles and workgroups as
        MatrixFreeOperator.last_sweep_plan of the scalar FE_Q(2) context)"""
        out = (C.c_int32 * 3)()
        _check(lib().stfem_stokes_last_sweep_plan(self._h, out), "stfem_stokes_last_sweep_plan")
        return tuple(out)

    def mass_vmult(self, dst_u, src_u, stream=None):
        dst_u, src_u = getattr(dst_u, "ptr", dst_u), getattr(src_u, "ptr", src_u)
        _check(lib().stfem_stokes_mass_vmult(self._h, dst_u, src_u, stream), "stfem_stokes_mass_vmult")

    def st_vmult(self, Alpha, Beta, n_timesteps_at_once, n_timedofs, dst_blocks, src_blocks,
                 variable_major=True, stream=None, lin=None, mode=0):
        """SystemMatrixStokes::vmult; dst_blocks / src_blocks: device pointers in BlockSlice order.  lin: the linearisation vector in
        the same order (only its velocity entries are read; pressure entries may be None)."""
        nb = 2 * n_timesteps_at_once * n_timedofs
        A = np.ascontiguousarray(Alpha, dtype=np.float64); B = np.ascontiguousarray(Beta, dtype=np.float64)
        assert A.shape == (nb, nb) and B.shape == (nb, nb) and len(dst_blocks) == nb and len(src_blocks) == nb
        d = (_vp * nb)(*[getattr(v, "ptr", v) for v in dst_blocks])
        s_ = (_vp * nb)(*[getattr(v, "ptr", v) for v in src_blocks])
        if mode == 0 and lin is None:
            _check(lib().stfem_stokes_st_vmult(self._h, n_timesteps_at_once, n_timedofs, int(variable_major),
                                               _p(A), _p(B), d, s_, stream), "stfem_stokes_st_vmult")
            return
        assert lin is None or len(lin) == nb
        l_ = None if lin is None else (_vp * nb)(*[getattr(v, "ptr", v) for v in lin])
        args = (self._h, int(mode), n_timesteps_at_once, n_timedofs, int(variable_major), _p(A), _p(B), d, s_, l_, stream)
        if self._space_entries:
            _check(lib().stfem_stokes_st_vmult_convection_space(*args), "stfem_stokes_st_vmult_convection_space")
        else:
            _check(lib().stfem_stokes_st_vmult_convection(*args), "stfem_stokes_st_vmult_convection")

    def st_Tvmult(self, Alpha, Beta, n_timesteps_at_once, n_timedofs, dst_blocks, src_blocks, variable_major=True, stream=None):
        """SystemMatrixStokes::Tvmult AS THE REFERENCE HAS IT (operators.h:708-745): its scatter overload (operators.h:111-123)
        takes j = index(it, v, id), i = index(jt, v, jd), so the result of source time dof (it, id) only goes to the destination
        blocks of the same time dof, weighted with the entries of row j summed over the time dofs - not a transpose.  Expressed
        with the effective matrices of that rule and run as one st_vmult."""
        nt, ns = n_timedofs, n_timesteps_at_once
        nb = 2 * nt * ns
        A = np.asarray(Alpha, dtype=np.float64); B = np.asarray(Beta, dtype=np.float64)
        eps10 = 10 * np.finfo(np.float64).eps
        Ae, Be = np.zeros((nb, nb)), np.zeros((nb, nb))
        idx = lambda it, v, d: stokes_block_index(nt, it, v, d, variable_major)  # noqa: E731
        for it in range(ns):
            for d in range(nt):
                col = idx(it, 0, d)  # the velocity column drives the scatters of st_vmult
                for v in range(2):
                    j = idx(it, v, d)
                    Ae[j, col] = sum(A[j, idx(jt, v, jd)] for jt in range(ns) for jd in range(nt) if abs(A[j, idx(jt, v, jd)]) > eps10)
                j = idx(it, 0, d)
                Be[j, col] = sum(B[j, idx(jt, 0, jd)] for jt in range(ns) for jd in range(nt) if abs(B[j, idx(jt, 0, jd)]) > eps10)
        self.st_vmult(Ae, Be, ns, nt, dst_blocks, src_blocks, variable_major, stream)

    def st_vmult_slice_add(self, Gamma, Zeta, n_timesteps_at_once, n_timedofs, dst_blocks, src_u, src_p,
                           variable_major=True, stream=None, lin=None, mode=0):
        """SystemMatrixStokes::vmult_slice_add (n x 1 right-hand-side case); dst is accumulated into."""
        nb = 2 * n_timesteps_at_once * n_timedofs
        g = np.ascontiguousarray(Gamma, dtype=np.float64).reshape(-1)
        z = np.ascontiguousarray(Zeta, dtype=np.float64).reshape(-1)
        assert g.size == nb and z.size == nb and len(dst_blocks) == nb
        d = (_vp * nb)(*[getattr(v, "ptr", v) for v in dst_blocks])
        if mode == 0 and lin is None:
            _check(lib().stfem_stokes_st_vmult_slice_add(self._h, n_timesteps_at_once, n_timedofs, int(variable_major),
                                                         _p(g), _p(z), d, getattr(src_u, "ptr", src_u),
                                                         getattr(src_p, "ptr", src_p), stream),
                   "stfem_stokes_st_vmult_slice_add")
            return
        args = (self._h, int(mode), n_timesteps_at_once, n_timedofs, int(variable_major), _p(g), _p(z), d, getattr(src_u, "ptr", src_u),
                getattr(src_p, "ptr", src_p), getattr(lin, "ptr", lin), stream)
        if self._space_entries:
            _check(lib().stfem_stokes_st_vmult_slice_add_convection_space(*args), "stfem_stokes_st_vmult_slice_add_convection_space")
        else:
            _check(lib().stfem_stokes_st_vmult_slice_add_convection(*args), "stfem_stokes_st_vmult_slice_add_convection")

    @property
    def n_cells(self):
        return int(np.prod(self.ncell))

    def pressure_quadrature_points(self, nq):
        """[n_cells, nq^3, 3]: QGauss(nq)^3 on the cells (axis-aligned uniform meshes)"""
        out = np.zeros((self.n_cells, max(int(nq), 1) ** 3, 3))
        if self._space_entries:
            _check(lib().stfem_stokes_pressure_quadrature_points_space(self._h, nq, _p(out)), "stfem_stokes_pressure_quadrature_points_space")
        else:
            _check(lib().stfem_stokes_pressure_quadrature_points(self._h, nq, _p(out)), "stfem_stokes_pressure_quadrature_points")
        return out

    def pressure_difference(self, nq, p, exact, stream=None):
        """(sum JxW (p_h - p)^2, max |p_h - p|) of the device pressure vector p against exact [n_cells, nq^3] at those points"""
        e = np.ascontiguousarray(exact, dtype=np.float64)
        if 1 <= nq <= 8:
            assert e.size == self.n_cells * nq ** 3
        out = np.zeros(2)
        args = (self._h, nq, getattr(p, "ptr", p), _p(e), _p(out), stream)
        if self._space_entries:
            _check(lib().stfem_stokes_pressure_difference_space(*args), "stfem_stokes_pressure_difference_space")
        else:
            _check(lib().stfem_stokes_pressure_difference(*args), "stfem_stokes_pressure_difference")
        return out

    def divergence(self, u, cells=False, stream=None):
        """StokesMatrixFreeOperator::compute_divergence (operators.h:1391-1439): sqrt(sum_cells int (div u_h)^2) of the device
        velocity vector u at the operator's Gauss points, the values read plain (constrained entries count as stored).
        cells=True: (total, [n_cells] cell values, cells lexicographic); cells=<device pointer>: the cell values are written there.
        stfem_stokes_divergence: velocity degree 2 only, on every operator (a degree-3 operator is refused; divergence_space runs)."""
        return self._divergence(lambda *args: lib().stfem_stokes_divergence(*args), "stfem_stokes_divergence", u, cells, stream)

    def divergence_space(self, u, cells=False, stream=None):
        """divergence through stfem_stokes_divergence_space (include/stfem_stokes_pressure_space.h): either velocity degree; at degree 2
        the bits of divergence"""
        return self._divergence(lambda *args: lib().stfem_stokes_divergence_space(*args), "stfem_stokes_divergence_space", u, cells, stream)

    def _divergence(self, entry, name, u, cells, stream):
        total = C.c_double(0.0)
        scratch = None
        if cells is True:  # (a pressure vector holds the cell values: either pressure space has at least one DoF per cell)
            scratch = StokesVector(self, 1)
            dptr = scratch.ptr
        else:
            dptr = None if cells is False or cells is None else getattr(cells, "ptr", cells)
        _check(entry(self._h, getattr(u, "ptr", u), dptr, C.byref(total), stream), name)
        return (total.value, scratch.download()[:self.n_cells].copy()) if scratch is not None else total.value

    def drag_lift_n_items(self, faces):
        """work items of drag_lift: the pairs (face of `faces`, boundary cell of that face)"""
        n = lib().stfem_stokes_drag_lift_n_items(self._h, _face_mask(faces))
        if n < 0:
            raise StfemError(int(n), "stfem_stokes_drag_lift_n_items")
        return int(n)

    def drag_lift(self, u, p, faces, scale=1.0, plain=False, items=False, stream=None):
        """StokesMatrixFreeOperator::compute_drag_lift (operators.h:1344-1389): scale * sum over the boundary faces `faces` (ids
        0..5, face 2 d + s: the reference's obstacle_id; or the bit mask) of int (p n - nu (grad u + grad u^T) n) dA at the 3 x 3 face
        Gauss points -> [3].  u, p: one device velocity and pressure vector, or two lists of the same length -> [n, 3] from one call.
        plain=False reads velocity entries on strongly constrained DoFs as 0 (the reference), plain=True as stored.
        items=True: (force, item values [n_items, 3] or [n, n_items, 3]): the unscaled force of every (face, boundary cell) pair,
        faces ascending, the cells of a face with the lower tangential axis fastest."""
        single = not isinstance(u, (list, tuple))
        if isinstance(p, (list, tuple)) == single or (not single and len(u) != len(p)):
            raise ValueError("drag_lift: u and p are one pair or two lists of the same length")
        us, ps = ([u], [p]) if single else (list(u), list(p))
        n, mask = len(us), _face_mask(faces)
        U = [getattr(v, "ptr", v) for v in us]
        P = [getattr(v, "ptr", v) for v in ps]
        out = np.zeros((max(n, 1), 3))

        def call(first, count, d_items):
            o = np.zeros((max(count, 1), 3))
            _check(lib().stfem_stokes_drag_lift(self._h, mask, float(scale), int(bool(plain)), count, (_vp * max(count, 1))(*U[first:first + count]),
                                                (_vp * max(count, 1))(*P[first:first + count]), d_items, _p(o), stream), "stfem_stokes_drag_lift")
            out[first:first + max(count, 1)] = o

        if not items:
            call(0, n, None)
            return out[0] if single else out
        # a velocity vector holds the item values (n_items < n_velocity on every mesh): as many pairs per call as fit into it;
        # how the pairs are grouped changes no bit of a result
        nitems = self.drag_lift_n_items(mask)
        scratch = StokesVector(self, 0)
        per_call = max(self.n_velocity // nitems, 1)
        it = np.zeros((max(n, 1), nitems, 3))
        for first in range(0, max(n, 1), per_call):
            count = min(per_call, n - first)
            call(first, count, scratch.ptr)
            it[first:first + count] = scratch.download()[:count * nitems * 3].reshape(count, nitems, 3)
        return (out[0], it[0]) if single else (out, it)

    def pressure_mean_vectors(self):
        """(ones, weights, volume): coefficients of p = 1, (1, psi_j), and the volume: mean(p) = weights . p / volume"""
        ones, weights, volume = np.zeros(self.n_pressure), np.zeros(self.n_pressure), C.c_double(0.0)
        args = (self._h, _p(ones), _p(weights), C.byref(volume))
        if self._space_entries:
            _check(lib().stfem_stokes_pressure_mean_vectors_space(*args), "stfem_stokes_pressure_mean_vectors_space")
        else:
            _check(lib().stfem_stokes_pressure_mean_vectors(*args), "stfem_stokes_pressure_mean_vectors")
        return ones, weights, volume.value

    def space(self):
        """(velocity degree, pressure space 0 = FE_Q / 1 = FE_DGP, viscosity) the context was made with (stfem_stokes_get_space)"""
        sd = _StokesSpaceDesc()
        _check(lib().stfem_stokes_get_space(self._h, C.byref(sd)), "stfem_stokes_get_space")
        return int(sd.velocity_degree), int(sd.pressure_space), float(sd.viscosity)

    def pressure_ctx(self):
        """The handle of the scalar context behind the pressure vectors (owned by the operator): for FE_Q the pressure space on the
        mesh, for FE_DGP a carrier for the vector arithmetic alone.  For stfem_vector_wrap, stfem_dot, stfem_vector_axpby ..."""
        h = _vp()
        if self._space_entries:
            _check(lib().stfem_stokes_pressure_ctx_space(self._h, C.byref(h)), "stfem_stokes_pressure_ctx_space")
        else:
            _check(lib().stfem_stokes_pressure_ctx(self._h, C.byref(h)), "stfem_stokes_pressure_ctx")
        return h

    def last_divergence_plan(self):
        """(workgroups, longest run of cells per wave or half-wave) of the last divergence launch"""
        out = (C.c_int32 * 2)()
        _check(lib().stfem_stokes_last_divergence_plan(self._h, out), "stfem_stokes_last_divergence_plan")
        return int(out[0]), int(out[1])


def stokes_dgp_prolongate(fine, coarse, dst, src, add=False, stream=None):
    """FE_DGP(1) pressure (FE_DGP(2) between two operators of velocity degree 3 made by with_degree): dst_fine (+)= embedding of
    src_coarse; `fine` has twice the cells of `coarse` per direction"""
    args = (fine._h, coarse._h, getattr(dst, "ptr", dst), getattr(src, "ptr", src), int(bool(add)), stream)
    if fine._space_entries and coarse._space_entries:
        _check(lib().stfem_stokes_dgp_prolongate_space(*args), "stfem_stokes_dgp_prolongate_space")
    else:
        _check(lib().stfem_stokes_dgp_prolongate(*args), "stfem_stokes_dgp_prolongate")


def stokes_dgp_restrict(fine, coarse, dst, src, add=False, stream=None):
    """dst_coarse (+)= the transpose of the embedding applied to src_fine"""
    args = (fine._h, coarse._h, getattr(dst, "ptr", dst), getattr(src, "ptr", src), int(bool(add)), stream)
    if fine._space_entries and coarse._space_entries:
        _check(lib().stfem_stokes_dgp_restrict_space(*args), "stfem_stokes_dgp_restrict_space")
    else:
        _check(lib().stfem_stokes_dgp_restrict(*args), "stfem_stokes_dgp_restrict")


class StokesPreconditionVanka:
    """PreconditionVanka over a two-variable BlockSlice (stmg.h:626-738, 832-872, as tests/tp_03stokes.cc:714-726 creates it).
    block_variable[i] = 0 (velocity) / 1 (pressure) for the blocks in BlockSlice order; Alpha, Beta: the matrices of
    get_fe_time_weights_stokes.  per_cell=True or a convection mode builds one block per cell from the operator linearised about
    `lin` (reinit_asm, stmg.h:929-965): device vectors in BlockSlice order like those of st_vmult, only the velocity entries are read
    (pressure entries may be None); update(lin) rebuilds the blocks for new states.  delta0 != 0 (implies one block per cell): the
    blocks hold the CIP term C(lin_j; .) too, weighted by the linearisation state of the column block in every mode
    (stfem_stokes_vanka_create_linearised_cip); update keeps that delta0.  The defaults are the class blocks of a box (one block per
    cell on a general mesh).  for_space(...): the constructor by descriptor, which also serves an operator of velocity degree 3."""

    def __init__(self, op, block_variable, Alpha, Beta, lin=None, mode=0, per_cell=False, delta0=0.0, partition=None):
        """partition=(extended_op, neighbour_mask, beyond_mask): `op` is a z-slab; the per-cell blocks are set up on extended_op (the
        slab plus one ghost cell layer per z neighbour of neighbour_mask, bit 4 below / 5 above; `lin`, also of update, lives there),
        built for the slab's own cells and applied on `op`, partial sums in the interface planes.  beyond_mask: cells beyond a ghost
        layer (read with delta0 != 0).  stfem_stokes_vanka_create_linearised_partitioned."""
        bv, A, B = self._blocks(op, block_variable, Alpha, Beta, partition)
        h = _vp()
        if partition is not None:
            ext, nmask, bmask = partition
            rc = lib().stfem_stokes_vanka_create_linearised_partitioned(getattr(op, "_h", None), getattr(ext, "_h", None), self.nb, bv, _p(A),
                                                                        _p(B), int(mode), self._lin(lin), float(delta0), int(nmask),
                                                                        int(bmask), C.byref(h))
            what = "stfem_stokes_vanka_create_linearised_partitioned"
        elif delta0 != 0.0:
            rc = lib().stfem_stokes_vanka_create_linearised_cip(op._h, self.nb, bv, _p(A), _p(B), int(mode), self._lin(lin), float(delta0),
                                                                C.byref(h))
            what = "stfem_stokes_vanka_create_linearised_cip"
        elif per_cell or mode != 0:
            rc = lib().stfem_stokes_vanka_create_linearised(op._h, self.nb, bv, _p(A), _p(B), int(mode), self._lin(lin), C.byref(h))
            what = "stfem_stokes_vanka_create_linearised"
        else:
            rc = lib().stfem_stokes_vanka_create(op._h, self.nb, bv, _p(A), _p(B), C.byref(h))
            what = "stfem_stokes_vanka_create"
        assert rc == 0 or not h.value
        _check(rc, what)
        self._h = h

    @classmethod
    def for_space(cls, op, block_variable, Alpha, Beta, reserved=(0, 0, 0, 0), lin=None, mode=0):
        """The smoother through stfem_stokes_vanka_create_space: one block per cell of the linear operator `op`, whatever its
        velocity degree.  Degree 2: the blocks of per_cell=True with mode 0, bit for bit.  Degree 3 (StokesMatrixFreeOperator.
        with_degree(3, ...)): 192 velocity and 27 / 10 pressure rows per time dof, at most 512 rows (two time dofs); this is the
        constructor that serves it - the plain one raises StfemError with status -2.  vmult / step / update(None) as usual.
        With `lin` or a convection mode: through stfem_stokes_vanka_create_linearised_space, the blocks of the operator linearised
        about `lin` (device vectors in BlockSlice order, pressure entries may be None) at either degree; update(lin) rebuilds them."""
        self = cls.__new__(cls)
        bv, A, B = self._blocks(op, block_variable, Alpha, Beta, None)
        if lin is not None or mode != 0:
            d = _StokesVankaLinearisedSpaceDesc()
            d.n_blocks, d.block_variable, d.Alpha, d.Beta, d.mode = self.nb, bv, _p(A), _p(B), int(mode)
            d.lin_blocks = self._lin(lin)
            d.reserved[:] = [int(v) for v in reserved]
            h = _vp()
            rc = lib().stfem_stokes_vanka_create_linearised_space(op._h, C.byref(d), C.byref(h))
            assert rc == 0 or not h.value
            _check(rc, "stfem_stokes_vanka_create_linearised_space")
            self._h = h
            return self
        d = _StokesVankaSpaceDesc()
        d.n_blocks, d.block_variable, d.Alpha, d.Beta = self.nb, bv, _p(A), _p(B)
        d.reserved[:] = [int(v) for v in reserved]
        h = _vp()
        rc = lib().stfem_stokes_vanka_create_space(op._h, C.byref(d), C.byref(h))
        assert rc == 0 or not h.value
        _check(rc, "stfem_stokes_vanka_create_space")
        self._h = h
        return self

    def _blocks(self, op, block_variable, Alpha, Beta, partition):
        """what every constructor starts with: the operator, the block count, and the block layout and weights as the C ABI takes them"""
        self.op, self.partition = op, partition
        self.nb = len(block_variable)
        bv = (C.c_int32 * self.nb)(*[int(v) for v in block_variable])
        A = np.ascontiguousarray(Alpha, dtype=np.float64); B = np.ascontiguousarray(Beta, dtype=np.float64)
        assert A.shape == (self.nb, self.nb) and B.shape == (self.nb, self.nb)
        return bv, A, B

    def _lin(self, lin):
        if lin is None:
            return None
        assert len(lin) == self.nb
        return (_vp * self.nb)(*[getattr(v, "ptr", v) for v in lin])

    def update(self, lin):
        """the blocks again, linearised about `lin` (same mode, same storage)"""
        _check(lib().stfem_stokes_vanka_update(self._h, self._lin(lin)), "stfem_stokes_vanka_update")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().stfem_stokes_vanka_destroy(self._h)
            self._h = None

    @property
    def n_classes(self):
        return lib().stfem_stokes_vanka_n_classes(self._h)

    @property
    def setup_batches(self):
        """batches of cell layers the last create / update of the per-cell blocks took (0: class blocks)"""
        return lib().stfem_stokes_vanka_setup_batches(self._h)

    def step(self, dst_blocks, omega, accumulate, src_blocks, stream=None):
        d = (_vp * self.nb)(*[getattr(v, "ptr", v) for v in dst_blocks])
        s_ = (_vp * self.nb)(*[getattr(v, "ptr", v) for v in src_blocks])
        _check(lib().stfem_stokes_vanka_step(self._h, d, omega, int(bool(accumulate)), s_, stream), "stfem_stokes_vanka_step")

    def vmult(self, dst_blocks, src_blocks, stream=None):
        self.step(dst_blocks, 1.0, False, src_blocks, stream)

    smooth = vmult


class StokesVector:
    """One device vector of a StokesMatrixFreeOperator (velocity: 3 * n_velocity, pressure: n_pressure)."""

    def __init__(self, op, variable, host=None):
        self.op, self.variable = op, variable
        self.size = 3 * op.n_velocity if variable == 0 else op.n_pressure
        h = _vp()
        _check(lib().stfem_stokes_vector_create(op._h, variable, C.byref(h)), "stfem_stokes_vector_create")
        self.ptr = h.value
        if host is not None:
            self.upload(host)

    def upload(self, host):
        a = np.ascontiguousarray(host, dtype=np.float64).reshape(-1)
        assert a.size == self.size
        _check(lib().stfem_stokes_vector_upload(self.op._h, self.variable, self.ptr, _p(a)), "stfem_stokes_vector_upload")
        return self

    def download(self):
        out = np.zeros(self.size)
        _check(lib().stfem_stokes_vector_download(self.op._h, self.variable, self.ptr, _p(out)),
               "stfem_stokes_vector_download")
        return out

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None and getattr(self.op, "_h", None):
            _lib.stfem_stokes_vector_destroy(self.op._h, self.ptr)
            self.ptr = None


class StokesCipGhost:
    """The two velocity DoF planes beyond one interface of a slab, all three components (StokesMatrixFreeOperator.cip_pack fills one,
    cip_add_slab / cip_bind_ghosts read one)."""

    def __init__(self, op):
        self.op, self.size = op, op.cip_ghost_size
        h = _vp()
        _check(lib().stfem_stokes_cip_ghost_create(op._h, C.byref(h)), "stfem_stokes_cip_ghost_create")
        self.ptr = h.value

    def free(self):
        """frees the array now; the operator forgets every binding that names it"""
        self.__del__()

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None and getattr(self.op, "_h", None):
            _lib.stfem_stokes_cip_ghost_destroy(self.op._h, self.ptr)
            self.ptr = None


def axpby_many(ctx, a, xs, b, ys, stream=None):
    """y_i = a x_i + b y_i on device arrays of different lengths in one launch (stfem_axpby_many); xs / ys: objects with .ptr and
    .size (StokesVector) or (pointer, length) pairs"""
    def pl(v):
        return (v.ptr, v.size) if hasattr(v, "ptr") else (int(v[0]), int(v[1]))
    n = len(ys)
    py = [pl(v) for v in ys]
    px = [pl(v) for v in xs] if xs is not None else [(None, ln) for _, ln in py]
    assert len(px) == n and all(a_[1] == b_[1] for a_, b_ in zip(px, py))
    lens = (C.c_int64 * n)(*[ln for _, ln in py])
    X = (_vp * n)(*[p for p, _ in px])
    Y = (_vp * n)(*[p for p, _ in py])
    _check(lib().stfem_axpby_many(ctx._h, n, lens, float(a), X, float(b), Y, stream), "stfem_axpby_many")
