"""ctypes binding of the C ABI in include/polydeal_hip.h (libpolydeal_hip.so, built in-tree).

There is no CPU fallback: if the shared library is missing or no HIP device is present every compute
entry point raises.  Nothing here imports ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDH_LIB: another build of the library (the diagnostic builds of tools/README.md, another commit's build for an A/B)
LIB_PATH = os.environ.get("PDH_LIB") or os.path.join(_HERE, "lib", "libpolydeal_hip.so")

PDH_BASIS_DGQ = 0
PDH_BASIS_AGGLODGP = 1
PDH_OK = 0
PDH_EINVAL, PDH_EUNSUPPORTED, PDH_EDEVICE, PDH_ESTATE, PDH_ENOCONV = -1, -2, -3, -4, -5
PDH_PREC_NONE, PDH_PREC_JACOBI, PDH_PREC_BLOCK_JACOBI, PDH_PREC_CHEBYSHEV, PDH_PREC_DIRECT, PDH_PREC_MULTIGRID = 0, 1, 2, 3, 4, 5
_PREC = {"none": PDH_PREC_NONE, "jacobi": PDH_PREC_JACOBI, "block_jacobi": PDH_PREC_BLOCK_JACOBI}
PDH_SMOOTHER_F64, PDH_SMOOTHER_F32 = 0, 1
_SMOOTHER = {"f64": PDH_SMOOTHER_F64, "f32": PDH_SMOOTHER_F32}
PDH_SMOOTHER_OP_STORED, PDH_SMOOTHER_OP_MATRIX_FREE = 0, 1
_SMOOTHER_OP = {"stored": PDH_SMOOTHER_OP_STORED, "matrix_free": PDH_SMOOTHER_OP_MATRIX_FREE}
PDH_ROWS_ALL, PDH_ROWS_INTERIOR, PDH_ROWS_BOUNDARY = 0, 1, 2
_WHICH = {"all": PDH_ROWS_ALL, "interior": PDH_ROWS_INTERIOR, "boundary": PDH_ROWS_BOUNDARY}
PDH_DCG_DONE, PDH_DCG_HALO_BEGIN, PDH_DCG_HALO_END, PDH_DCG_ALLREDUCE = 0, 1, 2, 3
CG_MAX_ITER = 20000  # solve_cg's default max_iter (the loop bound of examples/host_solver.h)


class PdhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pdh error %d: %s" % (code, msg))
        self.code = code


class pdh_cg_control(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double)]


class pdh_cg_result(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("residual0", C.c_double), ("residual", C.c_double)]


class pdh_halo_info(C.Structure):
    _fields_ = [("n_owned_rows", C.c_int64), ("n_ghost_rows", C.c_int64), ("n_interior", C.c_int32), ("n_boundary", C.c_int32)]


class pdh_dcg_request(C.Structure):
    _fields_ = [("kind", C.c_int32), ("d_send", C.c_void_p), ("d_recv", C.c_void_p), ("d_scalars", C.c_void_p), ("n_scalars", C.c_int32)]


class pdh_chebyshev_control(C.Structure):
    _fields_ = [("inner", C.c_int32), ("degree", C.c_int32), ("smoothing_range", C.c_double), ("eig_cg_n_iterations", C.c_int32),
                ("max_eigenvalue", C.c_double)]


class pdh_chebyshev_info(C.Structure):
    _fields_ = [("estimate", C.c_double), ("lambda_lo", C.c_double), ("lambda_hi", C.c_double), ("cg_iterations", C.c_int32),
                ("degree", C.c_int32), ("inner", C.c_int32)]


class pdh_direct_info(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("pivot_min", C.c_double), ("pivot_max", C.c_double)]


class pdh_matrix_free_info(C.Structure):
    _fields_ = [("table_bytes", C.c_int64), ("doubles_per_polytope", C.c_int32), ("max_cells", C.c_int32), ("max_subfaces", C.c_int32),
                ("max_interior_subfaces", C.c_int32)]


class _Opaque(C.c_void_p):
    """A typed opaque handle: accepts None, an address, or any c_void_p holding one."""

    @classmethod
    def from_param(cls, v):
        return super().from_param(v.value if isinstance(v, C.c_void_p) and not isinstance(v, cls) else v)


class pdh_ctx_p(_Opaque):
    """pdh_ctx * (the entry points of the level transfers and pdh_residual_device)"""


class pdh_transfer_p(_Opaque):
    """pdh_transfer *"""


class pdh_mg_p(_Opaque):
    """pdh_mg *"""


class pdh_transfer_desc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("degree", C.c_int32), ("basis", C.c_int32), ("n_fine", C.c_int32), ("n_coarse", C.c_int32),
                ("n_fine_rows", C.c_int32), ("n_coarse_rows", C.c_int32),
                ("fine_bbox", C.c_void_p), ("coarse_bbox", C.c_void_p), ("fine_dof_offset", C.c_void_p),
                ("coarse_dof_offset", C.c_void_p), ("parent", C.c_void_p)]


class pdh_ptransfer_desc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("fine_degree", C.c_int32), ("coarse_degree", C.c_int32), ("basis", C.c_int32),
                ("n_polytopes", C.c_int32), ("n_fine_rows", C.c_int32), ("n_coarse_rows", C.c_int32),
                ("fine_dof_offset", C.c_void_p), ("coarse_dof_offset", C.c_void_p)]


class pdh_galerkin_level(C.Structure):
    _fields_ = [("n_slots", C.c_int32), ("n_rows_owned", C.c_int32), ("n_rows", C.c_int32), ("exchange_mode", C.c_int32),
                ("device", C.c_int32), ("blk_ptr", C.c_void_p), ("blk_dof", C.c_void_p), ("dof_offset", C.c_void_p)]


class pdh_problem(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("degree", C.c_int32), ("basis", C.c_int32), ("n_agg", C.c_int32),
        ("n_faces", C.c_int32), ("n_rows", C.c_int32), ("diag_first", C.c_int32), ("local", C.c_int32),
        ("reaction_c", C.c_double),
        ("bbox", C.c_void_p), ("dof_offset", C.c_void_p),
        ("vq_ptr", C.c_void_p), ("vq_x", C.c_void_p), ("vq_w", C.c_void_p),
        ("face_in", C.c_void_p), ("face_out", C.c_void_p), ("fq_ptr", C.c_void_p),
        ("fq_x", C.c_void_p), ("fq_n", C.c_void_p), ("fq_w", C.c_void_p), ("fq_w_out", C.c_void_p),
        ("face_sigma", C.c_void_p),
        ("rowptr", C.c_void_p), ("colind", C.c_void_p),
        ("col_offset", C.c_void_p), ("agg_rank", C.c_void_p),
        ("vq_tensor_n", C.c_int32), ("fq_tensor_n", C.c_int32),
    ]


EXPORTS = [
    "pdh_create", "pdh_destroy", "pdh_last_error", "pdh_set_problem", "pdh_set_problem_local",
    "pdh_assemble_device", "pdh_assemble", "pdh_assemble_sip", "pdh_assemble_sip_local",
    "pdh_device_values", "pdh_synchronize", "pdh_stream", "pdh_set_profiling", "pdh_kernel_times_ms",
    "pdh_problem_stats", "pdh_check_problem", "pdh_version", "pdh_assemble_rhs", "pdh_kernel_work", "pdh_evaluate", "pdh_shape_values", "pdh_set_algorithm", "pdh_algorithm_in_use", "pdh_set_overlap",
    "pdh_set_exchange_mode", "pdh_exchange_layout", "pdh_exchange_get_send", "pdh_exchange_apply", "pdh_set_stream",
    "pdh_check_exchange", "pdh_copy_values", "pdh_check_rows", "pdh_values_checksum",
    "pdh_assemble_rhs_device", "pdh_evaluate_device", "pdh_shape_values_device",
    "pdh_global_error", "pdh_global_error_device", "pdh_rows_kernel_in_use", "pdh_check_terms", "pdh_terms_merge_stats", "pdh_set_problem_cartesian",
    "pdh_vmult", "pdh_vmult_device", "pdh_setup_preconditioner", "pdh_precondition_device", "pdh_solve_cg", "pdh_solve_cg_device",
    "pdh_setup_chebyshev", "pdh_chebyshev_step_device", "pdh_tridiagonal_eigenvalues",
    "pdh_residual_device", "pdh_check_transfer", "pdh_transfer_children", "pdh_transfer_create",
    "pdh_transfer_destroy", "pdh_prolongate_device", "pdh_prolongate_and_add_device", "pdh_restrict_device",
    "pdh_restrict_and_add_device", "pdh_prolongate", "pdh_restrict",
    "pdh_check_ptransfer", "pdh_ptransfer_index_map", "pdh_ptransfer_create",
    "pdh_setup_direct", "pdh_mg_create", "pdh_mg_destroy", "pdh_mg_vcycle_device",
    "pdh_set_smoother_precision", "pdh_smoother_precision", "pdh_smoother_vmult_device",
    "pdh_galerkin_plan", "pdh_galerkin_device",
    "pdh_setup_matrix_free", "pdh_matrix_free_vmult", "pdh_matrix_free_vmult_device", "pdh_set_smoother_operator", "pdh_smoother_operator",
    "pdh_check_halo", "pdh_halo_setup", "pdh_halo_pack_device", "pdh_vmult_local_device", "pdh_dcg_begin", "pdh_dcg_resume",
]

# (pdh_transfer_matrices_1d and pdh_ptransfer_matrix_1d are bound below like the others; tests/test_capi_cpu.py matches this list against the names of
# include/polydeal_hip.h that consist of letters and underscores)
_lib = None


class _Tolerant:
    """Attribute access that ignores entry points an OLDER build of the library lacks (tools/ab_bench.py loads two builds)."""

    class _Sink:
        argtypes = restype = None

    def __init__(self, lib):
        object.__setattr__(self, "_lib", lib)

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            return _Tolerant._Sink()


def _bind(lib):
    P = C.POINTER
    real, lib = lib, _Tolerant(lib)
    lib.pdh_create.argtypes = [P(C.c_void_p), C.c_int]
    lib.pdh_destroy.argtypes = [C.c_void_p]
    lib.pdh_destroy.restype = None
    lib.pdh_last_error.argtypes = [C.c_void_p]
    lib.pdh_last_error.restype = C.c_char_p
    lib.pdh_set_problem.argtypes = [C.c_void_p, P(pdh_problem)]
    lib.pdh_set_problem_local.argtypes = [C.c_void_p, P(pdh_problem), C.c_int32, C.c_int32]
    lib.pdh_set_problem_cartesian.argtypes = [C.c_void_p, P(pdh_problem), C.c_void_p, C.c_int32, C.c_int32]
    lib.pdh_assemble_device.argtypes = [C.c_void_p]
    lib.pdh_assemble.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdh_assemble_sip.argtypes = [C.c_void_p, P(pdh_problem), C.c_void_p]
    lib.pdh_assemble_sip_local.argtypes = [C.c_void_p, P(pdh_problem), C.c_int32, C.c_int32, C.c_void_p]
    lib.pdh_assemble_rhs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pdh_evaluate.argtypes = [C.c_void_p] * 6
    lib.pdh_set_algorithm.argtypes = [C.c_void_p, C.c_int]
    lib.pdh_set_overlap.argtypes = [C.c_void_p, C.c_int]
    lib.pdh_algorithm_in_use.argtypes = [C.c_void_p]
    lib.pdh_rows_kernel_in_use.argtypes = [C.c_void_p]
    lib.pdh_check_terms.argtypes = [P(pdh_problem), C.c_int32, C.c_int32, P(C.c_int64)]
    lib.pdh_terms_merge_stats.argtypes = [C.c_void_p, P(C.c_int64)]
    lib.pdh_set_exchange_mode.argtypes = [C.c_void_p, C.c_int]
    lib.pdh_exchange_layout.argtypes = [C.c_void_p, C.c_int, P(C.c_int64), P(C.c_int64)]
    lib.pdh_exchange_get_send.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdh_exchange_apply.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdh_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdh_check_exchange.argtypes = [P(pdh_problem), C.c_int32, C.c_int32, C.c_int, P(C.c_int64), P(C.c_int64)]
    lib.pdh_copy_values.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdh_check_rows.argtypes = [P(pdh_problem), C.c_int32, C.c_int32]
    lib.pdh_values_checksum.argtypes = [C.c_void_p, P(C.c_double)]
    lib.pdh_assemble_rhs_device.argtypes = [C.c_void_p] * 4
    lib.pdh_evaluate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.pdh_shape_values_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p]
    lib.pdh_shape_values.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.pdh_global_error.argtypes = [C.c_void_p] * 7 + [P(C.c_double)]
    lib.pdh_global_error_device.argtypes = [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [P(C.c_double)]
    lib.pdh_device_values.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_int64)]
    lib.pdh_synchronize.argtypes = [C.c_void_p]
    lib.pdh_stream.argtypes = [C.c_void_p]
    lib.pdh_stream.restype = C.c_void_p
    lib.pdh_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.pdh_kernel_times_ms.argtypes = [C.c_void_p, P(C.c_float), P(C.c_int)]
    lib.pdh_problem_stats.argtypes = [C.c_void_p, P(C.c_int64)]
    lib.pdh_kernel_work.argtypes = [C.c_void_p, P(C.c_int64)]
    lib.pdh_check_problem.argtypes = [P(pdh_problem), C.c_int32, C.c_int32, P(C.c_int64)]
    lib.pdh_version.restype = C.c_char_p
    lib.pdh_vmult.argtypes = [C.c_void_p] * 3
    lib.pdh_vmult_device.argtypes = [C.c_void_p] * 3
    lib.pdh_setup_preconditioner.argtypes = [C.c_void_p, C.c_int]
    lib.pdh_precondition_device.argtypes = [C.c_void_p] * 3
    lib.pdh_solve_cg.argtypes = [C.c_void_p, P(pdh_cg_control), C.c_void_p, C.c_void_p, P(pdh_cg_result)]
    lib.pdh_solve_cg_device.argtypes = [C.c_void_p, P(pdh_cg_control), C.c_void_p, C.c_void_p, P(pdh_cg_result)]
    lib.pdh_setup_chebyshev.argtypes = [C.c_void_p, P(pdh_chebyshev_control), P(pdh_chebyshev_info)]
    lib.pdh_chebyshev_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.pdh_tridiagonal_eigenvalues.argtypes = [C.c_int, C.c_void_p, C.c_void_p, P(C.c_double), P(C.c_double)]
    lib.pdh_residual_device.argtypes = [pdh_ctx_p] + [C.c_void_p] * 3
    lib.pdh_check_transfer.argtypes = [P(pdh_transfer_desc)]
    lib.pdh_transfer_matrices_1d.argtypes = [P(pdh_transfer_desc), C.c_void_p]
    lib.pdh_transfer_children.argtypes = [P(pdh_transfer_desc), C.c_void_p, C.c_void_p]
    lib.pdh_transfer_create.argtypes = [pdh_ctx_p, P(pdh_transfer_desc), P(C.c_void_p)]
    lib.pdh_transfer_destroy.argtypes = [pdh_transfer_p]
    lib.pdh_transfer_destroy.restype = None
    for name in ("pdh_prolongate_device", "pdh_prolongate_and_add_device", "pdh_restrict_device", "pdh_restrict_and_add_device",
                 "pdh_prolongate", "pdh_restrict"):
        getattr(lib, name).argtypes = [pdh_transfer_p, C.c_void_p, C.c_void_p]
    lib.pdh_check_ptransfer.argtypes = [P(pdh_ptransfer_desc)]
    lib.pdh_ptransfer_matrix_1d.argtypes = [P(pdh_ptransfer_desc), C.c_void_p]
    lib.pdh_ptransfer_index_map.argtypes = [P(pdh_ptransfer_desc), C.c_void_p]
    lib.pdh_ptransfer_create.argtypes = [pdh_ctx_p, P(pdh_ptransfer_desc), P(C.c_void_p)]
    lib.pdh_setup_direct.argtypes = [pdh_ctx_p, P(pdh_direct_info)]
    lib.pdh_mg_create.argtypes = [C.c_int, P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
    lib.pdh_mg_destroy.argtypes = [pdh_mg_p]
    lib.pdh_mg_destroy.restype = None
    lib.pdh_mg_vcycle_device.argtypes = [pdh_mg_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.pdh_set_smoother_precision.argtypes = [pdh_ctx_p, C.c_int]
    lib.pdh_smoother_precision.argtypes = [pdh_ctx_p]
    lib.pdh_smoother_vmult_device.argtypes = [pdh_ctx_p, C.c_void_p, C.c_void_p]
    lib.pdh_galerkin_plan.argtypes = [P(pdh_transfer_desc), P(pdh_galerkin_level), P(pdh_galerkin_level), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pdh_galerkin_device.argtypes = [pdh_transfer_p, pdh_ctx_p]
    lib.pdh_galerkin_matrices_1d.argtypes = [P(pdh_transfer_desc), C.c_void_p]
    lib.pdh_setup_matrix_free.argtypes = [pdh_ctx_p, P(pdh_matrix_free_info)]
    lib.pdh_matrix_free_vmult.argtypes = [pdh_ctx_p, C.c_void_p, C.c_void_p]
    lib.pdh_matrix_free_vmult_device.argtypes = [pdh_ctx_p, C.c_void_p, C.c_void_p]
    lib.pdh_set_smoother_operator.argtypes = [pdh_ctx_p, C.c_int]
    lib.pdh_smoother_operator.argtypes = [pdh_ctx_p]
    lib.pdh_check_halo.argtypes = [P(pdh_problem), C.c_int32, C.c_int32, C.c_int, C.c_void_p, P(C.c_int64), P(C.c_int64), P(pdh_halo_info)]
    lib.pdh_halo_setup.argtypes = [pdh_ctx_p, C.c_int, C.c_void_p, P(C.c_int64), P(C.c_int64), P(pdh_halo_info)]
    lib.pdh_halo_pack_device.argtypes = [pdh_ctx_p, C.c_void_p, C.c_void_p]
    lib.pdh_vmult_local_device.argtypes = [pdh_ctx_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.pdh_dcg_begin.argtypes = [pdh_ctx_p, P(pdh_cg_control), C.c_void_p, C.c_void_p, P(pdh_dcg_request)]
    lib.pdh_dcg_resume.argtypes = [pdh_ctx_p, P(pdh_dcg_request), P(pdh_cg_result)]
    return real


def smoother_operator_code(op):
    """PDH_SMOOTHER_OP_* of 'stored' | 'matrix_free' (or of the code itself); ValueError for anything else"""
    if isinstance(op, str):
        if op not in _SMOOTHER_OP:
            raise ValueError("smoother operator must be 'stored' or 'matrix_free'")
        return _SMOOTHER_OP[op]
    if int(op) not in _SMOOTHER_OP.values():
        raise ValueError("smoother operator must be PDH_SMOOTHER_OP_STORED or PDH_SMOOTHER_OP_MATRIX_FREE")
    return int(op)


def tridiagonal_eigenvalues(diag, offdiag):
    """(smallest, largest) eigenvalue of the symmetric tridiagonal matrix (diag [k], offdiag [k-1]); host only, no GPU."""
    lib = load_library()
    d = np.ascontiguousarray(diag, dtype=np.float64)
    e = np.ascontiguousarray(offdiag, dtype=np.float64)
    if d.ndim != 1 or e.shape != (max(len(d) - 1, 0),):
        raise ValueError("diag [k] and offdiag [k-1]")
    lo, hi = C.c_double(), C.c_double()
    rc = lib.pdh_tridiagonal_eigenvalues(len(d), d.ctypes.data, e.ctypes.data if len(e) else None, C.byref(lo), C.byref(hi))
    if rc != PDH_OK:
        raise PdhError(rc, lib.pdh_last_error(None).decode())
    return lo.value, hi.value


def load_library(path=None):
    """Loads libpolydeal_hip.so; raises if the HIP extension has not been built.  `path` loads another build
    of the library next to the default one (tools/ab_bench.py compares two builds in one process)."""
    global _lib
    if path is not None:
        return _bind(C.CDLL(path))
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "polydeal_amd: %s not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C polydeal_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


_DTYPES = {
    "bbox": np.float64, "dof_offset": np.int32, "vq_ptr": np.int64, "vq_x": np.float64, "vq_w": np.float64,
    "face_in": np.int32, "face_out": np.int32, "fq_ptr": np.int64, "fq_x": np.float64, "fq_n": np.float64,
    "fq_w": np.float64, "fq_w_out": np.float64, "face_sigma": np.float64, "rowptr": np.int64, "colind": np.int32,
    "col_offset": np.int32, "agg_rank": np.int32,
}


def _halo_result(n_ranks, s, r, info):
    return ([int(x) for x in s[:n_ranks]], [int(x) for x in r[:n_ranks]],
            {"n_owned_rows": int(info.n_owned_rows), "n_ghost_rows": int(info.n_ghost_rows), "n_interior": int(info.n_interior),
             "n_boundary": int(info.n_boundary)})


def check_halo(prob, row_begin, row_end, row_splits):
    """pdh_check_halo (host only, no GPU): (send_count, recv_count, info) of the vector halo of the rows [row_begin, row_end) of a
    description (a Problem or anything with a `.c` pdh_problem) among the ranks of row_splits [n_ranks + 1]; counts in doubles per peer,
    info = {n_owned_rows, n_ghost_rows, n_interior, n_boundary}."""
    lib = load_library()
    sp = np.ascontiguousarray(row_splits, dtype=np.int32)
    n_ranks = len(sp) - 1
    s, r, info = (C.c_int64 * max(n_ranks, 1))(), (C.c_int64 * max(n_ranks, 1))(), pdh_halo_info()
    rc = lib.pdh_check_halo(C.byref(prob.c), row_begin, row_end, n_ranks, sp.ctypes.data, s, r, C.byref(info))
    if rc != PDH_OK:
        raise PdhError(rc, lib.pdh_last_error(None).decode())
    return _halo_result(n_ranks, s, r, info)


class Problem:
    """Owns the NumPy arrays behind a pdh_problem (keeps them alive while the struct is in use)."""

    def __init__(self, *, dim, degree, basis, n_agg, n_faces, n_rows, diag_first=1, reaction_c=0.0, local=0, vq_tensor_n=0,
                 fq_tensor_n=0, **arrays):
        self.arrays = {}
        self.c = pdh_problem()
        self.c.dim, self.c.degree, self.c.basis = dim, degree, basis
        self.c.n_agg, self.c.n_faces, self.c.n_rows = n_agg, n_faces, n_rows
        self.c.diag_first, self.c.reaction_c, self.c.local = int(diag_first), float(reaction_c), int(local)
        self.c.vq_tensor_n = int(vq_tensor_n)
        self.c.fq_tensor_n = int(fq_tensor_n)
        for name, dt in _DTYPES.items():
            a = arrays.get(name)
            if a is None:
                setattr(self.c, name, None)
                continue
            a = np.ascontiguousarray(a, dtype=dt)
            self.arrays[name] = a
            setattr(self.c, name, a.ctypes.data)

    @property
    def nnz(self):
        return int(self.arrays["rowptr"][-1])

    def check(self, row_begin=0, row_end=None):
        lib = load_library()
        stats = (C.c_int64 * 8)()
        rc = lib.pdh_check_problem(C.byref(self.c), row_begin, self.c.n_rows if row_end is None else row_end, stats)
        if rc != PDH_OK:
            raise PdhError(rc, lib.pdh_last_error(None).decode())
        return list(stats)


class TransferDesc:
    """Owns the NumPy arrays behind a pdh_transfer_desc (two nested FE_DGQ levels: boxes [n][2][dim], first dof of every polytope,
    parent of every fine polytope)."""

    def __init__(self, *, dim, degree, fine_bbox, coarse_bbox, fine_dof_offset, coarse_dof_offset, parent, n_fine_rows=None,
                 n_coarse_rows=None, basis=PDH_BASIS_DGQ):
        self.fine_bbox = np.ascontiguousarray(fine_bbox, dtype=np.float64).reshape(-1, 2, dim)
        self.coarse_bbox = np.ascontiguousarray(coarse_bbox, dtype=np.float64).reshape(-1, 2, dim)
        self.fine_dof_offset = np.ascontiguousarray(fine_dof_offset, dtype=np.int32)
        self.coarse_dof_offset = np.ascontiguousarray(coarse_dof_offset, dtype=np.int32)
        self.parent = np.ascontiguousarray(parent, dtype=np.int32)
        self.dim, self.degree, self.basis = int(dim), int(degree), int(basis)
        self.n = (self.degree + 1) ** self.dim
        self.n_fine, self.n_coarse = len(self.fine_bbox), len(self.coarse_bbox)
        if self.fine_dof_offset.shape != (self.n_fine,) or self.parent.shape != (self.n_fine,) or \
                self.coarse_dof_offset.shape != (self.n_coarse,):
            raise ValueError("fine_dof_offset / parent [n_fine] and coarse_dof_offset [n_coarse]")
        self.n_fine_rows = self.n_fine * self.n if n_fine_rows is None else int(n_fine_rows)
        self.n_coarse_rows = self.n_coarse * self.n if n_coarse_rows is None else int(n_coarse_rows)
        self.c = pdh_transfer_desc(self.dim, self.degree, self.basis, self.n_fine, self.n_coarse, self.n_fine_rows, self.n_coarse_rows,
                                   self.fine_bbox.ctypes.data, self.coarse_bbox.ctypes.data, self.fine_dof_offset.ctypes.data,
                                   self.coarse_dof_offset.ctypes.data, self.parent.ctypes.data)

    @staticmethod
    def _chk(rc):
        if rc != PDH_OK:
            raise PdhError(rc, load_library().pdh_last_error(None).decode())

    def check(self):
        """pdh_check_transfer: host only, no GPU."""
        self._chk(load_library().pdh_check_transfer(C.byref(self.c)))

    def matrices_1d(self):
        """[n_fine][dim][p+1][p+1]: B_c[i][j], the 1-D factors of every injection block (host only)."""
        out = np.empty((self.n_fine, self.dim, self.degree + 1, self.degree + 1))
        self._chk(load_library().pdh_transfer_matrices_1d(C.byref(self.c), out.ctypes.data))
        return out

    def galerkin_matrices_1d(self):
        """[n_fine][dim][p+1][p+1]: the 1-D factors pdh_galerkin_device applies - matrices_1d() with the rows of fine support points that
        are coarse ones made exact unit vectors (host only)."""
        out = np.empty((self.n_fine, self.dim, self.degree + 1, self.degree + 1))
        self._chk(load_library().pdh_galerkin_matrices_1d(C.byref(self.c), out.ctypes.data))
        return out

    def children(self):
        """(child_ptr [n_coarse+1], child_idx [n_fine]): the summation order of the restriction (host only)."""
        ptr, idx = np.empty(self.n_coarse + 1, dtype=np.int32), np.empty(self.n_fine, dtype=np.int32)
        self._chk(load_library().pdh_transfer_children(C.byref(self.c), ptr.ctypes.data, idx.ctypes.data))
        return ptr, idx


class PTransferDesc:
    """Owns the NumPy arrays behind a pdh_ptransfer_desc: the SAME polytopes at a lower (coarse) and a higher (fine) degree of one kind
    of basis; first dof of every polytope on both levels."""

    def __init__(self, *, dim, fine_degree, coarse_degree, fine_dof_offset, coarse_dof_offset, n_fine_rows=None, n_coarse_rows=None,
                 basis=PDH_BASIS_DGQ):
        import math

        self.fine_dof_offset = np.ascontiguousarray(fine_dof_offset, dtype=np.int32)
        self.coarse_dof_offset = np.ascontiguousarray(coarse_dof_offset, dtype=np.int32)
        self.dim, self.fine_degree, self.coarse_degree, self.basis = int(dim), int(fine_degree), int(coarse_degree), int(basis)
        self.n_polytopes = len(self.fine_dof_offset)
        if self.fine_dof_offset.ndim != 1 or self.coarse_dof_offset.shape != (self.n_polytopes,):
            raise ValueError("fine_dof_offset and coarse_dof_offset [n_polytopes]")

        def n(degree):
            return (degree + 1) ** self.dim if self.basis == PDH_BASIS_DGQ else math.comb(max(degree, 0) + self.dim, self.dim)
        self.n_f, self.n_c = n(self.fine_degree), n(self.coarse_degree)
        self.n_fine_rows = self.n_polytopes * self.n_f if n_fine_rows is None else int(n_fine_rows)
        self.n_coarse_rows = self.n_polytopes * self.n_c if n_coarse_rows is None else int(n_coarse_rows)
        self.c = pdh_ptransfer_desc(self.dim, self.fine_degree, self.coarse_degree, self.basis, self.n_polytopes, self.n_fine_rows,
                                    self.n_coarse_rows, self.fine_dof_offset.ctypes.data, self.coarse_dof_offset.ctypes.data)

    _chk = staticmethod(TransferDesc._chk)

    def check(self):
        """pdh_check_ptransfer: host only, no GPU."""
        self._chk(load_library().pdh_check_ptransfer(C.byref(self.c)))

    def matrix_1d(self):
        """FE_DGQ, [p+1][q+1]: B[i][j] = l^q_j(node^p_i), the 1-D factor of every injection block (host only)."""
        out = np.empty((self.fine_degree + 1, self.coarse_degree + 1))
        self._chk(load_library().pdh_ptransfer_matrix_1d(C.byref(self.c), out.ctypes.data))
        return out

    def index_map(self):
        """FE_AggloDGP, [n_c]: the fine dof that is coarse dof j (host only)."""
        out = np.empty(self.n_c, dtype=np.int32)
        self._chk(load_library().pdh_ptransfer_index_map(C.byref(self.c), out.ctypes.data))
        return out


class GalerkinLevel:
    """Owns the NumPy arrays behind a pdh_galerkin_level: the block lists of one level's resident rows (slot s = polytope s; blk_dof
    [blk_ptr[s] + t] = first global dof of the t-th block of its rows in value order) and what the refusals of galerkin_plan read."""

    def __init__(self, *, blk_ptr, blk_dof, dof_offset, n_rows, n_rows_owned=None, exchange_mode=0, device=0):
        self.blk_ptr = np.ascontiguousarray(blk_ptr, dtype=np.int64)
        self.blk_dof = np.ascontiguousarray(blk_dof, dtype=np.int32)
        self.dof_offset = np.ascontiguousarray(dof_offset, dtype=np.int32)
        if self.blk_ptr.shape != (len(self.dof_offset) + 1,) or self.blk_dof.shape != (int(self.blk_ptr[-1]),):
            raise ValueError("blk_ptr [n_slots + 1], blk_dof [blk_ptr[-1]], dof_offset [n_slots]")
        self.c = pdh_galerkin_level(len(self.dof_offset), int(n_rows if n_rows_owned is None else n_rows_owned), int(n_rows),
                                    int(exchange_mode), int(device), self.blk_ptr.ctypes.data, self.blk_dof.ctypes.data,
                                    self.dof_offset.ctypes.data)


def galerkin_plan(desc: TransferDesc, fine: GalerkinLevel, coarse: GalerkinLevel):
    """pdh_galerkin_plan (host only, no GPU): (plan_ptr [n coarse blocks + 1], plan_slot, plan_pos [n fine blocks]) - the fine blocks
    (slot, block position) every coarse block of P^T A P receives, in summation order."""
    lib = load_library()
    ptr = np.empty(int(coarse.blk_ptr[-1]) + 1, dtype=np.int64)
    slot, pos = np.empty(int(fine.blk_ptr[-1]), dtype=np.int32), np.empty(int(fine.blk_ptr[-1]), dtype=np.int32)
    rc = lib.pdh_galerkin_plan(C.byref(desc.c), C.byref(fine.c), C.byref(coarse.c), ptr.ctypes.data, slot.ctypes.data, pos.ctypes.data)
    if rc != PDH_OK:
        raise PdhError(rc, lib.pdh_last_error(None).decode())
    return ptr, slot, pos


class Transfer:
    """pdh_transfer wrapper: prolongation / restriction between two nested levels (a TransferDesc) or two degrees on the same polytopes
    (a PTransferDesc) on the device and stream of `ctx`, which needs no resident problem.  Close it before its context."""

    def __init__(self, ctx, desc):
        self.ctx, self.lib, self.desc = ctx, ctx.lib, desc
        h = C.c_void_p()
        create = self.lib.pdh_ptransfer_create if isinstance(desc, PTransferDesc) else self.lib.pdh_transfer_create
        ctx._chk(create(ctx.h, C.byref(desc.c), C.byref(h)))
        self.h = h

    def _dev(self, fn, d_src, d_dst):
        self.ctx._chk(fn(self.h, C.c_void_p(d_src), C.c_void_p(d_dst)))

    def prolongate_device(self, d_coarse, d_fine):
        """fine = P coarse; device pointers (ints), asynchronous on the context's stream."""
        self._dev(self.lib.pdh_prolongate_device, d_coarse, d_fine)

    def prolongate_and_add_device(self, d_coarse, d_fine):
        """fine += P coarse"""
        self._dev(self.lib.pdh_prolongate_and_add_device, d_coarse, d_fine)

    def restrict_device(self, d_fine, d_coarse):
        """coarse = P^T fine"""
        self._dev(self.lib.pdh_restrict_device, d_fine, d_coarse)

    def restrict_and_add_device(self, d_fine, d_coarse):
        """coarse += P^T fine"""
        self._dev(self.lib.pdh_restrict_and_add_device, d_fine, d_coarse)

    def galerkin_device(self, coarse_ctx):
        """The values of `coarse_ctx` (a Context with its problem resident: the pattern is all it needs) become P^T A P, A the values of
        this transfer's context as they stand (pdh_galerkin_device).  Synchronises; a preconditioner of `coarse_ctx` set up before is
        stale afterwards."""
        self.ctx._chk(self.lib.pdh_galerkin_device(self.h, coarse_ctx.h))

    def _host(self, fn, src, n_src, n_dst):
        a = np.ascontiguousarray(src, dtype=np.float64)
        if a.shape != (n_src,):
            raise ValueError("the source vector must have %d entries" % n_src)
        out = np.empty(n_dst)
        self.ctx._chk(fn(self.h, C.c_void_p(a.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    def prolongate(self, coarse):
        """P coarse for a host array"""
        return self._host(self.lib.pdh_prolongate, coarse, self.desc.n_coarse_rows, self.desc.n_fine_rows)

    def restrict(self, fine):
        """P^T fine for a host array"""
        return self._host(self.lib.pdh_restrict, fine, self.desc.n_fine_rows, self.desc.n_coarse_rows)

    def close(self):
        if self.h:
            self.lib.pdh_transfer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:  # a context closed first took the device with it: nothing to free through
                self.close()
        except Exception:
            pass


class Multigrid:
    """pdh_mg wrapper: the V-cycle over `levels` (Contexts, coarse to fine, each with its assembled matrix; Chebyshev set up on every
    level above the coarsest, any preconditioner - setup_direct - on the coarsest) and `transfers` (transfers[l] between level l and
    l + 1, created on levels[l + 1]).  Creating it makes the cycle the preconditioner of the finest context: precondition_device and
    solve_cg* there.  Errors are reported on the finest context.  Close it before its transfers and contexts."""

    def __init__(self, levels, transfers):
        self.levels, self.transfers = list(levels), list(transfers)
        self.finest = self.levels[-1]
        self.lib = self.finest.lib
        lv = (C.c_void_p * len(self.levels))(*[c.h.value for c in self.levels])
        tr = (C.c_void_p * max(len(self.transfers), 1))(*[t.h.value for t in self.transfers])
        h = C.c_void_p()
        self.h = None
        self.finest._chk(self.lib.pdh_mg_create(len(self.levels), lv, tr, C.byref(h)))
        self.h = h

    def vcycle_device(self, d_b, d_x, zero_initial_guess=False):
        """One V-cycle on x for the right-hand side b (device pointers as ints, the finest level's size), queued on the finest
        context's stream."""
        self.finest._chk(self.lib.pdh_mg_vcycle_device(self.h, C.c_void_p(d_b), C.c_void_p(d_x), int(bool(zero_initial_guess))))

    def close(self):
        if self.h:
            self.lib.pdh_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.finest.h:  # (as Transfer: a context closed first took the device with it)
                self.close()
        except Exception:
            pass


def _request(req):
    return {"kind": int(req.kind), "d_send": req.d_send or 0, "d_recv": req.d_recv or 0, "d_scalars": req.d_scalars or 0,
            "n_scalars": int(req.n_scalars)}


class Context:
    """pdh_ctx wrapper (one per device and host thread)."""

    def __init__(self, device=0, lib_path=None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.pdh_create(C.byref(h), device)
        if rc != PDH_OK:
            raise PdhError(rc, self.lib.pdh_last_error(None).decode())
        self.h = h
        self.n_values = 0

    def _chk(self, rc):
        if rc != PDH_OK:
            raise PdhError(rc, self.lib.pdh_last_error(self.h).decode())

    def set_problem(self, prob, row_begin=0, row_end=None):
        """prob: a Problem (NumPy-backed) or anything with a `.c` pdh_problem (e.g. handler.FlatView)."""
        row_end = prob.c.n_rows if row_end is None else row_end
        cart = getattr(prob, "cartesian", None)
        if cart:  # a flatten_cartesian view: the points are generated on the device
            self._chk(self.lib.pdh_set_problem_cartesian(self.h, C.byref(prob.c), C.c_void_p(cart), row_begin, row_end))
        else:
            self._chk(self.lib.pdh_set_problem_local(self.h, C.byref(prob.c), row_begin, row_end))
        st = self.stats()
        self.n_values = st["n_values"]
        self.n_rows, self.n_rows_owned = int(prob.c.n_rows), st["n_owned_agg"] * st["dofs_per_cell"]
        off = np.array((C.c_int32 * prob.c.n_agg).from_address(int(prob.c.dof_offset)), dtype=np.int64)
        self._owned = (off >= row_begin) & (off < row_end)  # polytopes whose rows live here

    def owned_point_mask(self, pt_ptr):
        """Boolean mask over per-polytope CSR points: True for the points of polytopes owned by this context."""
        ptr = np.asarray(pt_ptr, dtype=np.int64)
        return np.repeat(self._owned, np.diff(ptr))

    def assemble_device(self):
        self._chk(self.lib.pdh_assemble_device(self.h))

    def synchronize(self):
        self._chk(self.lib.pdh_synchronize(self.h))

    def assemble(self):
        out = np.empty(self.n_values, dtype=np.float64)
        self._chk(self.lib.pdh_assemble(self.h, out.ctypes.data))
        return out

    def checksum(self):
        """{sum, abs_sum, max_abs, non_finite} of the values as they stand in HBM (one device pass, nothing copied back)."""
        o = (C.c_double * 4)()
        self._chk(self.lib.pdh_values_checksum(self.h, o))
        return {"sum": float(o[0]), "abs_sum": float(o[1]), "max_abs": float(o[2]), "non_finite": int(o[3])}

    def values(self):
        """The CSR values as they stand in HBM (no re-assembly)."""
        out = np.empty(self.n_values, dtype=np.float64)
        self._chk(self.lib.pdh_copy_values(self.h, out.ctypes.data))
        return out

    def assemble_rhs(self, f_vol=None, g_bdry=None):
        """rhs of the owned rows; f_vol / g_bdry sampled at the caller's volume / face quadrature points."""
        n_rows = self.stats()["n_owned_agg"] * self.stats()["dofs_per_cell"]
        out = np.empty(n_rows, dtype=np.float64)
        fv = None if f_vol is None else np.ascontiguousarray(f_vol, dtype=np.float64)
        gb = None if g_bdry is None else np.ascontiguousarray(g_bdry, dtype=np.float64)
        self._chk(self.lib.pdh_assemble_rhs(self.h, None if fv is None else fv.ctypes.data,
                                            None if gb is None else gb.ctypes.data, out.ctypes.data))
        return out

    def assemble_rhs_device(self, d_f_vol, d_g_bdry, d_rhs):
        """Device pointers (ints or None), caller order; asynchronous on the context's stream."""
        self._chk(self.lib.pdh_assemble_rhs_device(self.h, C.c_void_p(d_f_vol or 0), C.c_void_p(d_g_bdry or 0), C.c_void_p(d_rhs)))

    def evaluate_device(self, d_solution, d_pt_ptr, d_pts, n_points, d_u, d_grad=None):
        self._chk(self.lib.pdh_evaluate_device(self.h, C.c_void_p(d_solution), C.c_void_p(d_pt_ptr), C.c_void_p(d_pts), n_points,
                                               C.c_void_p(d_u), C.c_void_p(d_grad or 0)))

    def evaluate(self, solution, pt_ptr, pts, want_grad=False):
        """u_h (and grad u_h) at caller-given real points; pt_ptr [n_agg+1], pts [dim][N]."""
        sol = np.ascontiguousarray(solution, dtype=np.float64)
        ptr = np.ascontiguousarray(pt_ptr, dtype=np.int64)
        p = np.ascontiguousarray(pts, dtype=np.float64)
        n = int(ptr[-1])
        u = np.zeros(n)
        g = np.zeros((p.shape[0], n)) if want_grad else None
        self._chk(self.lib.pdh_evaluate(self.h, sol.ctypes.data, ptr.ctypes.data, p.ctypes.data, u.ctypes.data,
                                        None if g is None else g.ctypes.data))
        return (u, g) if want_grad else u

    def global_error_sums(self, solution, pt_ptr, pts, w, exact_u, exact_grad):
        """(sum w (u - u_h)^2, sum w |grad u - grad u_h|^2) over the owned polytopes, formed on the device
        (pdh_global_error); exact_u [N], exact_grad [dim][N] sampled at pts [dim][N]."""
        sol = np.ascontiguousarray(solution, dtype=np.float64)
        ptr = np.ascontiguousarray(pt_ptr, dtype=np.int64)
        p = np.ascontiguousarray(pts, dtype=np.float64)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        eu = np.ascontiguousarray(exact_u, dtype=np.float64)
        eg = np.ascontiguousarray(exact_grad, dtype=np.float64)
        n = int(ptr[-1])
        if ww.shape != (n,) or eu.shape != (n,) or eg.shape != (p.shape[0], n) or p.shape[1] != n:
            raise ValueError("w / exact_u [N], exact_grad / pts [dim][N] with N = pt_ptr[-1]")
        out = (C.c_double * 2)()
        self._chk(self.lib.pdh_global_error(self.h, sol.ctypes.data, ptr.ctypes.data, p.ctypes.data, ww.ctypes.data,
                                            eu.ctypes.data, eg.ctypes.data, out))
        return float(out[0]), float(out[1])

    def global_error_sums_device(self, d_solution, d_pt_ptr, d_pts, n_points, d_w, d_exact_u, d_exact_grad):
        out = (C.c_double * 2)()
        self._chk(self.lib.pdh_global_error_device(self.h, C.c_void_p(d_solution), C.c_void_p(d_pt_ptr), C.c_void_p(d_pts), n_points,
                                                   C.c_void_p(d_w), C.c_void_p(d_exact_u), C.c_void_p(d_exact_grad), out))
        return float(out[0]), float(out[1])

    def shape_values(self, dim, degree, basis, bbox, pt_ptr, pts):
        """phi_j(x_q) of the box basis (dim, degree, basis) for every box's points: [N][n]."""
        bb = np.ascontiguousarray(bbox, dtype=np.float64).reshape(-1, 2 * dim)
        ptr = np.ascontiguousarray(pt_ptr, dtype=np.int64)
        p = np.ascontiguousarray(pts, dtype=np.float64)
        from .handler import FiniteElement
        n = FiniteElement(dim, degree, basis).n_dofs_per_cell
        out = np.zeros((int(ptr[-1]), n))
        self._chk(self.lib.pdh_shape_values(self.h, dim, degree, basis, bb.shape[0], bb.ctypes.data, ptr.ctypes.data,
                                            p.ctypes.data, out.ctypes.data))
        return out

    def device_values(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.lib.pdh_device_values(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def poison_values(self):
        """Tests: overwrite the resident CSR values with NaN bit patterns (0xFF bytes), so that a value an assembly fails
        to write is seen."""
        ptr, n = self.device_values()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.synchronize()
        if hip.hipMemset(C.c_void_p(ptr), 0xFF, C.c_size_t(8 * n)) != 0 or hip.hipDeviceSynchronize() != 0:
            raise PdhError(-1, "hipMemset of the values failed")

    # -- solving with the resident matrix (include/polydeal_hip.h: pdh_vmult, pdh_setup_preconditioner, pdh_solve_cg) ------
    def vmult(self, x):
        """A x for the owned rows; x [n_rows] in the global dof numbering."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.shape != (self.n_rows,):
            raise ValueError("x must have n_rows = %d entries" % self.n_rows)
        y = np.empty(self.n_rows_owned)
        self._chk(self.lib.pdh_vmult(self.h, xx.ctypes.data, y.ctypes.data))
        return y

    def vmult_device(self, d_x, d_y):
        """Device pointers (ints); asynchronous on the context's stream."""
        self._chk(self.lib.pdh_vmult_device(self.h, C.c_void_p(d_x), C.c_void_p(d_y)))

    def residual_device(self, d_b, d_x, d_r):
        """r = b - A x on the resident values; device pointers (ints), asynchronous on the context's stream."""
        self._chk(self.lib.pdh_residual_device(self.h, C.c_void_p(d_b), C.c_void_p(d_x), C.c_void_p(d_r)))

    def setup_preconditioner(self, kind):
        """'none' | 'jacobi' | 'block_jacobi' (or PDH_PREC_*), built from the values as they stand."""
        self._chk(self.lib.pdh_setup_preconditioner(self.h, _PREC[kind] if isinstance(kind, str) else int(kind)))

    def precondition_device(self, d_r, d_z):
        self._chk(self.lib.pdh_precondition_device(self.h, C.c_void_p(d_r), C.c_void_p(d_z)))

    def setup_chebyshev(self, inner="block_jacobi", degree=5, smoothing_range=20.0, eig_cg_n_iterations=20, max_eigenvalue=0.0):
        """Chebyshev polynomial of `degree` in P^-1 A over the inner preconditioner 'jacobi' | 'block_jacobi' (pdh_setup_chebyshev); it
        becomes the preconditioner of precondition_device and solve_cg*.  Returns {estimate, lambda_lo, lambda_hi, cg_iterations,
        degree, inner}."""
        ctl = pdh_chebyshev_control(_PREC[inner] if isinstance(inner, str) else int(inner), int(degree), float(smoothing_range),
                                    int(eig_cg_n_iterations), float(max_eigenvalue))
        info = pdh_chebyshev_info()
        self._chk(self.lib.pdh_setup_chebyshev(self.h, C.byref(ctl), C.byref(info)))
        return {"estimate": float(info.estimate), "lambda_lo": float(info.lambda_lo), "lambda_hi": float(info.lambda_hi),
                "cg_iterations": int(info.cg_iterations), "degree": int(info.degree),
                "inner": {v: k for k, v in _PREC.items()}[int(info.inner)]}

    def setup_direct(self):
        """Dense direct solve (pdh_setup_direct: at most 1024 rows): the explicit inverse becomes the preconditioner of
        precondition_device and solve_cg*.  Returns {n_rows, pivot_min, pivot_max}."""
        info = pdh_direct_info()
        self._chk(self.lib.pdh_setup_direct(self.h, C.byref(info)))
        return {"n_rows": int(info.n_rows), "pivot_min": float(info.pivot_min), "pivot_max": float(info.pivot_max)}

    def set_smoother_precision(self, precision):
        """'f32' | 'f64' (or PDH_SMOOTHER_*): with 'f32' the Chebyshev smoother set up last, and the residual of this level inside a
        V-cycle, read a float32 copy of the matrix and of the block inverses built now from the values as they stand
        (pdh_set_smoother_precision); vectors and sums stay double.  Every setup_* call goes back to 'f64'."""
        self._chk(self.lib.pdh_set_smoother_precision(self.h, _SMOOTHER[precision] if isinstance(precision, str) else int(precision)))

    @property
    def smoother_precision(self):
        """'f32' | 'f64': the one in force"""
        rc = self.lib.pdh_smoother_precision(self.h)
        if rc < 0:
            self._chk(rc)
        return {v: k for k, v in _SMOOTHER.items()}[rc]

    def smoother_vmult_device(self, d_x, d_y):
        """y = A~ x with the float32 copy of the matrix ('f32' in force); device pointers (ints), asynchronous on the context's stream."""
        self._chk(self.lib.pdh_smoother_vmult_device(self.h, C.c_void_p(d_x), C.c_void_p(d_y)))

    def setup_matrix_free(self):
        """The 1-D tables of the matrix-free SIP operator, built on the device once per resident problem (pdh_setup_matrix_free; needs the
        term kernels' plan, else PdhError PDH_EUNSUPPORTED): what the set-up reports."""
        info = pdh_matrix_free_info()
        self._chk(self.lib.pdh_setup_matrix_free(self.h, C.byref(info)))
        return {"table_bytes": int(info.table_bytes), "doubles_per_polytope": int(info.doubles_per_polytope),
                "max_cells": int(info.max_cells), "max_subfaces": int(info.max_subfaces),
                "max_interior_subfaces": int(info.max_interior_subfaces)}

    def matrix_free_vmult(self, x):
        """A x for the owned rows from the tables, no stored value read; x [n_rows] in the global dof numbering."""
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.shape != (self.n_rows,):
            raise ValueError("x must have n_rows = %d entries" % self.n_rows)
        y = np.empty(self.n_rows_owned)
        self._chk(self.lib.pdh_matrix_free_vmult(self.h, xx.ctypes.data, y.ctypes.data))
        return y

    def matrix_free_vmult_device(self, d_x, d_y):
        """Device pointers (ints); asynchronous on the context's stream."""
        self._chk(self.lib.pdh_matrix_free_vmult_device(self.h, C.c_void_p(d_x), C.c_void_p(d_y)))

    def set_smoother_operator(self, op):
        """'stored' | 'matrix_free' (or PDH_SMOOTHER_OP_*): with 'matrix_free' the products of the Chebyshev smoother set up last, and the
        residual of this level inside a V-cycle, come from the tables of setup_matrix_free instead of the stored values
        (pdh_set_smoother_operator).  Every setup_* call goes back to 'stored'."""
        self._chk(self.lib.pdh_set_smoother_operator(self.h, smoother_operator_code(op)))

    @property
    def smoother_operator(self):
        """'stored' | 'matrix_free': the one in force"""
        rc = self.lib.pdh_smoother_operator(self.h)
        if rc < 0:
            self._chk(rc)
        return {v: k for k, v in _SMOOTHER_OP.items()}[rc]

    def chebyshev_step_device(self, d_b, d_x, zero_initial_guess=False):
        """One application of the smoother to b from the x in d_x (device pointers as ints); asynchronous on the context's stream."""
        self._chk(self.lib.pdh_chebyshev_step_device(self.h, C.c_void_p(d_b), C.c_void_p(d_x), int(bool(zero_initial_guess))))

    def chebyshev_step(self, b, x=None):
        """One application of the smoother to b from x (None: from zero); host arrays, returns the new x."""
        bb = np.ascontiguousarray(b, dtype=np.float64)
        xx = np.zeros(self.n_rows) if x is None else np.array(x, dtype=np.float64, copy=True)
        if bb.shape != (self.n_rows,) or xx.shape != (self.n_rows,):
            raise ValueError("b and x must have n_rows = %d entries" % self.n_rows)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        d_b, d_x = C.c_void_p(), C.c_void_p()
        try:
            if hip.hipMalloc(C.byref(d_b), max(bb.nbytes, 8)) != 0 or hip.hipMalloc(C.byref(d_x), max(xx.nbytes, 8)) != 0:
                raise PdhError(PDH_EDEVICE, "chebyshev_step: out of device memory")
            if hip.hipMemcpy(d_b, bb.ctypes.data, bb.nbytes, 1) != 0 or hip.hipMemcpy(d_x, xx.ctypes.data, xx.nbytes, 1) != 0:
                raise PdhError(PDH_EDEVICE, "chebyshev_step: copy to the device failed")
            self.chebyshev_step_device(d_b.value, d_x.value, x is None)
            self.synchronize()
            if hip.hipMemcpy(xx.ctypes.data, d_x, xx.nbytes, 2) != 0:
                raise PdhError(PDH_EDEVICE, "chebyshev_step: copy from the device failed")
        finally:
            for p in (d_b, d_x):
                if p.value:
                    hip.hipFree(p)
        return xx

    def _cg(self, fn, b, x, rel_tol, abs_tol, max_iter, on_noconv):
        ctl = pdh_cg_control(CG_MAX_ITER if max_iter is None else int(max_iter), float(rel_tol), float(abs_tol))
        res = pdh_cg_result()
        rc = fn(self.h, C.byref(ctl), b, x, C.byref(res))
        info = {"iterations": int(res.iterations), "residual0": float(res.residual0), "residual": float(res.residual)}
        if rc == PDH_ENOCONV:
            e = PdhError(rc, self.lib.pdh_last_error(self.h).decode())
            e.info = info
            on_noconv(e)
            raise e
        self._chk(rc)
        return info

    def solve_cg(self, b, x0=None, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        """Preconditioned CG with the preconditioner set up last; returns (x, info), info = {iterations, residual0, residual}.
        PDH_ENOCONV raises PdhError carrying .x (the last iterate) and .info."""
        bb = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros(self.n_rows) if x0 is None else np.array(x0, dtype=np.float64, copy=True)
        if bb.shape != (self.n_rows,) or x.shape != (self.n_rows,):
            raise ValueError("b and x0 must have n_rows = %d entries" % self.n_rows)

        def attach(e):
            e.x = x
        info = self._cg(self.lib.pdh_solve_cg, C.c_void_p(bb.ctypes.data), C.c_void_p(x.ctypes.data), rel_tol, abs_tol, max_iter, attach)
        return x, info

    def solve_cg_device(self, d_b, d_x, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        """Device pointers (ints); d_x holds the initial guess and receives the solution.  Returns info (PDH_ENOCONV raises
        PdhError carrying .info; d_x then holds the last iterate)."""
        return self._cg(self.lib.pdh_solve_cg_device, C.c_void_p(d_b), C.c_void_p(d_x), rel_tol, abs_tol, max_iter, lambda e: None)

    # -- solving over several ranks (include/polydeal_hip.h: pdh_halo_*, pdh_vmult_local_device, pdh_dcg_*) ----------------
    def halo_setup(self, row_splits):
        """Builds the halo plan of the resident problem among the ranks of row_splits [n_ranks + 1]; returns (send_count, recv_count,
        info) like check_halo.  The local vector has info['n_owned_rows'] + info['n_ghost_rows'] doubles."""
        sp = np.ascontiguousarray(row_splits, dtype=np.int32)
        n_ranks = len(sp) - 1
        s, r, info = (C.c_int64 * max(n_ranks, 1))(), (C.c_int64 * max(n_ranks, 1))(), pdh_halo_info()
        self._chk(self.lib.pdh_halo_setup(self.h, n_ranks, sp.ctypes.data, s, r, C.byref(info)))
        return _halo_result(n_ranks, s, r, info)

    def halo_pack(self, d_v, d_send):
        """Gathers the send buffer from the owned part of the local vector; device pointers (ints), asynchronous."""
        self._chk(self.lib.pdh_halo_pack_device(self.h, C.c_void_p(d_v), C.c_void_p(d_send or 0)))

    def vmult_local(self, d_v, d_y, which="all"):
        """y = A v on the local vector for the rows of 'all' | 'interior' | 'boundary' polytopes (or PDH_ROWS_*); device pointers
        (ints), asynchronous on the context's stream."""
        self._chk(self.lib.pdh_vmult_local_device(self.h, C.c_void_p(d_v), C.c_void_p(d_y), _WHICH[which] if isinstance(which, str) else int(which)))

    def dcg_begin(self, d_b, d_x, rel_tol=1e-13, abs_tol=0.0, max_iter=None):
        """Opens a CG run over the ranks (pdh_dcg_begin); d_b, d_x [n_owned_rows] device pointers (ints).  Returns the first request
        as a dict {kind, d_send, d_recv, d_scalars, n_scalars} (kind: PDH_DCG_*)."""
        ctl = pdh_cg_control(CG_MAX_ITER if max_iter is None else int(max_iter), float(rel_tol), float(abs_tol))
        req = pdh_dcg_request()
        self._chk(self.lib.pdh_dcg_begin(self.h, C.byref(ctl), C.c_void_p(d_b), C.c_void_p(d_x), C.byref(req)))
        return _request(req)

    def dcg_resume(self):
        """Resumes the run after the caller carried out the last request: (request, info), info = {iterations, residual0, residual}
        once request['kind'] is PDH_DCG_DONE, else None.  PDH_ENOCONV raises PdhError carrying .info (the run is over)."""
        req, res = pdh_dcg_request(), pdh_cg_result()
        rc = self.lib.pdh_dcg_resume(self.h, C.byref(req), C.byref(res))
        info = {"iterations": int(res.iterations), "residual0": float(res.residual0), "residual": float(res.residual)}
        if rc == PDH_ENOCONV:
            e = PdhError(rc, self.lib.pdh_last_error(self.h).decode())
            e.info = info
            raise e
        self._chk(rc)
        return _request(req), (info if req.kind == PDH_DCG_DONE else None)

    def set_algorithm(self, alg):
        """'auto' | 'direct' (MFMA contraction over the points) | 'moment' (Legendre moments + sum factorisation)."""
        self._chk(self.lib.pdh_set_algorithm(self.h, {"auto": 0, "direct": 1, "moment": 2, "rows": 4}[alg]))

    def set_exchange_mode(self, mode):
        """'none': owner-computes-rows (no matrix traffic); 'ghost': the reference's scheme - the owner of a cut face ships
        M21 / M22 to the owner of those rows (needs agg_rank in the problem).  Takes effect at the next set_problem."""
        self._chk(self.lib.pdh_set_exchange_mode(self.h, {"none": 0, "ghost": 1}[mode]))

    def exchange_layout(self, n_ranks):
        """(send_count, recv_count): doubles per peer rank of the ghost-block exchange."""
        s = (C.c_int64 * n_ranks)()
        r = (C.c_int64 * n_ranks)()
        self._chk(self.lib.pdh_exchange_layout(self.h, n_ranks, s, r))
        return [int(x) for x in s], [int(x) for x in r]

    def exchange_get_send(self, d_send_ptr):
        self._chk(self.lib.pdh_exchange_get_send(self.h, C.c_void_p(d_send_ptr)))

    def exchange_apply(self, d_recv_ptr):
        self._chk(self.lib.pdh_exchange_apply(self.h, C.c_void_p(d_recv_ptr)))

    def set_stream(self, stream_handle):
        """Launch on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); None: own stream."""
        self._chk(self.lib.pdh_set_stream(self.h, C.c_void_p(stream_handle or 0)))

    def set_overlap(self, on=True):
        """Run the two kernels of a step concurrently on large problems (default) or strictly one after the other."""
        self._chk(self.lib.pdh_set_overlap(self.h, int(on)))

    def algorithm_in_use(self):
        rc = self.lib.pdh_algorithm_in_use(self.h)
        if rc < 0:
            self._chk(rc)
        return {1: "direct", 2: "moment", 3: "mixed", 4: "rows"}[rc]

    def rows_kernel_in_use(self):
        """Which row kernel serves the resident problem (include/polydeal_hip.h: PDH_ROWS_*)."""
        rc = self.lib.pdh_rows_kernel_in_use(self.h)
        if rc < 0:
            self._chk(rc)
        return {0: "none", 1: "pieces", 2: "multi", 3: "streamed", 4: "terms"}[rc]

    def terms_merge_stats(self):
        """Term kernels: {cells, cells_merged, sub_faces, sub_faces_merged} of the owned polytopes (pdh_terms_merge_stats)."""
        out = (C.c_int64 * 4)()
        self._chk(self.lib.pdh_terms_merge_stats(self.h, out))
        return dict(cells=out[0], cells_merged=out[1], sub_faces=out[2], sub_faces_merged=out[3])

    def set_profiling(self, on=True):
        self._chk(self.lib.pdh_set_profiling(self.h, int(on)))

    def kernel_times_ms(self):
        ms = (C.c_float * 2)()
        n = C.c_int()
        self._chk(self.lib.pdh_kernel_times_ms(self.h, ms, C.byref(n)))
        return [float(ms[0]), float(ms[1])], int(n.value)

    def kernel_work(self):
        """MFMA instructions (512 flop each) issued per launch by [k_diag, k_offdiag]."""
        w = (C.c_int64 * 2)()
        self._chk(self.lib.pdh_kernel_work(self.h, w))
        return [int(w[0]), int(w[1])]

    def stats(self):
        st = (C.c_int64 * 8)()
        self._chk(self.lib.pdh_problem_stats(self.h, st))
        keys = ["n_owned_agg", "n_offdiag_items", "n_vq_points", "n_face_side_points", "n_values",
                "dofs_per_cell", "lds_bytes_diag", "lds_bytes_offdiag"]
        return dict(zip(keys, [int(x) for x in st]))

    def close(self):
        if self.h:
            self.lib.pdh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
