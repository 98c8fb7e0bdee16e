"""C ABI checks that need no GPU: the library loads, exports every symbol include/polydeal_hip.h
declares, validates problem descriptions, and refuses to compute without a HIP device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import polydeal_amd as pa
from polydeal_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    hdr = open(os.path.join(ROOT, "include", "polydeal_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pdh_[a-z_]+)\s*\(", hdr))
    declared -= {"pdh_ctx", "pdh_problem"}
    assert len(declared) >= 17
    lib = pa.load_library()
    for sym in sorted(declared):
        assert hasattr(lib, sym), sym
    assert set(_capi.EXPORTS) == declared
    assert b"gfx950" in lib.pdh_version()


def small_problem(dim=2, basis="dgp", p=2, refine=2):
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, refine)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, True)
    kw = {k: (None if v is None else np.array(v)) for k, v in flat.arrays().items()}
    c = flat.c
    kw.update(dim=c.dim, degree=c.degree, basis=c.basis, n_agg=c.n_agg, n_faces=c.n_faces, n_rows=c.n_rows,
              diag_first=c.diag_first, reaction_c=c.reaction_c)
    return kw


def test_check_problem_accepts_valid_and_reports_stats():
    kw = small_problem()
    st = pa.Problem(**kw).check()
    assert st[0] == kw["n_agg"] and st[4] == kw["rowptr"][-1] and st[5] == 6
    assert st[1] == int(np.sum(kw["face_out"] >= 0))  # one coupling item per interior face (A[Q,P] = A[P,Q]^T)
    assert st[2] == kw["vq_ptr"][-1]


@pytest.mark.parametrize("mutate,code", [
    (lambda k: k.update(dim=4), _capi.PDH_EINVAL),
    (lambda k: k.update(basis=7), _capi.PDH_EINVAL),
    (lambda k: k.update(n_rows=k["n_rows"] + 1), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("dof_offset", k["dof_offset"] + 1), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("bbox", np.zeros_like(k["bbox"])), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("face_out", np.where(k["face_out"] >= 0, k["n_agg"] + 3, -1)), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("rowptr", k["rowptr"] * 2), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("colind", k["colind"][::-1].copy()), _capi.PDH_EINVAL),
    (lambda k: k.__setitem__("vq_w", None), _capi.PDH_EINVAL),
])
def test_check_problem_rejects_malformed(mutate, code):
    kw = small_problem()
    mutate(kw)
    with pytest.raises(pa.PdhError) as ei:
        pa.Problem(**kw).check()
    assert ei.value.code == code


def test_unsupported_block_size_is_reported_not_silently_wrong():
    kw = small_problem(dim=3, basis="dgq", p=4, refine=1)  # n = 125 > 64: taken since round 4 (64 x 64 tiles, csrc/pdh_tiled.h)
    assert pa.Problem(**kw).check()[5] == 125
    kw = small_problem(dim=2, basis="dgq", p=8, refine=1)  # n = 81 in 2-D: degree 8 has no kernel anywhere
    with pytest.raises(pa.PdhError) as ei:
        pa.Problem(**kw).check()
    assert ei.value.code == _capi.PDH_EUNSUPPORTED


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pa.PdhError) as ei:
        pa.Context(0)
    assert ei.value.code == _capi.PDH_EDEVICE
    grid = pa.BackgroundGrid.hyper_cube_refined(2, 0.0, 1.0, 1)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(1)
    fe = pa.FE_DGQ(2, 1)
    ah.initialize_fe_values(2, 2)
    ah.distribute_agglomerated_dofs(fe)
    with pytest.raises(pa.HostError):
        pa.assemble_dg_matrix(fe, ah)


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "polydeal_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".cpp", ".hip")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "sip_ref" not in src, f


def _rows_applies(flat, r0=0, r1=None):
    lib = pa.load_library()
    lib.pdh_check_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.pdh_last_error.restype = C.c_char_p
    rc = lib.pdh_check_rows(C.byref(flat.c), r0, flat.c.n_rows if r1 is None else r1)
    return rc, (lib.pdh_last_error(None) or b"").decode()


@pytest.mark.parametrize("basis,p", [("dgq", 3), ("dgp", 3), ("dgq", 2), ("dgp", 2), ("dgq", 1), ("dgp", 1)])
def test_row_kernel_eligibility_is_decided_on_the_quadrature_data(basis, p):
    """pdh_check_rows (host only): the row kernel applies to agglomerates of Cartesian cells - planar faces and tensor rules
    are recognised on the points - and refuses distorted cells, unstructured rules (for the kinds that need tensor rules), 2-D
    problems and - for the small elements - polytopes too large for the term kernel that also have staircase faces, saying why."""
    def handler(dim, refine, groups=None, distort=0.0, nq=None):
        grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, refine)
        if distort:
            grid.distort(distort, seed=2)
        ah = pa.AgglomerationHandler(grid)
        if groups is None:
            ah.define_block_agglomerates(2)
        else:
            for g in groups:
                ah.define_agglomerate(g)
        fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(dim, p)
        ah.initialize_fe_values(nq or p + 1, nq or p + 1)
        ah.distribute_agglomerated_dofs(fe)
        return ah, fe

    ah, fe = handler(3, 2)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, False)
    assert _rows_applies(flat)[0] == 1
    n = fe.n_dofs_per_cell
    assert _rows_applies(flat, 2 * n, 5 * n)[0] == 1           # a row range
    # claims are verified, not believed; no claim = the library looks itself; negative = do not look
    flat.c.vq_tensor_n, flat.c.fq_tensor_n = 7, 7
    rc, why = _rows_applies(flat)
    assert rc == (1 if p == 3 else 0) and (p == 3 or "tensor" in why)   # degree 3 has general-point paths
    flat.c.vq_tensor_n, flat.c.fq_tensor_n = -1, -1
    assert _rows_applies(flat)[0] == (1 if p == 3 else 0)
    # distorted cells: faces are no longer planar to rounding
    ah, fe = handler(3, 2, distort=1e-6)
    rc, why = _rows_applies(ah.flatten(pa.SipVariant.poisson_example(fe), True, False))
    assert rc == 0 and ("planar" in why or "axis-aligned" in why), why
    # an L-shaped polytope touches a neighbour along two planes
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 2)
    cell = {tuple(int(round(v * 4)) for v in grid.cell_vertices(c)[0]): c for c in range(grid.n_cells)}
    groups = [sorted([cell[(0, 0, 0)], cell[(1, 0, 0)], cell[(0, 1, 0)]]), sorted([cell[(1, 1, 0)], cell[(1, 1, 1)]])]
    used = {c for g in groups for c in g}
    groups += [[c] for c in range(grid.n_cells) if c not in used]
    ah, fe = handler(3, 2, groups=groups)
    rc, why = _rows_applies(ah.flatten(pa.SipVariant.poisson_example(fe), True, False))
    # FE_DGQ(3) has the instantiation for several planes per neighbour (pdh_rows.h: MULTI), the other elements the term kernel
    # (pdh_terms.h), for which a sub-face is a sub-face whatever plane it lies in
    assert rc == 1, why
    # ... but the term kernel keeps a polytope's tables in LDS: 4^3 cells with up to 96 sub-faces exceed its budget, and with a
    # staircase face on top no row kernel is left for the small elements
    if not (basis == "dgq" and p == 3):
        grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 3)
        cell = {tuple(int(round(v * 8)) for v in grid.cell_vertices(c)[0]): c for c in range(grid.n_cells)}
        blocks = {}
        for (i, j, k), c in cell.items():
            blocks.setdefault((i // 4, j // 4, k // 4), []).append(c)
        moved = cell[(3, 0, 0)]
        blocks[(0, 0, 0)].remove(moved)
        blocks[(1, 0, 0)].append(moved)
        ah, fe = handler(3, 3, groups=[sorted(blocks[key]) for key in sorted(blocks)])
        flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, False)
        # (as given; merged - the 4 x 4 sub-faces of a plane summed over as 2 x 2 with composite rules, the intact blocks as 2^3 cells -
        # they fit: pdh_terms_tables.h)
        rc, why = _rows_applies(flat)
        if p < 3:  # (degree 3: the 63 and 65 cells of the two polytopes that are no grids any more exceed the budget by themselves)
            assert rc == 1, why
        os.environ["PDH_TERMS_MERGE"] = "0"
        try:
            rc, why = _rows_applies(flat)
        finally:
            del os.environ["PDH_TERMS_MERGE"]
        if p == 1 or (basis == "dgp" and p == 2):  # (2 x 2 matrices / ten functions with the tables in two passes: even these fit)
            assert rc == 1, why
        else:
            assert rc == 0 and "plane" in why and "LDS" in why, why
    # 2-D
    ah, fe = handler(2, 3)
    rc, why = _rows_applies(ah.flatten(pa.SipVariant.poisson_example(fe), True, False))
    assert rc == 0 and "3-D" in why, why


def test_every_entry_point_has_declared_argument_types():
    """ctypes passes an undeclared Python int as a C int: a 64-bit pointer survives that only by accident (found as a segfault
    of a new entry point on the GPU box).  Every exported function that takes arguments must have its argtypes declared."""
    from polydeal_amd import _capi

    lib = pa.load_library()
    missing = [s for s in _capi.EXPORTS if s != "pdh_version" and getattr(lib, s).argtypes is None]
    assert not missing, missing


_NULL = (_capi.PDH_EINVAL, "ctx is NULL")
_NONE_RESIDENT = (_capi.PDH_ESTATE, "no problem resident")
_NO_GHOST = (_capi.PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode")
# what every entry point that takes a context answers for ctx = NULL, every other pointer valid (transcribed from the driver's source
# before it was split into units: some answer like "no problem resident", two name their other required argument)
NULL_CTX_ANSWERS = {
    "pdh_set_problem": _NULL, "pdh_set_problem_local": _NULL, "pdh_set_problem_cartesian": _NULL,
    "pdh_assemble_device": _NULL, "pdh_assemble": _NULL, "pdh_assemble_sip": _NULL, "pdh_assemble_sip_local": _NULL,
    "pdh_device_values": _NONE_RESIDENT, "pdh_synchronize": _NULL, "pdh_set_profiling": _NULL,
    "pdh_kernel_times_ms": (_capi.PDH_EINVAL, "ctx or ms is NULL"), "pdh_problem_stats": _NONE_RESIDENT,
    "pdh_assemble_rhs": _NULL, "pdh_kernel_work": _NONE_RESIDENT, "pdh_evaluate": _NULL, "pdh_shape_values": _NULL,
    "pdh_set_algorithm": _NULL, "pdh_algorithm_in_use": _NONE_RESIDENT, "pdh_set_overlap": _NULL, "pdh_set_exchange_mode": _NULL,
    "pdh_exchange_layout": _NONE_RESIDENT, "pdh_exchange_get_send": _NO_GHOST, "pdh_exchange_apply": _NO_GHOST,
    "pdh_set_stream": _NULL, "pdh_copy_values": _NONE_RESIDENT, "pdh_values_checksum": _NONE_RESIDENT,
    "pdh_assemble_rhs_device": _NULL, "pdh_evaluate_device": _NULL, "pdh_shape_values_device": _NULL, "pdh_global_error": _NULL,
    "pdh_global_error_device": _NULL, "pdh_rows_kernel_in_use": _NONE_RESIDENT,
    "pdh_terms_merge_stats": (_capi.PDH_EINVAL, "ctx and out4 are required"),
    "pdh_vmult": _NULL, "pdh_vmult_device": _NULL, "pdh_setup_preconditioner": _NULL, "pdh_precondition_device": _NULL,
    "pdh_solve_cg": _NULL, "pdh_solve_cg_device": _NULL, "pdh_setup_chebyshev": _NULL, "pdh_chebyshev_step_device": _NULL,
    "pdh_debug_rows_stamps": (_capi.PDH_ESTATE, "no row-kernel problem resident"),  # (diagnostic, not in the public header)
}


def test_every_entry_point_answers_a_null_context_as_before():
    """ctx = NULL is an argument error answered on the host, with the code and the text of pdh_last_error(NULL) each entry point has
    always given.  Every other argument is valid, so that the answer is the one about the context."""
    lib = pa.load_library()
    lib.pdh_debug_rows_stamps.argtypes = [C.c_void_p, C.c_void_p]
    takes_ctx = {s for s in _capi.EXPORTS if (getattr(lib, s).argtypes or [None])[0] is C.c_void_p and not s.startswith("pdh_check_")}
    takes_ctx -= {"pdh_destroy", "pdh_last_error", "pdh_stream"}  # no code to return: below
    assert takes_ctx | {"pdh_debug_rows_stamps"} == set(NULL_CTX_ANSWERS)
    kw = small_problem()
    problem = pa.Problem(**kw)
    room = (C.c_double * 64)()  # what any output or input pointer may point to: never reached
    for name, (code, text) in sorted(NULL_CTX_ANSWERS.items()):
        fn = getattr(lib, name)
        args = [None]
        for t in fn.argtypes[1:]:
            if t is C.c_void_p:
                args.append(C.addressof(room))
            elif t is C.POINTER(_capi.pdh_problem):
                args.append(C.byref(problem.c))
            elif hasattr(t, "contents"):  # POINTER(struct or scalar)
                args.append(C.cast(room, t))
            else:
                args.append(0)
        lib.pdh_last_error(None)
        rc = fn(*args)
        assert (rc, lib.pdh_last_error(None).decode()) == (code, text), name
    lib.pdh_destroy(None)
    assert lib.pdh_stream(None) is None
