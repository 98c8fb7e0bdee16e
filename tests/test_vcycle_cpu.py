"""The V-cycle's NumPy restatement (tests/vcycle_ref.py) on oracle-assembled matrices, no GPU: the applied cycle is a symmetric positive
operator, PCG with it needs fewer iterations than PCG with Chebyshev(3) and its count does not grow with the mesh; the restatement's
long-double tools agree with each other; header and ctypes agree on what the feature adds."""
import os
import re

import numpy as np
import pytest

import cheb_ref as cr
import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL = 1e-10  # of the PCG runs


@pytest.mark.parametrize("case", vc.CPU_CASES, ids=vc.case_id)
def test_the_cycle_is_symmetric(case):
    """u^T M v = v^T M u for the applied cycle M (from zero), within 1e-12 |u| |M v|"""
    H = vc.oracle_hierarchy(case)
    rng = np.random.default_rng(5)
    N = H.mats[-1].shape[0]
    for _ in range(3):
        u, v = rng.standard_normal(N), rng.standard_normal(N)
        Mv, Mu = vr.cycle(H, v), vr.cycle(H, u)
        a, b = float(u @ Mv), float(v @ Mu)
        scale = float(np.linalg.norm(u) * np.linalg.norm(Mv))
        print("%s: u^T M v = %.15e, v^T M u = %.15e, difference / scale = %.3e" % (vc.case_id(case), a, b, abs(a - b) / scale))
        assert abs(a - b) <= 1e-12 * scale


def test_the_cycle_is_positive():
    """dense eigenvalues of the applied cycle on the 256-row case"""
    H = vc.oracle_hierarchy(vc.CASES[0])
    N = H.mats[-1].shape[0]
    assert N == 256
    M = np.stack([vr.cycle(H, e) for e in np.eye(N)], axis=1)
    assert np.max(np.abs(M - M.T)) <= 1e-12 * np.max(np.abs(M))
    ev = np.linalg.eigvalsh((M + M.T) / 2)
    print("eigenvalues of the cycle: %.3e .. %.3e; of M A: %.4f .. %.4f" % (ev[0], ev[-1], *np.sort(np.linalg.eigvals(M @ H.mats[-1].toarray()).real)[[0, -1]]))
    assert ev[0] > 0


def _counts(case):
    H = vc.oracle_hierarchy(case)
    A = H.mats[-1]
    b = vc.rhs(A.shape[0])
    lo, hi = H.bounds[-1]
    _, it_mg, _ = pcg_ref.pcg(A, b, vr.preconditioner(H), rel_tol=REL_TOL)
    _, it_ch, _ = pcg_ref.pcg(A, b, cr.chebyshev_preconditioner(A, H.n, H.kind, lo, hi, vc.DEGREE), rel_tol=REL_TOL)
    return it_mg, it_ch


@pytest.mark.parametrize("case", vc.CPU_CASES, ids=vc.case_id)
def test_pcg_with_the_cycle_beats_chebyshev(case):
    it_mg, it_ch = _counts(case)
    print("%s: PCG iterations to %.0e: V-cycle %d, Chebyshev(%d) %d" % (vc.case_id(case), REL_TOL, it_mg, vc.DEGREE, it_ch))
    assert it_mg < it_ch


def test_the_count_does_not_grow_with_the_mesh():
    counts = []
    for case in vc.MESH_PAIR:
        H = vc.oracle_hierarchy(case)
        A = H.mats[-1]
        counts.append(pcg_ref.pcg(A, vc.rhs(A.shape[0]), vr.preconditioner(H), rel_tol=REL_TOL)[1])
    print("PCG iterations with the V-cycle, one refinement apart: %s" % counts)
    assert abs(counts[0] - counts[1]) <= 3


def test_long_double_inverse_agrees_with_gauss_jordan():
    """vcycle_ref.inverse_longdouble (float64 inverse + one refinement step with an exactly split product) against cheb_ref's long-double
    Gauss-Jordan sweep on the 125-row matrix: both are long-double answers, they differ by the sweep's own rounding"""
    D = np.asarray(vc.direct_oracle_matrix(vc.DIRECT_SIZES[2]).todense())
    G = vr.inverse_longdouble(D)
    ref = cr.batched_inverse(D[None], np.longdouble)[0]
    err = float(np.max(np.abs(G - ref)) / np.max(np.abs(ref)))
    cond = float(np.linalg.cond(D))
    print("refined inverse against Gauss-Jordan: %.3e (cond %.3e)" % (err, cond))
    assert err <= 100 * cond * float(np.finfo(np.longdouble).eps)
    cols = vc.direct_columns(1024)
    assert len(cols) == vc.DIRECT_FEW_COLUMNS and cols[0] == 0 and cols[-1] == 1023
    assert np.array_equal(vr.inverse_longdouble(D, cols[cols < 125]), G[:, cols[cols < 125]])


def test_direct_sizes_are_what_they_say():
    rows = [s[1] for s in vc.DIRECT_SIZES]
    assert rows == [9, 64, 125, 576, 1000, 1024] and vc.DIRECT_REFUSED[1] == 1600
    for size in vc.DIRECT_SIZES + [vc.DIRECT_REFUSED]:
        vc.direct_handler(size)  # asserts its row count
    for case in vc.CASES:
        vc.check_shape(case, vc.handlers(*case)[0])


def test_header_and_ctypes_agree_on_the_new_structs_and_codes():
    from polydeal_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "polydeal_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(PDH_\w+)\s+(-?\d+)", hdr)}
    assert defs["PDH_PREC_DIRECT"] == _capi.PDH_PREC_DIRECT == 4
    assert defs["PDH_PREC_MULTIGRID"] == _capi.PDH_PREC_MULTIGRID == 5
    assert len({v for k, v in defs.items() if k.startswith("PDH_PREC_")}) == 6
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctype = {"int32_t": "c_int", "double": "c_double"}
    text = re.search(r"typedef struct pdh_direct_info\s*\{(.*?)\}", body, re.S).group(1)
    fields = []
    for t, names in re.findall(r"(\w+)\s+([\w\s,]+);", text):
        fields += [(nm.strip(), ctype[t]) for nm in names.split(",")]
    assert [(f[0], f[1].__name__.replace("c_int32", "c_int")) for f in _capi.pdh_direct_info._fields_] == fields
    assert re.search(r"typedef struct pdh_mg pdh_mg;", body)
    for sym in ("pdh_setup_direct", "pdh_mg_create", "pdh_mg_destroy", "pdh_mg_vcycle_device"):
        assert sym in _capi.EXPORTS and re.search(r"\b%s\s*\(" % sym, body), sym
    if os.path.exists(_capi.LIB_PATH):
        lib = _capi.load_library()
        assert lib.pdh_setup_direct.argtypes[0] is _capi.pdh_ctx_p
        assert lib.pdh_mg_vcycle_device.argtypes[0] is _capi.pdh_mg_p and lib.pdh_mg_destroy.restype is None
