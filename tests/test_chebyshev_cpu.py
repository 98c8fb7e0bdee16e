"""The Chebyshev smoother's yardstick and ABI, without a GPU: the host-only tridiagonal eigenvalue routine of the planner
(pdh_tridiagonal_eigenvalues) against numpy.linalg.eigvalsh; the NumPy restatement (tests/cheb_ref.py) against the conditions that
make the polynomial a symmetric positive definite preconditioner, on the oracle matrices of tests/test_solve_cpu.py and on the cases
the GPU test runs (tests/cheb_cases.py); the header and the exported symbols."""
import os
import re

import numpy as np
import pytest

import cheb_cases as cc
import cheb_ref as cr
from oracle import polydeal_oracle as po
from pcg_ref import pcg, preconditioner
from test_solve_cpu import _oracle_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi_or_skip():
    from polydeal_amd import _capi

    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libpolydeal_hip.so not built")
    return _capi


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) pdh_tridiagonal_eigenvalues
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_tridiagonal(_capi, diag, off, what):
    lo, hi = _capi.tridiagonal_eigenvalues(diag, off)
    ev = np.linalg.eigvalsh(np.diag(diag) + np.diag(off, 1) + np.diag(off, -1))
    scale = np.max(np.abs(ev))
    print(what, len(diag), "lo %.3e hi %.3e (relative to max |lambda|)" % (abs(lo - ev[0]) / scale, abs(hi - ev[-1]) / scale))
    assert abs(lo - ev[0]) <= 1e-13 * scale and abs(hi - ev[-1]) <= 1e-13 * scale, (what, len(diag), lo, hi, ev[0], ev[-1])


def test_tridiagonal_eigenvalues_random_and_lanczos():
    """k = 1 .. 64: random symmetric tridiagonals (indefinite, entries of mixed size) and the Lanczos matrices of k CG steps on an
    oracle matrix, extreme eigenvalues within 1e-13 max |lambda| of eigvalsh."""
    _capi = _capi_or_skip()
    rng = np.random.default_rng(0)
    A, n = _oracle_system(2, 3, 2, po.FE_AggloDGP(2, 2), True)
    mv, b = cr.operator(A), cr.b0(A.shape[0])
    for k in range(1, 65):
        _check_tridiagonal(_capi, rng.standard_normal(k), rng.standard_normal(k - 1), "random")
        _check_tridiagonal(_capi, rng.standard_normal(k) * 10.0 ** rng.integers(-3, 4, k), rng.standard_normal(k - 1) * 1e-2, "graded")
        alpha, beta = cr.cg_coefficients(mv, cr.inner_preconditioner(A, n, "jacobi" if k % 2 else "block_jacobi"), b, k)
        assert len(alpha) == k
        _check_tridiagonal(_capi, *cr.lanczos_tridiagonal(alpha, beta), "lanczos")
    # a diagonal matrix, a constant one, and one whose largest eigenvalue is known: 2 - 2 cos(k pi / (k + 1))
    _check_tridiagonal(_capi, np.arange(5.0), np.zeros(4), "diagonal")
    lo, hi = _capi.tridiagonal_eigenvalues(np.full(64, 2.0), np.full(63, -1.0))
    assert abs(hi - (2 - 2 * np.cos(64 * np.pi / 65))) <= 4e-13 and abs(lo - (2 - 2 * np.cos(np.pi / 65))) <= 4e-13


def test_tridiagonal_eigenvalues_refuses_bad_input():
    _capi = _capi_or_skip()
    lib = _capi.load_library()
    import ctypes as C

    d, e = np.ones(300), np.ones(299)
    lo, hi = C.c_double(), C.c_double()
    for k, dp, ep in ((0, d, e), (257, d, e), (-1, d, e)):
        assert lib.pdh_tridiagonal_eigenvalues(k, dp.ctypes.data, ep.ctypes.data, C.byref(lo), C.byref(hi)) == _capi.PDH_EINVAL
    assert lib.pdh_tridiagonal_eigenvalues(2, None, e.ctypes.data, C.byref(lo), C.byref(hi)) == _capi.PDH_EINVAL
    assert lib.pdh_tridiagonal_eigenvalues(2, d.ctypes.data, None, C.byref(lo), C.byref(hi)) == _capi.PDH_EINVAL
    assert lib.pdh_tridiagonal_eigenvalues(1, d.ctypes.data, None, C.byref(lo), C.byref(hi)) == _capi.PDH_OK and lo.value == hi.value == 1.0
    d[1] = np.nan
    assert lib.pdh_tridiagonal_eigenvalues(3, d.ctypes.data, e.ctypes.data, C.byref(lo), C.byref(hi)) == _capi.PDH_EINVAL
    assert "not finite" in lib.pdh_last_error(None).decode()
    with pytest.raises(_capi.PdhError):
        _capi.tridiagonal_eigenvalues(np.ones(257), np.ones(256))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the reference alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _reference_conditions(A, n, kinds, what, iterations):
    N = A.shape[0]
    D = A.toarray()
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(N), rng.standard_normal(N)
    for kind in kinds:
        est, steps = cr.estimate(A, n, kind)
        assert 1 <= steps <= 20
        lo, hi = cr.bounds(est)
        # P^-1 A is similar to the symmetric L^-1 A L^-T, P = L L^T: its spectrum from a dense symmetric eigen-solve
        prec = preconditioner(A, n, kind)
        Pinv = np.stack([prec(e) for e in np.eye(N)], axis=1)
        L = np.linalg.cholesky(0.5 * (Pinv + Pinv.T))
        lam_max = np.linalg.eigvalsh(L.T @ D @ L)[-1]
        print(what, kind, "est %.6g, 1.2 est / lambda_max %.4f" % (est, hi / lam_max))
        assert hi >= lam_max, (what, kind, est, lam_max)
        for m in cc.DEGREES:
            Mu, Mv = cr.apply(A, n, kind, lo, hi, m, u), cr.apply(A, n, kind, lo, hi, m, v)
            assert abs(u @ Mv - v @ Mu) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(Mv), (what, kind, m)
            assert u @ Mu > 0 and v @ Mv > 0
        theta = (hi + lo) / 2
        z1, want = cr.apply(A, n, kind, lo, hi, 1, u), prec(u) / theta
        assert np.max(np.abs(z1 - want)) <= 4 * np.finfo(float).eps * np.max(np.abs(want)), (what, kind)
    if iterations:
        b = A @ u
        est, _ = cr.estimate(A, n, "block_jacobi")
        lo, hi = cr.bounds(est)
        x, it_c, res = pcg(A, b, cr.chebyshev_preconditioner(A, n, "block_jacobi", lo, hi, 3))
        _, it_b, _ = pcg(A, b, preconditioner(A, n, "block_jacobi"))
        print(what, "iterations: Chebyshev(3) over block Jacobi %d, block Jacobi %d" % (it_c, it_b))
        assert np.linalg.norm(x - u) <= 1e-9 * np.linalg.norm(u) and res <= 1e-13 * np.linalg.norm(b)
        assert it_c < it_b, (what, it_c, it_b)


@pytest.mark.parametrize("dim,lg,b,fe", [(2, 3, 2, po.FE_DGQ(2, 1)), (2, 3, 2, po.FE_AggloDGP(2, 2)), (3, 2, 2, po.FE_DGQ(3, 1)),
                                         (3, 2, 2, po.FE_AggloDGP(3, 2))], ids=lambda v: getattr(v, "name", str(v)))
@pytest.mark.parametrize("diag_first", [True, False])
def test_reference_on_the_solver_tests_oracle_systems(dim, lg, b, fe, diag_first):
    """On the oracle matrices of tests/test_solve_cpu.py, both inner kinds, 20 CG steps: 1.2 est bounds the spectrum of P^-1 A (the
    polynomial is then positive on it), the applied operator is symmetric and positive, degree 1 is (1 / theta) P^-1, and CG with
    Chebyshev (block Jacobi, degree 3) takes strictly fewer iterations than CG with block Jacobi."""
    A, n = _oracle_system(dim, lg, b, fe, diag_first)
    _reference_conditions(A, n, ("jacobi", "block_jacobi"), (fe.name, diag_first), True)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
@pytest.mark.parametrize("diag_first", [True, False])
def test_reference_on_the_cases_of_the_gpu_test(case, diag_first):
    """The same conditions on every case the device is compared on (tests/cheb_cases.py).  The iteration count is compared where
    there is more than one polytope: with one, block Jacobi is the exact inverse and CG takes a single step."""
    A, n = cc.oracle_system(case, diag_first)
    _reference_conditions(A, n, case[6], (cc.case_id(case), diag_first), "block_jacobi" in case[6] and A.shape[0] > n)


def test_tolerances_come_from_the_recorded_spreads():
    assert cc.Z_TOL == 100 * cc.Z_SPREAD >= 1e-13 and cc.EST_TOL == 100 * cc.EST_SPREAD >= 1e-13
    # the recorded spreads on one case (the full measurement is `python tests/cheb_cases.py`)
    case = cc.CASES[0]
    A, n = cc.oracle_system(case, True)
    b, x0 = cc.vectors(A.shape[0])
    LD = np.longdouble
    for kind in case[6]:
        e64, eld = cr.estimate(A, n, kind)[0], cr.estimate(A, n, kind, dtype=LD)[0]
        assert abs(LD(e64) - eld) / eld <= cc.EST_SPREAD
        lo, hi = cr.bounds(e64)
        z64, zld = cr.apply(A, n, kind, lo, hi, 5, b, x0), cr.apply(A, n, kind, lo, hi, 5, b, x0, dtype=LD)
        assert np.max(np.abs(z64 - zld)) / np.max(np.abs(zld)) <= cc.Z_SPREAD


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) header and exports
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_what_python_uses():
    from polydeal_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "polydeal_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(PDH_\w+)\s+(-?\d+)", hdr)}
    assert defs["PDH_PREC_CHEBYSHEV"] == _capi.PDH_PREC_CHEBYSHEV == 3
    assert len({defs[k] for k in ("PDH_PREC_NONE", "PDH_PREC_JACOBI", "PDH_PREC_BLOCK_JACOBI", "PDH_PREC_CHEBYSHEV")}) == 4
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    ctype = {"int32_t": "c_int", "double": "c_double"}
    for name, struct in (("pdh_chebyshev_control", _capi.pdh_chebyshev_control), ("pdh_chebyshev_info", _capi.pdh_chebyshev_info)):
        text = re.search(r"typedef struct %s\s*\{(.*?)\}" % name, body, re.S).group(1)
        fields = []
        for t, names in re.findall(r"(\w+)\s+([\w\s,]+);", text):
            fields += [(nm.strip(), ctype[t]) for nm in names.split(",")]
        assert [(f[0], f[1].__name__.replace("c_int32", "c_int")) for f in struct._fields_] == fields, name


def test_library_exports_the_chebyshev_entry_points():
    _capi = _capi_or_skip()
    lib = _capi.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polydeal_hip.h")).read(), flags=re.S)
    for sym in ("pdh_setup_chebyshev", "pdh_chebyshev_step_device", "pdh_tridiagonal_eigenvalues"):
        assert sym in _capi.EXPORTS and hasattr(lib, sym), sym
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
