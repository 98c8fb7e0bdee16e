"""p-multigrid on the device: levels.p_multigrid_hierarchy on hierarchies A - G of tests/ptransfer_cases.py (p-pairs of FE_DGQ and
FE_AggloDGP, mixed p/h hierarchies, an element beyond 64 dofs, both kinds of coarsest level) against the NumPy restatement
(tests/pmg_ref.py) on the matrices read back from the device with the device's own smoother bounds: three V-cycles, the CG iteration
counts, the float32 and matrix-free smoothers per level, and the state rule; examples/poisson --device-solve --p-multigrid on the
reference's own mesh (364 grown FE_AggloDGP agglomerates, a coarsest level of 1092 rows smoothed by Chebyshev)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import pcg_ref
import pmg_ref
import ptransfer_cases as pc
from test_gpu_solve import _Device, _global_matrix

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _pa():
    import polydeal_amd as pa
    return pa


def _variant(fe):
    return _pa().SipVariant.poisson_example(fe)


def _hierarchy(name, coarsest=None, **kw):
    """(MultigridHierarchy, pmg_ref.Hierarchy on the matrices read back with the device's smoother bounds, mirror handlers)"""
    from polydeal_amd.levels import p_multigrid_hierarchy

    mirror, _ = pc.handlers(name)
    hier = p_multigrid_hierarchy(mirror, _variant, diag_first=False, degree=pc.DEGREE, coarsest=coarsest, **kw)
    try:
        mats = [_global_matrix(ctx, ah.flatten(_variant(ah.fe), False, True).arrays(), ah.n_dofs) for ctx, ah in zip(hier.contexts, mirror)]
        ns = pc.level_ns(name)
        assert [ah.fe.n_dofs_per_cell for ah in mirror] == ns
        bounds = [(i.get("lambda_lo"), i.get("lambda_hi")) for i in hier.info]
        coarse = "direct" if "pivot_min" in hier.info[0] else "chebyshev"
        H = pmg_ref.Hierarchy(mats, ns, pc.injections(name), bounds, pc.DEGREE, [pc.inner_kind(n) for n in ns], coarse)
    except Exception:
        hier.close()
        raise
    return hier, H, mirror


def _rel(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


def _three_cycles(name, hier, H, dev, b):
    N = len(b)
    tol = pc.CYCLE_TOL + 10.0 * float(np.linalg.cond(H.mats[0].toarray())) * EPS
    d_b, d_x = dev.put(b), dev.put(np.full(N, np.nan))
    x_ref = None
    for cyc in range(3):
        hier.vcycle_device(d_b, d_x, zero_initial_guess=(cyc == 0))
        hier.finest.synchronize()
        x = dev.get(d_x, N)
        x_ref = pmg_ref.cycle(H, b, x_ref)
        print("%s: cycle %d: %.3e (bound %.3e)" % (name, cyc + 1, _rel(x, x_ref), tol))
        assert _rel(x, x_ref) <= tol, (cyc, _rel(x, x_ref), tol)


CASES = [(name, None) for name in pc.HIERARCHIES] + [("F", "chebyshev")]


@pytest.mark.parametrize("name,coarsest", CASES, ids=["%s_%s" % (n, c or "auto") for n, c in CASES])
def test_p_vcycle_and_cg_against_the_numpy_restatement(name, coarsest):
    hier, H, mirror = _hierarchy(name, coarsest)
    dev = _Device()
    try:
        assert H.coarse == (coarsest or "direct")  # (every coarsest level here has at most 1024 rows)
        assert [i["smoother_operator"] for i in hier.info] == ["stored"] * len(mirror)
        A = H.mats[-1]
        N = A.shape[0]
        b = pc.rhs(N)
        _three_cycles(name, hier, H, dev, b)
        x, cg = hier.solve_cg(b)
        x_sp = spla.spsolve(A.tocsc(), b)
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        it_ref = pcg_ref.pcg(A, b, pmg_ref.preconditioner(H), rel_tol=1e-13)[1]
        recorded = pc.F_CHEBYSHEV_COUNT if coarsest == "chebyshev" else pc.PCG_COUNTS[name][0]
        print("%s: CG iterations %d (restatement on the device's matrices %d, recorded on the CPU %d)" % (name, cg["iterations"], it_ref, recorded))
        assert abs(cg["iterations"] - it_ref) <= 1 and abs(cg["iterations"] - recorded) <= 1
        x2, cg2 = hier.solve_cg(b)
        assert np.array_equal(x2, x) and cg2 == cg
    finally:
        hier.close()
        dev.free()


def test_smoother_precision_and_operator_per_level():
    """B with float32 smoothers: the bounds of test_gpu_smoother_f32.py::test_multigrid_hierarchy_with_f32_smoothers, the test of
    multigrid_hierarchy(smoother_precision="f32") (iterations within one of the double run, the solution within 1e-9 of spsolve).  B with matrix-free smoothers: info says where the tables were granted; the cycle and the counts as stored."""
    name = "B"
    b = pc.rhs(pc.ROWS[name][-1])
    hier, H, mirror = _hierarchy(name, smoother_precision="f32")
    try:
        assert [c.smoother_precision for c in hier.contexts] == ["f64", "f32", "f32"]
        x, cg = hier.solve_cg(b)
        x_sp = spla.spsolve(H.mats[-1].tocsc(), b)
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        print("B, f32 smoothers: %d iterations" % cg["iterations"])
        assert abs(cg["iterations"] - pc.PCG_COUNTS[name][0]) <= 1
    finally:
        hier.close()
    hier, H, mirror = _hierarchy(name, smoother_operator="matrix_free")
    dev = _Device()
    try:
        granted = [i["smoother_operator"] for i in hier.info]
        print("B, matrix-free smoothers granted:", granted)
        assert granted == [c.smoother_operator for c in hier.contexts] and granted[0] == "stored"
        assert granted[1:] == ["matrix_free"] * 2  # (polytopes of one Cartesian cell in 3-D: the term tables exist on both levels)
        _three_cycles(name + " matrix_free", hier, H, dev, b)
        _, cg = hier.solve_cg(b)
        assert abs(cg["iterations"] - pc.PCG_COUNTS[name][0]) <= 1
    finally:
        hier.close()
        dev.free()


def test_reassembling_a_level_makes_the_solve_stale():
    pa = _pa()
    from polydeal_amd import _capi

    hier, H, mirror = _hierarchy("G")
    try:
        b = pc.rhs(pc.ROWS["G"][-1])
        hier.solve_cg(b)
        hier.contexts[1].assemble_device()
        with pytest.raises(pa.PdhError) as ei:
            hier.solve_cg(b)
        assert ei.value.code == _capi.PDH_ESTATE and "level 1 of 3" in str(ei.value), str(ei.value)
    finally:
        hier.close()


def _example(*flags):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "poisson")
    assert os.path.exists(exe), "examples/poisson is built by __graft_entry__.build()"
    out = subprocess.run([exe, "--device-solve"] + list(flags) + [os.path.join(root, "tests", "golden", "t3.msh")], capture_output=True,
                         text=True, timeout=600, cwd=os.path.join(root, "examples"))
    assert out.returncode == 0, out.stdout + out.stderr  # (2: the p-convergence check failed)
    errors = [l for l in out.stdout.splitlines() if l.startswith(("Error (", "L2 error:"))]
    its = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"\((\d+) dofs, (\d+) CG iterations", out.stderr)]
    return errors, its, out.stderr


def test_poisson_example_with_the_p_vcycle():
    """examples/poisson --device-solve --p-multigrid on tests/golden/t3.msh: FE_AggloDGP(1 .. 4) on 364 grown agglomerates, degrees 2 .. 4
    solved with the V-cycle over the degrees 1 .. p (coarsest level 1092 rows: one Chebyshev application).  Exit status 0 (the
    p-convergence check passes), every error line equal to the --device-solve run's to the printed digits, and fewer iterations than
    block-Jacobi CG for every degree >= 2."""
    errors_bj, its_bj, _ = _example()
    errors_mg, its_mg, stderr = _example("--p-multigrid")
    print("block Jacobi:", its_bj, "p-V-cycle:", its_mg)
    assert len(errors_bj) == 9 and errors_mg == errors_bj, (errors_bj, errors_mg)  # the reference case's line + 4 x (L2, H1)
    assert [n for n, _ in its_mg] == [n for n, _ in its_bj] == [364 * k for k in (3, 6, 10, 15)]
    assert its_mg[0] == its_bj[0] and stderr.count("V-cycle over the degrees") == 3  # degree 1 keeps block Jacobi
    for (n, mg), (_, bj) in zip(its_mg[1:], its_bj[1:]):
        assert mg < bj, (n, mg, bj)
