"""The matrix-free SIP operator on the device (csrc/pdh_matfree.h: k_mf_tables, k_mf_vmult; C ABI: pdh_setup_matrix_free,
pdh_matrix_free_vmult*, pdh_set_smoother_operator, pdh_smoother_operator) against the ORACLE's matrix of the same description, and the
Chebyshev chain and the V-cycle that take their products from it against their NumPy restatements.

Tolerance of a product (tests/matfree_cases.py, measured on the CPU, not on the device): the restatement of the term form in float64
against itself in numpy.longdouble differs by at most 8.761e-16 sum_j |A_ij| |x_j| in a row; the device may differ from the long-double
product of the oracle's matrix by 100 x that, never less than 1e-13: PRODUCT_TOL = 1e-13.  The Chebyshev and V-cycle bounds are those
of their own tests (cheb_cases.Z_TOL, vcycle_cases.CYCLE_TOL, mixed_cases.MIXED_CYCLE_TOL): the operator is the same up to rounding."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cheb_cases as cc
import cheb_ref as cr
import matfree_cases as mc
import mixed_cases as mxc
import mixed_ref as mxr
import parity
import pcg_ref
import vcycle_cases as vc
import vcycle_ref as vr
from flatten_oracle import flatten
from test_gpu_solve import _Device, _global_matrix, _handler
from test_gpu_vcycle import _permuted_problem, _rel, _variant

pytestmark = pytest.mark.gpu

LAYOUTS = [True, False]
LAYOUT_IDS = ["dealii", "ascending"]


def _pa():
    import polydeal_amd as pa
    return pa


def _context(problem, *rows):
    """a context with the problem resident, the term kernels' plan asserted before the device computes anything"""
    ctx = _pa().Context(0)
    try:
        ctx.set_problem(problem, *rows)
        assert ctx.rows_kernel_in_use() == "terms"
    except Exception:
        ctx.close()
        raise
    return ctx


def _case_context(cid, diag_first):
    pa = _pa()
    ah, var = mc.oracle_handler(cid)
    mc.check_property(cid, ah)
    return _context(pa.Problem(**flatten(ah, var, diag_first, True)))


_LD = {}


def _reference(key, A, x):
    """(long-double product of the oracle's rows A with x, sum_j |A_ij| |x_j|), computed once per (key, vector)"""
    k = (key, x.tobytes()[:64])
    if k not in _LD:
        D = A.toarray()
        _LD[k] = (D.astype(np.longdouble) @ x.astype(np.longdouble), np.abs(D) @ np.abs(x))
    return _LD[k]


def _product_error(y, key, A, x):
    """worst row of |y - A x| / sum_j |A_ij| |x_j| against the long-double product of the oracle's rows"""
    ref, scale = _reference(key, A, x)
    assert np.all(np.isfinite(y))
    return float(np.max(np.abs(y.astype(np.longdouble) - ref) / scale))


def _check_product(y, key, A, x, what):
    err = _product_error(y, key, A, x)
    print("%s: worst row %.3e sum|a x| (bound %.1e)" % (what, err, mc.PRODUCT_TOL))
    assert err <= mc.PRODUCT_TOL, (what, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole operator
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mc.WHOLE_OPERATOR_IDS)
def test_the_operator_read_column_by_column_is_the_oracles_matrix(cid):
    """the product with every unit vector: the matrix so read equals the oracle's to 1e-12 per block (tests/parity.py) and is exactly
    zero outside the pattern; nothing was assembled"""
    ctx = _case_context(cid, False)
    try:
        info = ctx.setup_matrix_free()
        ah, _ = mc.oracle_handler(cid)
        A = mc.oracle_matrix(cid)
        N, n = ah.n_dofs, ah.fe.n_dofs_per_cell
        assert N <= 512 and info["table_bytes"] == 8 * info["doubles_per_polytope"] * ah.n_agglomerates and info["max_cells"] >= 1
        M = np.zeros((N, N))
        e = np.zeros(N)
        for j in range(N):
            e[j] = 1.0
            M[:, j] = ctx.matrix_free_vmult(e)
            e[j] = 0.0
        rows = np.repeat(np.arange(N), np.diff(A.indptr))
        worst = parity.assert_parity(M[rows, A.indices], A.data, A.indptr, A.indices, n, what=cid)
        outside = np.ones((N, N), dtype=bool)
        outside[rows, A.indices] = False
        assert not np.any(M[outside])
        print(cid, "operator read back against the oracle: %.2e max|A|" % worst, info)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(mc.CASES))
@pytest.mark.parametrize("diag_first", LAYOUTS, ids=LAYOUT_IDS)
def test_products_against_the_oracle_in_long_double(cid, diag_first):
    """both vectors of cheb_cases.vectors: every row within PRODUCT_TOL sum_j |A_ij| |x_j| of the long-double product of the oracle's
    matrix; host-pointer and device-pointer forms, two calls, before and after the assembly: the same bits.

    Measured on an MI355X: 3.6e-16 .. 5.2e-14, and 8.8e-14 on offset_mod_dgq3, the mesh at |x| / h = 56.  There the STORED product of the
    same context (printed, not asserted) is 4.1e-13 from the oracle's: the assembly takes the plane coordinate of a sub-face from one
    face point of the description, whose two ulps of rounding at |x| ~ 13 (7e-15 of the box) put sigma B'_k 7e-15 into penalty entries
    that vanish exactly where the plane is a box face.  k_mf_tables takes such a plane from the box instead (csrc/pdh_matfree.h); what
    is left is the oracle's own rounding on that mesh (tests/matfree_ref.py with the exact planes is 8.5e-14 from its product)."""
    ctx = _case_context(cid, diag_first)
    dev = _Device()
    try:
        A = mc.oracle_matrix(cid)
        N = A.shape[0]
        ctx.setup_matrix_free()
        ys, errs = [], []
        for x in cc.vectors(N):
            y = ctx.matrix_free_vmult(x)
            errs.append(_product_error(y, cid, A, x))
            d_x, d_y = dev.put(x), dev.put(np.full(N, np.nan))
            for _ in range(2):
                ctx.matrix_free_vmult_device(d_x, d_y)
                ctx.synchronize()
                assert np.array_equal(dev.get(d_y, N), y)
            ys.append(y)
        ctx.assemble()
        for x, y in zip(cc.vectors(N), ys):
            assert np.array_equal(ctx.matrix_free_vmult(x), y)
        # (figures only: the stored product of the same context against the same reference)
        stored = [_product_error(ctx.vmult(x), cid, A, x) for x in cc.vectors(N)]
        print("%s diag_first=%d: worst row of the matrix-free product %.3e, %.3e sum|a x| (bound %.1e); of the stored product %.3e, %.3e" %
              ((cid, diag_first) + tuple(errs) + (mc.PRODUCT_TOL,) + tuple(stored)))
        assert max(errs) <= mc.PRODUCT_TOL, (cid, errs)
    finally:
        ctx.close()
        dev.free()


def _mirror_6():
    pa = _pa()
    ah, fe = _handler(3, 6, 2, "dgq", 3)
    return ah, fe, pa.SipVariant.poisson_example(fe)


def test_generated_points_permuted_numbering_row_ranges_and_rank_local_descriptions():
    """the 6^3 mesh of c6_b2_dgq3 from the product's host mirror: through pdh_set_problem_cartesian (generated points); with the
    polytopes' dof ranges shuffled (dof_offset); a row range of the global description; rank-local descriptions in both layouts and in
    Epetra column order (col_offset) - global x, ghost columns read from it, owned rows out"""
    from polydeal_amd.partition import row_range

    ah, fe, var = _mirror_6()
    A = mc.oracle_matrix("c6_b2_dgq3")
    N, n, nA = ah.n_dofs, fe.n_dofs_per_cell, ah.n_agglomerates
    x = cc.vectors(N)[0]
    cf = ah.flatten_cartesian(var, True, True)
    assert cf.cartesian
    ctx = _context(cf)
    try:
        ctx.setup_matrix_free()
        y_all = ctx.matrix_free_vmult(x)
        _check_product(y_all, "c6", A, x, "cartesian description")
        # shuffled dof ranges (ascending layout)
        prob, m = _permuted_problem(ah, fe)
        ctx.set_problem(prob)
        assert ctx.rows_kernel_in_use() == "terms"
        with pytest.raises(_pa().PdhError) as e:  # the tables went with the problem
            ctx.matrix_free_vmult(x)
        assert e.value.code == _pa()._capi.PDH_ESTATE
        ctx.setup_matrix_free()
        xp = np.zeros(N)
        xp[m] = x
        _check_product(ctx.matrix_free_vmult(xp)[m], "c6", A, x, "permuted dof_offset")
        # a row range, rank-local descriptions
        world = 3
        splits = [row_range(nA, n, r, world)[0] for r in range(world)] + [N]
        gflat = ah.flatten(var, True, True)
        for r in (1,):
            r0, r1 = splits[r], splits[r + 1]
            ctx.set_problem(gflat, r0, r1)
            assert ctx.rows_kernel_in_use() == "terms"
            ctx.setup_matrix_free()
            y = ctx.matrix_free_vmult(x)
            assert y.shape == (r1 - r0,)
            _check_product(y, ("c6", r0, r1), A[r0:r1], x, "row range %d:%d" % (r0, r1))
            for diag_first, epetra in ((True, False), (False, False), (False, True)):
                loc = ah.flatten_local(var, r0, r1, diag_first, True, row_splits=splits, epetra_columns=epetra)
                assert loc.c.local == 1 and (loc.arrays().get("col_offset") is not None) == epetra
                ctx.set_problem(loc, r0, r1)
                assert ctx.rows_kernel_in_use() == "terms"
                ctx.setup_matrix_free()
                _check_product(ctx.matrix_free_vmult(x), ("c6", r0, r1), A[r0:r1], x,
                               "rank-local diag_first=%d epetra=%d" % (diag_first, epetra))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Chebyshev with the matrix-free operator
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mc.CHEB_IDS)
def test_chebyshev_applications_with_the_matrix_free_operator(cid):
    """degrees 1, 2, 5 over both inner kinds, zero and non-zero start, against cheb_ref on the matrix read back with the device's
    lambda_lo / lambda_hi, within cheb_cases.Z_TOL |z|_inf; the same bits twice; not the bits of the stored operator"""
    ctx = _case_context(cid, True)
    dev = _Device()
    try:
        ah, var = mc.oracle_handler(cid)
        N, n = ah.n_dofs, ah.fe.n_dofs_per_cell
        ctx.setup_matrix_free()
        ctx.assemble()
        A = _global_matrix(ctx, flatten(ah, var, True, True), N)
        b, x0 = cc.vectors(N)
        d_b, d_z = dev.put(b), dev.put(np.full(N, np.nan))
        differs = False
        for kind in ("jacobi", "block_jacobi"):
            for m in cc.DEGREES:
                info = ctx.setup_chebyshev(kind, degree=m)
                assert ctx.smoother_operator == "stored"
                ctx.precondition_device(d_b, d_z)
                ctx.synchronize()
                z_stored = dev.get(d_z, N)
                ctx.set_smoother_operator("matrix_free")
                assert ctx.smoother_operator == "matrix_free"
                lo, hi = info["lambda_lo"], info["lambda_hi"]
                zs = []
                for _ in range(2):
                    ctx.precondition_device(d_b, d_z)
                    ctx.synchronize()
                    zs.append(dev.get(d_z, N))
                assert np.array_equal(zs[0], zs[1])
                dz = _rel(zs[0], cr.apply(A, n, kind, lo, hi, m, b))
                d_x = dev.put(x0)
                ctx.chebyshev_step_device(d_b, d_x)
                ctx.synchronize()
                dx = _rel(dev.get(d_x, N), cr.apply(A, n, kind, lo, hi, m, b, x0))
                print("%s %-12s degree %d: zero start %.2e, non-zero start %.2e (bound %.3e)" % (cid, kind, m, dz, dx, cc.Z_TOL))
                assert dz <= cc.Z_TOL and dx <= cc.Z_TOL, (kind, m, dz, dx)
                differs = differs or (m > 1 and not np.array_equal(zs[0], z_stored))
        assert differs  # (degree 1 from zero takes no product; the others do, in another order of summation)
    finally:
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# V-cycle
# ---------------------------------------------------------------------------------------------------------------------------------
class _ExactProductHierarchy(mxr.Hierarchy):
    """mixed_ref.Hierarchy whose F32 levels round the block inverses only: the product is the unrounded matrix's, as with
    PDH_SMOOTHER_OP_MATRIX_FREE under PDH_SMOOTHER_F32"""

    def smoother(self, l, dtype):
        if (l, dtype) not in self._sm:
            S = mxr.Smoother(self.mats[l], self.n, self.kind, dtype, self.inv64[l])
            S.mv = cr.operator(self.mats[l], dtype)
            self._sm[(l, dtype)] = S
        return self._sm[(l, dtype)]


def _double_inverses(ah, fe, dev):
    """the double block inverses the device stores for a level as multigrid_hierarchy describes it, read back bit for bit from a
    context of its own (the kernels are deterministic)"""
    from test_gpu_solve_shapes import _stored_inverse

    ctx = _pa().Context(0)
    try:
        ctx.set_problem(ah.flatten_cartesian(_variant(fe), False, False))
        ctx.assemble_device()
        ctx.setup_preconditioner("block_jacobi")
        return _stored_inverse(ctx, dev, fe.n_dofs_per_cell, ah.n_dofs)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [vc.HIERARCHY_CASE, vc.CASES[4]], ids=vc.case_id)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_vcycle_and_cg_through_multigrid_hierarchy(case, precision):
    """levels.multigrid_hierarchy(smoother_operator='matrix_free'): every level above the coarsest is granted the operator; three
    consecutive cycles within the cycle bound + 10 cond_2(A_0) 2.2e-16 of the restatement on the matrices read back (vcycle_ref; with
    F32 block inverses on top mixed_ref with the exact product), CG iterations within one of pcg_ref's, the solution against spsolve"""
    pa = _pa()
    from polydeal_amd.levels import multigrid_hierarchy

    mirror, _ = vc.handlers(*case)
    fe = pa.FE_DGQ(case[0], case[3])
    n = fe.n_dofs_per_cell
    kind = vc.inner_kind(n)
    hier = multigrid_hierarchy(mirror, fe, _variant(fe), diag_first=False, degree=vc.DEGREE, smoother_precision=precision,
                               smoother_operator="matrix_free")
    dev = _Device()
    try:
        assert [i["smoother_operator"] for i in hier.info] == ["stored"] + ["matrix_free"] * (len(mirror) - 1)
        assert [c.smoother_operator for c in hier.contexts] == ["stored"] + ["matrix_free"] * (len(mirror) - 1)
        assert [c.smoother_precision for c in hier.contexts] == ["f64"] + [precision] * (len(mirror) - 1)
        assert all(c.rows_kernel_in_use() == "terms" for c in hier.contexts[1:])
        mats = [_global_matrix(c, ah.flatten(_variant(fe), False, True).arrays(), ah.n_dofs) for c, ah in zip(hier.contexts, mirror)]
        bounds = [(i.get("lambda_lo"), i.get("lambda_hi")) for i in hier.info]
        H = vr.Hierarchy(mats, n, vc.injections(case), bounds, vc.DEGREE, kind, "direct")
        tol = vc.CYCLE_TOL
        cycle, prec = vr.cycle, vr.preconditioner
        if precision == "f32":
            # the float block inverses of the device (its own doubles, rounded) under the EXACT product
            inv = [None] + [_double_inverses(ah, fe, dev) for ah in mirror[1:]]
            H = _ExactProductHierarchy(H, f32=[False] + [True] * (len(mirror) - 1), inv64=inv)
            tol = mxc.MIXED_CYCLE_TOL
            cycle, prec = mxr.cycle, mxr.preconditioner
        tol += 10.0 * float(np.linalg.cond(mats[0].toarray())) * 2.2e-16
        N, A = mirror[-1].n_dofs, mats[-1]
        b = vc.rhs(N)
        d_b, d_x = dev.put(b), dev.put(np.full(N, np.nan))
        x_ref = None
        for cyc in range(3):
            hier.vcycle_device(d_b, d_x, zero_initial_guess=(cyc == 0))
            hier.finest.synchronize()
            x = dev.get(d_x, N)
            x_ref = cycle(H, b, x_ref)
            print("%s %s: cycle %d: %.3e (bound %.3e)" % (vc.case_id(case), precision, cyc + 1, _rel(x, x_ref), tol))
            assert _rel(x, x_ref) <= tol, (cyc, _rel(x, x_ref), tol)
        x, cg = hier.solve_cg(b)
        x_sp = spla.spsolve(A.tocsc(), b)
        _, it_ref, _ = pcg_ref.pcg(A, b, prec(H), rel_tol=1e-13)
        print("%s %s: CG iterations %d (restatement %d)" % (vc.case_id(case), precision, cg["iterations"], it_ref))
        assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
        assert cg["iterations"] == it_ref
        x2, cg2 = hier.solve_cg(b)
        assert np.array_equal(x2, x) and cg2 == cg
    finally:
        hier.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# state rules and refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_rules_and_refusals():
    pa = _pa()
    E = pa._capi
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import level_transfer
    from oracle import polydeal_oracle as po
    import aniso_meshes as am

    def refused(call, code, *words):
        with pytest.raises(pa.PdhError) as e:
            call()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    dev = _Device()
    ctxs, ts, mg = [], [], None
    try:
        # ---- what the set-up refuses: PDH_EUNSUPPORTED naming the reason; the stored product still serves
        def unsupported(problem, word, env=None):
            ctx = pa.Context(0)
            ctxs.append(ctx)
            ctx.set_problem(problem)
            ctx.assemble()
            x = cc.vectors(ctx.n_rows)[0]
            y = ctx.vmult(x)
            refused(ctx.setup_matrix_free, E.PDH_EUNSUPPORTED, word)
            refused(lambda: ctx.matrix_free_vmult(x), E.PDH_ESTATE, "pdh_setup_matrix_free")
            ctx.setup_chebyshev("jacobi", degree=2)
            refused(lambda: ctx.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "pdh_setup_matrix_free")
            assert ctx.smoother_operator == "stored" and np.array_equal(ctx.vmult(x), y)

        ah2, fe2 = _handler(2, 8, 2, "dgq", 2)
        unsupported(ah2.flatten(pa.SipVariant.poisson_example(fe2), True, True), "not 3-D")
        ah4, fe4 = _handler(3, 2, 1, "dgq", 4)
        unsupported(ah4.flatten(pa.SipVariant.poisson_example(fe4), True, True), "degree is above 3")
        grid = po.hyper_cube_refined(3, 0.0, 1.0, 2)
        grid.distort(0.15, seed=3)
        ad = po.AgglomerationHandler(grid)
        for g in po.block_agglomerates(grid, 2):
            ad.define_agglomerate(g)
        fed = po.FE_DGQ(3, 2)
        ad.initialize_fe_values(3, 3)
        ad.distribute_agglomerated_dofs(fed)
        unsupported(pa.Problem(**flatten(ad, po.variant_poisson_example(fed), True, True)), "matrix-free operator needs")

        # ---- a three-level hierarchy of the 3-D case: contexts, Chebyshev on 1 and 2, the direct solve on 0
        case = vc.CASES[2]
        mirror, _ = vc.handlers(*case)
        fe = pa.FE_DGQ(case[0], case[3])
        for l, ah in enumerate(mirror):
            ctx = pa.Context(0)
            ctxs.append(ctx)
            ctx.set_problem(ah.flatten(_variant(fe), False, True))
            if l:
                ts.append(level_transfer(ctx, mirror[l - 1], ah))
        c0, c1, c2 = ctxs[-3:]
        N = mirror[-1].n_dofs
        b, x0 = cc.vectors(N)
        d_b, d_z = dev.put(b), dev.put(np.full(N, np.nan))
        assert c2.rows_kernel_in_use() == "terms"
        # before the tables; the argument checks of the product
        refused(lambda: c2.matrix_free_vmult(b), E.PDH_ESTATE, "pdh_setup_matrix_free")
        c2.setup_matrix_free()
        assert c2.setup_matrix_free() == c2.setup_matrix_free()  # (a second call only reports)
        assert c2.lib.pdh_matrix_free_vmult_device(c2.h, C.c_void_p(d_b), C.c_void_p(d_b)) == E.PDH_EINVAL
        assert c2.lib.pdh_matrix_free_vmult_device(c2.h, C.c_void_p(d_b), None) == E.PDH_EINVAL
        assert c2.lib.pdh_matrix_free_vmult(c2.h, b.ctypes.data, b.ctypes.data) == E.PDH_EINVAL
        assert "overlap" in c2.lib.pdh_last_error(c2.h).decode()
        # never assembled; not Chebyshev; a bad value
        refused(lambda: c2.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "PDH_PREC_CHEBYSHEV")
        c2.assemble_device()
        c2.setup_preconditioner("block_jacobi")
        refused(lambda: c2.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "PDH_PREC_CHEBYSHEV")
        c2.setup_chebyshev("block_jacobi", degree=3)
        assert c2.lib.pdh_set_smoother_operator(c2.h, 2) == E.PDH_EINVAL and c2.lib.pdh_set_smoother_operator(c2.h, -1) == E.PDH_EINVAL
        assert c2.smoother_operator == "stored"

        def z_of(ctx, d_in=d_b, count=N):
            ctx.precondition_device(d_in, d_z)
            ctx.synchronize()
            return dev.get(d_z, count)

        z_st = z_of(c2)
        c2.set_smoother_operator("stored")  # (stored on a stored context is fine)
        c2.set_smoother_operator("matrix_free")
        z_mf = z_of(c2)
        assert c2.smoother_operator == "matrix_free" and not np.array_equal(z_mf, z_st) and _rel(z_mf, z_st) <= cc.Z_TOL
        c2.set_smoother_operator("stored")
        assert np.array_equal(z_of(c2), z_st)
        # orthogonal to the precision: F32 inverses under the matrix-free product are neither of the two, and pdh_smoother_vmult_device
        # stays the shadow's product
        c2.set_smoother_precision("f32")
        z_32 = z_of(c2)
        c2.set_smoother_operator("matrix_free")
        z_mf32 = z_of(c2)
        assert c2.smoother_precision == "f32" and not np.array_equal(z_mf32, z_32) and not np.array_equal(z_mf32, z_mf)
        # every set-up call goes back to the stored operator
        for setup in (lambda: c2.setup_preconditioner("jacobi"), lambda: c2.setup_chebyshev("block_jacobi", degree=3), c2.setup_direct):
            c2.setup_chebyshev("block_jacobi", degree=3)
            c2.set_smoother_operator("matrix_free")
            setup()
            assert c2.smoother_operator == "stored"
        # the values changed: stale until Chebyshev is set up again; the tables stay
        c2.setup_chebyshev("block_jacobi", degree=3)
        c2.set_smoother_operator("matrix_free")
        c2.assemble_device()
        refused(lambda: c2.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "values changed")
        refused(lambda: c2.precondition_device(d_b, d_z), E.PDH_ESTATE, "values changed")
        c2.setup_chebyshev("block_jacobi", degree=3)
        c2.set_smoother_operator("matrix_free")
        assert np.array_equal(z_of(c2), z_mf)
        # ---- Galerkin-written coarse contexts: the tables are not their operator
        c1.setup_matrix_free()
        ts[1].galerkin_device(c1)
        ts[0].galerkin_device(c0)
        c1.setup_chebyshev("block_jacobi", degree=3)
        refused(lambda: c1.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "pdh_galerkin_device")
        assert c1.smoother_operator == "stored"
        c1.assemble_device()
        c1.setup_chebyshev("block_jacobi", degree=3)
        c1.set_smoother_operator("matrix_free")
        ts[1].galerkin_device(c1)  # a later Galerkin product puts the context back
        assert c1.smoother_operator == "stored"
        c1.setup_chebyshev("block_jacobi", degree=3)
        refused(lambda: c1.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "pdh_galerkin_device")
        # ---- a multigrid attached: the operator is chosen before pdh_mg_create; a level's change makes the mg stale
        c1.assemble_device()
        c1.setup_chebyshev("block_jacobi", degree=3)
        c0.assemble_device()
        c0.setup_direct()
        refused(lambda: c0.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "PDH_PREC_CHEBYSHEV")
        mg = Multigrid([c0, c1, c2], ts)
        refused(lambda: c2.set_smoother_operator("stored"), E.PDH_ESTATE, "pdh_mg_create")
        refused(lambda: c2.set_smoother_operator("matrix_free"), E.PDH_ESTATE, "pdh_mg_create")
        mg.vcycle_device(d_b, d_z, True)
        c2.synchronize()
        c1.set_smoother_operator("matrix_free")
        refused(lambda: mg.vcycle_device(d_b, d_z, True), E.PDH_ESTATE, "level 1 of 3")
        refused(lambda: c2.solve_cg(b), E.PDH_ESTATE, "level 1 of 3")
    finally:
        if mg is not None:
            mg.close()
        for t in ts:
            t.close()
        for c in ctxs:
            c.close()
        dev.free()
