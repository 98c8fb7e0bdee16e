"""Single-precision smoother matrices on the device (csrc/pdh_shadow.hip; C ABI: pdh_set_smoother_precision, pdh_smoother_precision,
pdh_smoother_vmult_device): the float32 shadow entry by entry, the product with it on long rows and large elements, the Chebyshev
applications and the V-cycle against their NumPy restatement (tests/mixed_ref.py) on the matrices read back, CG with the mixed cycle,
levels.multigrid_hierarchy(smoother_precision="f32"), the state rules, the example's flag and the headline hierarchy.

Shapes and bounds: tests/mixed_cases.py (100 x the float64-against-long-double spread of the restatement, never below 1e-13; tests/
test_mixed_cpu.py shows on the CPU that the mixed and the double results lie 1000 bounds apart, so a device that ignored the switch
fails here).  The restatement rounds the double block inverses THE DEVICE stores (read back bit for bit as in test_gpu_solve_shapes.py):
a float ulp is 6e-8 of an entry, so a double inverse that differed from NumPy's in its last bits would now and then round the other way.

Mutations these tests were seen to catch on the device (each built, run against this file, and taken out again; the first test that
failed):
  the conversion without the diagonal-first un-shift                      -> shadow entries, dealii, dgq1_2d
  a row stride without the pad on odd rows                                -> shadow entries, dealii, dgq2_2d
  the surplus lanes of the tail piece not discarded (address clamp kept)  -> shadow entries, dealii, dgq1_2d
  float products and lane sums instead of double                          -> shadow product, dealii, dgq4_3x3x3 (the entries pass: exact)
  the block inverse read in double after the switch                       -> Chebyshev applications, dealii, dgq1_2d"""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import golden_cases as gc
import mixed_cases as mc
import mixed_ref as mr
import pcg_ref
import vcycle_cases as vc
from test_gpu_solve import _Device, _global_matrix, _kernels
from test_gpu_solve_shapes import _Resident, _stored_inverse
from test_gpu_vcycle import _Levels, _rel, _variant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT_IDS = ["dealii", "ascending"]


def _pa():
    import polydeal_amd as pa
    return pa


class _Shape:
    """a shape of mixed_cases.CHEB_SHAPES assembled on the device, its property asserted first: context, matrix of the values in HBM"""

    def __init__(self, sid, diag_first):
        pa = _pa()
        self.ah, self.fe, self.flat = mc.mirror_flat(sid, diag_first)
        self.arr = self.flat.arrays()
        self.n, self.N = self.fe.n_dofs_per_cell, self.ah.n_dofs
        mc.check_shape_property(sid, self.n, self.ah.n_agglomerates, self.arr["rowptr"])
        self.ctx, self.dev = pa.Context(0), _Device()
        try:
            self.ctx.set_problem(self.flat)
            _kernels(self.ctx)
            self.ctx.assemble()
            self.A = _global_matrix(self.ctx, self.arr, self.N)
        except Exception:
            self.close()
            raise

    def close(self):
        self.ctx.close()
        self.dev.free()


def _f32(ctx, kind, degree, estimate=None):
    """Chebyshev set up over `kind`, then the shadow; returns (info, the double block inverses the device stores or None)"""
    inv64 = None
    if kind == "block_jacobi":
        st = ctx.stats()
        ctx.setup_preconditioner("block_jacobi")
        dev = _Device()
        try:
            inv64 = _stored_inverse(ctx, dev, st["dofs_per_cell"], ctx.n_rows)
        finally:
            dev.free()
    info = ctx.setup_chebyshev(kind, degree=degree, max_eigenvalue=estimate or 0.0)
    assert ctx.smoother_precision == "f64"
    ctx.set_smoother_precision("f32")
    assert ctx.smoother_precision == "f32"
    return info, inv64


# ---------------------------------------------------------------------------------------------------------------------------------
# the shadow, entry by entry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", list(mc.ENTRY_SHAPES))
@pytest.mark.parametrize("diag_first", mc.LAYOUTS, ids=LAYOUT_IDS)
def test_shadow_entries_are_the_rounded_entries_bit_for_bit(sid, diag_first):
    """pdh_smoother_vmult_device on every unit vector: one product per row is a~_ij * 1 and every other term an exact zero, so column j
    comes back as float32(A_ij) exactly - the conversion (the diagonal-first shift undone, the pad), the row bases and strides, and the
    piece walk of the product kernel, with nothing to hide behind."""
    R = _Shape(sid, diag_first)
    try:
        _f32(R.ctx, "block_jacobi", 1, 1.0)
        At = mr.rounded_matrix(R.A).tocsc()
        N, chunk = R.N, 256
        for c0 in range(0, N, chunk):
            cols = np.arange(c0, min(c0 + chunk, N))
            E = np.zeros((len(cols), N))
            E[np.arange(len(cols)), cols] = 1.0
            d_e, d_y = R.dev.put(E), R.dev.put(np.full((len(cols), N), np.nan))
            for k in range(len(cols)):
                R.ctx.smoother_vmult_device(d_e + 8 * N * k, d_y + 8 * N * k)
            R.ctx.synchronize()
            got = R.dev.get(d_y, len(cols) * N).reshape(len(cols), N)
            want = At[:, cols].toarray().T
            assert np.array_equal(got, want), (sid, diag_first, c0, int(np.sum(got != want)))
            R.dev.free()
        assert abs(At - R.A).max() > 0  # (the matrix is not representable in float32: the comparison could tell)
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the product on long rows and large n
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mc.PRODUCT_IDS)
@pytest.mark.parametrize("diag_first", mc.LAYOUTS, ids=LAYOUT_IDS)
def test_shadow_product_on_long_rows_and_large_elements(cid, diag_first):
    """y = A~ x per row within 1e-13 sum_j |a~_ij x_j| of NumPy's product with the rounded matrix read back; the same bits twice; and it
    is not the double product.  n = 125, 343 (odd), 512, 84 (FE_AggloDGP): row groups; rows of 1372, 2048 and 8000 entries: the default
    loop of 1024 entries per trip and its clamped last piece."""
    R = _Resident(cid, diag_first)
    try:
        R.ctx.setup_chebyshev("jacobi", degree=1, max_eigenvalue=1.0)
        R.ctx.set_smoother_precision("f32")
        At = mr.rounded_matrix(R.A)
        x = np.random.default_rng(1).standard_normal(R.N)
        d_x, d_y = R.dev.put(x), R.dev.put(np.full(R.N, np.nan))
        R.ctx.smoother_vmult_device(d_x, d_y)
        R.ctx.synchronize()
        y = R.dev.get(d_y, R.N)
        ref, scale = At @ x, abs(At) @ np.abs(x)
        worst = float(np.max(np.abs(y - ref) / scale))
        print(cid, diag_first, "worst row %.3e of sum |a~ x| (bound 1e-13); against the double product %.3e" %
              (worst, float(np.max(np.abs(y - R.A @ x) / scale))))
        assert np.all(np.abs(y - ref) <= 1e-13 * scale), worst
        assert np.max(np.abs(y - R.A @ x) / scale) > 1e-10
        R.ctx.smoother_vmult_device(d_x, d_y)
        R.ctx.synchronize()
        assert np.array_equal(R.dev.get(d_y, R.N), y)
        assert np.array_equal(R.dev.get(d_x, R.N), x)
    finally:
        R.close()


def test_rows_of_more_than_8192_entries_are_refused_by_the_shadow_too():
    """lds_cap_out: no Chebyshev set-up exists (it is refused), so the precision cannot be chosen; the shadow product names the bound;
    the context then serves a smaller problem in F32"""
    pa = _pa()
    E = pa._capi
    R = _Resident("lds_cap_out", True)
    try:
        d = [R.dev.put(np.ones(R.N)) for _ in range(2)]
        with pytest.raises(pa.PdhError) as e:
            R.ctx.set_smoother_precision("f32")
        assert e.value.code == E.PDH_ESTATE
        with pytest.raises(pa.PdhError) as e:
            R.ctx.smoother_vmult_device(d[0], d[1])
        assert e.value.code == E.PDH_EUNSUPPORTED and "8192" in str(e.value)
        S = _Shape("dgq1_2d", True)
        S.ctx.close()
        R.ctx.set_problem(S.flat)
        R.ctx.assemble()
        A = _global_matrix(R.ctx, S.arr, S.N)
        _f32(R.ctx, "block_jacobi", 2)
        x = np.random.default_rng(2).standard_normal(S.N)
        d_x, d_y = R.dev.put(x), R.dev.put(np.full(S.N, np.nan))
        R.ctx.smoother_vmult_device(d_x, d_y)
        R.ctx.synchronize()
        At = mr.rounded_matrix(A)
        assert np.all(np.abs(R.dev.get(d_y, S.N) - At @ x) <= 1e-13 * (abs(At) @ np.abs(x)))
        S.dev.free()
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Chebyshev applications
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", list(mc.CHEB_SHAPES))
@pytest.mark.parametrize("diag_first", mc.LAYOUTS, ids=LAYOUT_IDS)
def test_chebyshev_applications_with_the_shadow(sid, diag_first):
    """Degrees 1, 2, 5, from zero (pdh_precondition_device) and from a non-zero start (pdh_chebyshev_step_device), every inner kind of
    the shape: within the pair's bound of mixed_ref.apply with the device's lambda_lo / lambda_hi; more than 1000 bounds from the F64
    application of the same context wherever a shadow entry enters (the same bits where none does); the same bits twice."""
    R = _Shape(sid, diag_first)
    try:
        ctx, dev, N = R.ctx, R.dev, R.N
        b, x0 = mc.vectors(N)
        d_b, d_z = dev.put(b), dev.put(np.full(N, np.nan))

        def applications():
            ctx.precondition_device(d_b, d_z)
            ctx.synchronize()
            z = dev.get(d_z, N)
            d_x = dev.put(x0)
            ctx.chebyshev_step_device(d_b, d_x)
            ctx.synchronize()
            return z, dev.get(d_x, N)
        for kind in mc.kinds_of(sid):
            tol, est, S = mc.z_tol(sid, kind), None, None
            for m in mc.DEGREES:
                info = ctx.setup_chebyshev(kind, degree=m, max_eigenvalue=est or 0.0)
                est = info["estimate"]
                lo, hi = info["lambda_lo"], info["lambda_hi"]
                z64, x64 = applications()
                info32, inv64 = _f32(ctx, kind, m, est)
                assert (info32["lambda_lo"], info32["lambda_hi"]) == (lo, hi)
                if S is None:
                    S = mr.Smoother(R.A, R.n, kind, inv64=inv64)
                z, x = applications()
                z2, x2 = applications()
                assert np.array_equal(z, z2) and np.array_equal(x, x2)
                dz, dx = _rel(z, S.apply(lo, hi, m, b)), _rel(x, S.apply(lo, hi, m, b, x0))
                print(sid, diag_first, kind, m, "zero start %.2e, non-zero start %.2e (bound %.3e); against F64 %.2e, %.2e" %
                      (dz, dx, tol, _rel(z, z64), _rel(x, x64)))
                assert dz <= tol and dx <= tol, (kind, m, dz, dx, tol)
                for got, dbl, zero in ((z, z64, True), (x, x64, False)):
                    if not mc.shadow_enters(kind, m, zero):
                        assert np.array_equal(got, dbl)
                    elif (sid, kind) not in mc.ILL_CONDITIONED:
                        assert _rel(got, dbl) > mc.SEPARATION * tol, (kind, m, zero, _rel(got, dbl))
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# V-cycle
# ---------------------------------------------------------------------------------------------------------------------------------
def _switch_levels(L, f32):
    """every level l >= 1 set up again with its own estimate (the mg was closed: the finest needs it; the same polynomial), F32 where
    f32[l]; returns the mixed_ref.Hierarchy of the device's matrices, bounds and stored block inverses"""
    inv = [None] * len(L.ctxs)
    for l in range(1, len(L.ctxs)):
        ctx, est = L.ctxs[l], L.infos[l]["estimate"]
        if f32[l]:
            info, inv[l] = _f32(ctx, L.kind, L.degree, est)
        else:
            info = ctx.setup_chebyshev(L.kind, degree=L.degree, max_eigenvalue=est)
        assert (info["lambda_lo"], info["lambda_hi"]) == (L.infos[l]["lambda_lo"], L.infos[l]["lambda_hi"])
    assert [c.smoother_precision == "f32" for c in L.ctxs] == list(f32)
    return mr.Hierarchy(L.H, f32=f32, inv64=inv)


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_vcycle_and_cg_with_f32_smoothers(case):
    """Every level above the coarsest in F32: three consecutive cycles within the cycle bound + 10 cond_2(A_0) 2.2e-16 of mixed_ref.cycle
    on the matrices read back (relative to |x|_inf), the same bits twice; CG on the finest context takes the iterations of pcg_ref with
    the mixed restatement +-1, converges to rel_tol 1e-13, and its error against spsolve stays within 10 x that of the F64 solve."""
    L = _Levels(case)
    dev = _Device()
    try:
        N, A = L.N, L.mats[-1]
        b = vc.rhs(N)
        x_sp = spla.spsolve(A.tocsc(), b)
        L.attach()
        x64, cg64 = L.finest.solve_cg(b)
        err64 = float(np.linalg.norm(x64 - x_sp) / np.linalg.norm(x_sp))
        L.mg.close()
        L.mg = None
        H = _switch_levels(L, [False] + [True] * (len(L.ctxs) - 1))
        tol = mc.MIXED_CYCLE_TOL + 10.0 * float(np.linalg.cond(L.mats[0].toarray())) * 2.2e-16
        mg = L.attach()
        d_b, d_x, d_z = dev.put(b), dev.put(np.full(N, np.nan)), dev.put(np.full(N, np.nan))
        x_ref = None
        for cyc in range(3):
            mg.vcycle_device(d_b, d_x, zero_initial_guess=(cyc == 0))
            L.finest.synchronize()
            x = dev.get(d_x, N)
            x_ref = mr.cycle(H, b, x_ref)
            print("%s: cycle %d: %.3e (bound %.3e)" % (vc.case_id(case), cyc + 1, _rel(x, x_ref), tol))
            assert _rel(x, x_ref) <= tol, (cyc, _rel(x, x_ref), tol)
            if cyc == 0:
                L.finest.precondition_device(d_b, d_z)
                L.finest.synchronize()
                assert np.array_equal(dev.get(d_z, N), x)
        assert np.array_equal(dev.get(d_b, N), b)
        x32, cg32 = L.finest.solve_cg(b)
        _, it_ref, _ = pcg_ref.pcg(A, b, mr.preconditioner(H), rel_tol=1e-13)
        err32 = float(np.linalg.norm(x32 - x_sp) / np.linalg.norm(x_sp))
        print("%s: CG iterations: F32 smoothers %d (restatement %d), F64 %d; error against spsolve %.3e (F64: %.3e)" %
              (vc.case_id(case), cg32["iterations"], it_ref, cg64["iterations"], err32, err64))
        assert abs(cg32["iterations"] - it_ref) <= 1
        assert cg32["residual"] <= 1e-13 * np.linalg.norm(b)
        assert err32 <= 10.0 * err64
        x2, cg2 = L.finest.solve_cg(b)
        assert np.array_equal(x2, x32) and cg2 == cg32
    finally:
        L.close()
        dev.free()


def test_levels_mix_precisions():
    """16 / 64 / 256 rows with the finest level alone in F32: the cycle is mixed_ref's with f32 = [no, no, yes], and not the one with both
    smoother levels in F32"""
    case = vc.CASES[0]
    L = _Levels(case)
    dev = _Device()
    try:
        H = _switch_levels(L, [False, False, True])
        tol = mc.MIXED_CYCLE_TOL + 10.0 * float(np.linalg.cond(L.mats[0].toarray())) * 2.2e-16
        mg = L.attach()
        b = vc.rhs(L.N)
        d_b, d_x = dev.put(b), dev.put(np.full(L.N, np.nan))
        mg.vcycle_device(d_b, d_x, True)
        L.finest.synchronize()
        x = dev.get(d_x, L.N)
        both = mr.Hierarchy(L.H, f32=[False, True, True], inv64=H.inv64)
        print("finest level alone in F32: %.3e (bound %.3e); against both levels in F32 %.3e" % (_rel(x, mr.cycle(H, b)), tol, _rel(x, mr.cycle(both, b))))
        assert _rel(x, mr.cycle(H, b)) <= tol
        assert _rel(x, mr.cycle(both, b)) > mc.SEPARATION * tol
    finally:
        L.close()
        dev.free()


@pytest.mark.parametrize("diag_first", mc.LAYOUTS, ids=LAYOUT_IDS)
def test_multigrid_hierarchy_with_f32_smoothers(diag_first):
    pa = _pa()
    from polydeal_amd.levels import multigrid_hierarchy

    case = vc.HIERARCHY_CASE
    mirror, _ = vc.handlers(*case)
    assert vc.check_shape(case, mirror) == (27, 216, 1728)
    fe = pa.FE_DGQ(case[0], case[3])
    N = mirror[-1].n_dofs
    b = vc.rhs(N)
    its = {}
    for prec in ("f64", "f32"):
        hier = multigrid_hierarchy(mirror, fe, _variant(fe), diag_first=diag_first, degree=vc.DEGREE, smoother_precision=prec)
        try:
            assert [c.smoother_precision for c in hier.contexts] == ["f64"] + [prec] * 2
            A = _global_matrix(hier.finest, mirror[-1].flatten(_variant(fe), diag_first, True).arrays(), N)
            x, cg = hier.solve_cg(b)
            x_sp = spla.spsolve(A.tocsc(), b)
            assert np.max(np.abs(x - x_sp)) <= 1e-9 * np.max(np.abs(x_sp))
            its[prec] = cg["iterations"]
        finally:
            hier.close()
    print("multigrid_hierarchy (diag_first=%d): iterations %s" % (diag_first, its))
    assert abs(its["f32"] - its["f64"]) <= 1
    with pytest.raises(ValueError):
        multigrid_hierarchy(mirror, fe, _variant(fe), smoother_precision="f16")


# ---------------------------------------------------------------------------------------------------------------------------------
# state rules
# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    pa = _pa()
    E = pa._capi
    L = _Levels(vc.CASES[0])  # 16 / 64 / 256, block Jacobi, Chebyshev(3) on levels 1 and 2, the direct solve on level 0
    dev = _Device()
    fresh = pa.Context(0)
    try:
        c0, c1, c2 = L.ctxs
        N = L.N
        b = vc.rhs(N)
        d_b, d_z = dev.put(b), dev.put(np.full(N, np.nan))

        def refused(call, code, *fragments):
            with pytest.raises(pa.PdhError) as e:
                call()
            assert e.value.code == code, str(e.value)
            for f in fragments:
                assert f in str(e.value), (f, str(e.value))

        def z_of(ctx):
            ctx.precondition_device(d_b, d_z)
            ctx.synchronize()
            return dev.get(d_z, N)
        # no problem, no Chebyshev set-up
        assert fresh.lib.pdh_set_smoother_precision(fresh.h, E.PDH_SMOOTHER_F32) == E.PDH_ESTATE
        assert fresh.lib.pdh_smoother_precision(fresh.h) == E.PDH_ESTATE
        fresh.set_problem(L.mirror[2].flatten(_variant(pa.FE_DGQ(2, 1)), False, True))
        fresh.assemble()
        refused(lambda: fresh.set_smoother_precision("f32"), E.PDH_ESTATE, "PDH_PREC_CHEBYSHEV")
        fresh.setup_preconditioner("block_jacobi")
        refused(lambda: fresh.set_smoother_precision("f32"), E.PDH_ESTATE, "PDH_PREC_CHEBYSHEV")
        refused(lambda: fresh.smoother_vmult_device(d_b, d_z), E.PDH_ESTATE, "PDH_SMOOTHER_F32")
        # the coarsest level has the direct solve, not Chebyshev
        refused(lambda: c0.set_smoother_precision("f32"), E.PDH_ESTATE)
        # a bad value; F64 on an F64 context is fine
        refused(lambda: c2.set_smoother_precision(2), E.PDH_EINVAL, "PDH_SMOOTHER_F32")
        refused(lambda: c2.set_smoother_precision(-1), E.PDH_EINVAL)
        assert c2.smoother_precision == "f64"
        z64 = z_of(c2)
        c2.set_smoother_precision("f64")
        assert np.array_equal(z_of(c2), z64)
        # F32 and back: the bits of a context that never switched (`fresh`, the same matrix)
        c2.set_smoother_precision("f32")
        z32 = z_of(c2)
        assert c2.smoother_precision == "f32" and not np.array_equal(z32, z64)
        c2.set_smoother_precision("f64")
        assert c2.smoother_precision == "f64" and np.array_equal(z_of(c2), z64)
        refused(lambda: c2.smoother_vmult_device(d_b, d_z), E.PDH_ESTATE, "PDH_SMOOTHER_F32")
        fresh.setup_chebyshev(L.kind, degree=L.degree)
        assert np.array_equal(z_of(fresh), z64)
        c2.set_smoother_precision("f32")
        assert np.array_equal(z_of(c2), z32)  # (and F32 again gives the F32 bits again)
        # every later set-up call reports F64 again
        for setup in (lambda: c2.setup_preconditioner("jacobi"), lambda: c2.setup_chebyshev(L.kind, degree=L.degree), lambda: c2.setup_direct()):
            c2.setup_chebyshev(L.kind, degree=L.degree)
            c2.set_smoother_precision("f32")
            assert c2.smoother_precision == "f32"
            setup()
            assert c2.smoother_precision == "f64"
        c2.setup_chebyshev(L.kind, degree=L.degree)
        assert np.array_equal(z_of(c2), z64)
        # the values changed: stale, for the switch and for the shadow product
        c2.set_smoother_precision("f32")
        c2.assemble_device()
        refused(lambda: c2.set_smoother_precision("f32"), E.PDH_ESTATE, "values changed")
        refused(lambda: c2.set_smoother_precision("f64"), E.PDH_ESTATE, "values changed")
        refused(lambda: c2.smoother_vmult_device(d_b, d_z), E.PDH_ESTATE, "values changed")
        refused(lambda: c2.precondition_device(d_b, d_z), E.PDH_ESTATE, "values changed")
        c2.setup_chebyshev(L.kind, degree=L.degree)
        # a multigrid-attached finest context: the precision is chosen before pdh_mg_create
        mg = L.attach()
        refused(lambda: c2.set_smoother_precision("f32"), E.PDH_ESTATE, "pdh_mg_create")
        refused(lambda: c2.set_smoother_precision("f64"), E.PDH_ESTATE, "pdh_mg_create")
        mg.vcycle_device(d_b, d_z, True)
        c2.synchronize()
        # a level's precision changed after pdh_mg_create: the mg is stale and says which level, in either direction
        c1.set_smoother_precision("f32")
        refused(lambda: mg.vcycle_device(d_b, d_z, True), E.PDH_ESTATE, "level 1 of 3")
        refused(lambda: c2.solve_cg(b), E.PDH_ESTATE, "level 1 of 3")
        mg.close()
        L.mg = None
        c2.setup_chebyshev(L.kind, degree=L.degree)
        mg = L.attach()
        mg.vcycle_device(d_b, d_z, True)
        c2.synchronize()
        c1.set_smoother_precision("f64")
        refused(lambda: mg.vcycle_device(d_b, d_z, True), E.PDH_ESTATE, "level 1 of 3")
    finally:
        fresh.close()
        L.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# the example and the headline hierarchy
# ---------------------------------------------------------------------------------------------------------------------------------
def test_poisson_example_smoother_f32():
    """examples/poisson --device-solve --chebyshev 3 --smoother-f32 prints the reference's L2 line; the flag alone is refused"""
    exe = os.path.join(ROOT, "examples", "poisson")
    assert os.path.exists(exe), "examples/poisson is built by __graft_entry__.build()"
    cwd = os.path.join(ROOT, "examples")
    out = subprocess.run([exe, "--device-solve", "--chebyshev", "3", "--smoother-f32"], capture_output=True, text=True, timeout=600, cwd=cwd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert gc.golden_lines("poisson.output")[0] == "L2 error:0.00647702"
    assert "L2 error:0.00647702" in out.stdout.splitlines(), out.stdout
    for args in (["--smoother-f32"], ["--device-solve", "--smoother-f32"]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, cwd=cwd)
        assert out.returncode == 1 and "--smoother-f32" in out.stderr and "L2 error" not in out.stdout, (args, out.stdout, out.stderr)


def test_headline_vcycle_solve_with_f32_smoothers():
    """64^3 cells, FE_DGQ(3), polytopes of 32^3 .. 2^3 cells (8 .. 32 768 polytopes, 2 097 152 rows on the finest level): b = A x* for a random
    x*, solved with the V-cycle in F64 and then, on the same contexts, with every smoother level in F32; the iteration counts differ by
    at most one and the TRUE relative residual |b - A x| / |b| of the F32 solve, formed with the double matrix, is <= 1e-12."""
    pa = _pa()
    from polydeal_amd._capi import Multigrid
    from polydeal_amd.levels import block_hierarchy, multigrid_hierarchy

    fe = pa.FE_DGQ(3, 3)
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 6)
    handlers = block_hierarchy(grid, fe, [32, 16, 8, 4, 2])
    assert [h.n_agglomerates for h in handlers] == [8, 64, 512, 4096, 32768]
    N = handlers[-1].n_dofs
    hier = multigrid_hierarchy(handlers, fe, pa.SipVariant.poisson_example(fe), diag_first=True, degree=3)
    try:
        fin = hier.finest
        xs = np.random.default_rng(21).standard_normal(N)
        b = fin.vmult(xs)
        x64, cg64 = hier.solve_cg(b)
        hier.mg.close()
        hier.mg = None
        fin.setup_chebyshev("block_jacobi", degree=3, max_eigenvalue=hier.info[-1]["estimate"])
        for c in hier.contexts[1:]:
            c.set_smoother_precision("f32")
        hier.mg = Multigrid(hier.contexts, hier.transfers)
        x32, cg32 = hier.solve_cg(b)
        res = float(np.linalg.norm(b - fin.vmult(x32)) / np.linalg.norm(b))
        print("headline V-cycle solve: F64", cg64, "F32 smoothers", cg32, "true relative residual %.3e, |x - x*| / |x*| %.3e (F64: %.3e)" %
              (res, np.linalg.norm(x32 - xs) / np.linalg.norm(xs), np.linalg.norm(x64 - xs) / np.linalg.norm(xs)))
        assert abs(cg32["iterations"] - cg64["iterations"]) <= 1
        assert res <= 1e-12
    finally:
        hier.close()
