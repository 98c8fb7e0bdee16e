"""The Chebyshev smoother / preconditioner on the resident matrix (csrc/pdh_solve.hip: k_cheb_update; C ABI: pdh_setup_chebyshev,
pdh_chebyshev_step_device, PDH_PREC_CHEBYSHEV in pdh_precondition_device and pdh_solve_cg) against its NumPy restatement
(tests/cheb_ref.py) on the matrix as read back from the device.

Tolerances (tests/cheb_cases.py, measured on the CPU, not on the device): cheb_ref in float64 against cheb_ref in numpy.longdouble on
the cases below, both layouts, both inner kinds, degrees 1, 2, 5, zero and non-zero start, differs by at most 1.596e-14 |z|_inf in an
application and by 2.662e-15 est in the estimate.  The device may differ from the float64 yardstick by 100 x that: 1.596e-12 |z|_inf
and 2.662e-13 est."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import cheb_cases as cc
import cheb_ref as cr
import golden_cases as gc
from pcg_ref import pcg, preconditioner
from test_gpu_solve import _Device, _global_matrix, _handler, _kernels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pa():
    import polydeal_amd as pa
    return pa


def _resident(case, diag_first):
    """(context with the assembled case, scipy matrix of the values in HBM, n, N)"""
    pa = _pa()
    dim, cells, per, basis, p, kind = case[:6]
    ah, fe = _handler(dim, cells, per, basis, p, kind)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(flat)
        _kernels(ctx)
        ctx.assemble()
        A = _global_matrix(ctx, flat.arrays(), ah.n_dofs)
    except Exception:
        ctx.close()
        raise
    return ctx, A, fe.n_dofs_per_cell, ah.n_dofs, ah.n_agglomerates


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
@pytest.mark.parametrize("diag_first", [True, False])
def test_estimate_and_applications_against_numpy(case, diag_first):
    """info.estimate against cheb_ref's on the same matrix; pdh_precondition_device and pdh_chebyshev_step_device (zero and non-zero
    start) against cheb_ref with the DEVICE's lambda_lo / lambda_hi, degrees 1, 2, 5, every inner kind of the case; the same call
    twice gives the same bits; the matrix in HBM is the oracle's of the CPU test."""
    ctx, A, n, N, nA = _resident(case, diag_first)
    dev = _Device()
    try:
        if case[1:3] == (2, 2):
            assert nA == 1
        Ao, _ = cc.oracle_system(case, diag_first)
        assert abs(A - Ao).max() <= 1e-11 * abs(Ao).max()
        b, x0 = cc.vectors(N)
        d_b, d_x, d_z = dev.put(b), dev.put(x0), dev.put(np.full(N, np.nan))
        for kind in case[6]:
            est_ref, steps_ref = cr.estimate(A, n, kind)
            for m in cc.DEGREES:
                info = ctx.setup_chebyshev(kind, degree=m)
                de = abs(info["estimate"] - est_ref) / est_ref
                print(cc.case_id(case), diag_first, kind, m, "estimate %.15g (ref %.15g, rel %.2e), %d steps" %
                      (info["estimate"], est_ref, de, info["cg_iterations"]))
                assert de <= cc.EST_TOL, (kind, info, est_ref)
                assert 1 <= info["cg_iterations"] <= 20 and info["degree"] == m and info["inner"] == kind
                lo, hi = info["lambda_lo"], info["lambda_hi"]
                assert hi == 1.2 * info["estimate"] and lo == hi / 20.0
                # z = M b from zero: the preconditioner entry and the smoother entry
                ctx.precondition_device(d_b, d_z)
                ctx.synchronize()
                z = dev.get(d_z, N)
                ref = cr.apply(A, n, kind, lo, hi, m, b)
                dz = np.max(np.abs(z - ref)) / np.max(np.abs(ref))
                ctx.chebyshev_step_device(d_b, d_z, True)
                ctx.synchronize()
                assert np.array_equal(dev.get(d_z, N), z)
                assert np.array_equal(ctx.chebyshev_step(b), z)
                # non-zero start
                xs = []
                for _ in range(2):
                    assert dev.hip.hipMemcpy(C.c_void_p(d_x), C.c_void_p(x0.ctypes.data), x0.nbytes, 1) == 0
                    ctx.chebyshev_step_device(d_b, d_x)
                    ctx.synchronize()
                    xs.append(dev.get(d_x, N))
                assert np.array_equal(xs[0], xs[1])
                ref1 = cr.apply(A, n, kind, lo, hi, m, b, x0)
                dx = np.max(np.abs(xs[0] - ref1)) / np.max(np.abs(ref1))
                print("   application: zero start %.2e, non-zero start %.2e (relative to |z|_inf; bound %.3e)" % (dz, dx, cc.Z_TOL))
                assert dz <= cc.Z_TOL and dx <= cc.Z_TOL, (kind, m, dz, dx)
            # a given max_eigenvalue replaces the estimate: no CG step, the same polynomial as the estimate's own value
            given = ctx.setup_chebyshev(kind, degree=5, max_eigenvalue=info["estimate"])
            assert given["cg_iterations"] == 0 and given["estimate"] == info["estimate"] and given["lambda_hi"] == info["lambda_hi"]
            ctx.precondition_device(d_b, d_z)
            ctx.synchronize()
            assert np.array_equal(dev.get(d_z, N), z)
    finally:
        ctx.close()
        dev.free()


@pytest.mark.parametrize("case", [c for c in cc.CASES if "block_jacobi" in c[6] and c[1:3] != (2, 2)], ids=cc.case_id)
@pytest.mark.parametrize("diag_first", [True, False])
def test_cg_with_chebyshev(case, diag_first):
    """pdh_solve_cg preconditioned with Chebyshev (block Jacobi, degree 3): x within 1e-9 of spsolve and the residual within the
    bound (as test_cg_against_spsolve_and_the_host_loop), iterations within one of pcg with cheb_ref, strictly fewer than with block
    Jacobi on the same problem; two solves and the device entry give the same bits; the other kinds still work afterwards."""
    ctx, A, n, N, _ = _resident(case, diag_first)
    dev = _Device()
    try:
        b = np.random.default_rng(8).standard_normal(N)
        ref = spla.spsolve(A.tocsc(), b)
        ctx.setup_preconditioner("block_jacobi")
        xb, info_b = ctx.solve_cg(b)
        for kind, m in (("block_jacobi", 3), ("jacobi", 2)):
            ch = ctx.setup_chebyshev(kind, degree=m)
            x, info = ctx.solve_cg(b)
            _, it_ref, _ = pcg(A, b, cr.chebyshev_preconditioner(A, n, kind, ch["lambda_lo"], ch["lambda_hi"], m))
            print(cc.case_id(case), diag_first, kind, m, info, "reference iterations", it_ref, "block Jacobi", info_b["iterations"])
            assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), (kind, info)
            assert abs(info["iterations"] - it_ref) <= 1, (kind, info, it_ref)
            assert info["residual"] <= 1e-13 * np.linalg.norm(b) and info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
            if kind == "block_jacobi":
                assert info["iterations"] < info_b["iterations"], (info, info_b)
            x2, info2 = ctx.solve_cg(b)
            assert np.array_equal(x, x2) and info == info2
            d_b, d_x = dev.put(b), dev.put(np.zeros(N))
            assert ctx.solve_cg_device(d_b, d_x) == info
            assert np.array_equal(dev.get(d_x, N), x)
        # the existing kinds are untouched by a Chebyshev set-up before them
        ctx.setup_preconditioner("block_jacobi")
        xb2, info_b2 = ctx.solve_cg(b)
        assert np.array_equal(xb, xb2) and info_b == info_b2
        _, it_b, _ = pcg(A, b, preconditioner(A, n, "block_jacobi"))
        assert abs(info_b["iterations"] - it_b) <= 1
    finally:
        ctx.close()
        dev.free()


def test_chebyshev_failures():
    """Host-side refusals: bad control values (PDH_EINVAL), block inner with n > 64 and a row-range context (PDH_EUNSUPPORTED), values
    changed since the set-up (PDH_ESTATE), an indefinite diagonal block (PDH_EINVAL naming its polytope), overlapping b and x, the
    smoother without a Chebyshev set-up, and pdh_setup_preconditioner(3) as before."""
    pa = _pa()
    from polydeal_amd import _capi
    from pcg_ref import diag_blocks

    ah, fe = _handler(2, 8, 2, "dgq", 2)
    n, N = fe.n_dofs_per_cell, ah.n_dofs
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, True)
    ctx = pa.Context(0)
    dev = _Device()
    try:
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_chebyshev()
        assert e.value.code == _capi.PDH_ESTATE
        ctx.set_problem(flat)
        ctx.assemble()
        d_b, d_x = dev.put(np.ones(N)), dev.put(np.zeros(N))
        with pytest.raises(pa.PdhError) as e:
            ctx.chebyshev_step_device(d_b, d_x)
        assert e.value.code == _capi.PDH_ESTATE
        for bad in (dict(degree=0), dict(degree=-2), dict(smoothing_range=1.0), dict(smoothing_range=0.5), dict(inner=0), dict(inner=3),
                    dict(inner=7), dict(eig_cg_n_iterations=0), dict(eig_cg_n_iterations=257), dict(smoothing_range=float("nan")),
                    dict(max_eigenvalue=float("inf"))):
            with pytest.raises(pa.PdhError) as e:
                ctx.setup_chebyshev(**bad)
            assert e.value.code == _capi.PDH_EINVAL, bad
        assert ctx.lib.pdh_setup_chebyshev(ctx.h, None, None) == _capi.PDH_EINVAL
        assert ctx.lib.pdh_setup_preconditioner(ctx.h, 3) == _capi.PDH_EINVAL
        # info may be NULL; eig_cg_n_iterations is not looked at when max_eigenvalue is given
        ctl = _capi.pdh_chebyshev_control(_capi.PDH_PREC_JACOBI, 2, 20.0, 0, 2.5)
        assert ctx.lib.pdh_setup_chebyshev(ctx.h, C.byref(ctl), None) == _capi.PDH_OK
        assert ctx.lib.pdh_chebyshev_step_device(ctx.h, C.c_void_p(d_b), C.c_void_p(d_b), 1) == _capi.PDH_EINVAL
        assert "overlap" in ctx.lib.pdh_last_error(ctx.h).decode()
        assert ctx.lib.pdh_chebyshev_step_device(ctx.h, None, C.c_void_p(d_x), 1) == _capi.PDH_EINVAL
        ctx.chebyshev_step_device(d_b, d_x, True)
        ctx.synchronize()
        # the values change: every user of the set-up refuses
        ctx.setup_chebyshev()
        ctx.assemble_device()
        for call in (lambda: ctx.solve_cg(np.ones(N)), lambda: ctx.precondition_device(d_b, d_x),
                     lambda: ctx.chebyshev_step_device(d_b, d_x)):
            with pytest.raises(pa.PdhError) as e:
                call()
            assert e.value.code == _capi.PDH_ESTATE
        ctx.setup_chebyshev()
        ctx.solve_cg(np.ones(N))
        # a row range
        ctx.set_problem(flat, 0, (ah.n_agglomerates // 2) * n)
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_chebyshev()
        assert e.value.code == _capi.PDH_EUNSUPPORTED and "all rows" in str(e.value)
        # an indefinite block (test_preconditioner_failures' problem)
        kw = {k: (None if v is None else np.array(v)) for k, v in flat.arrays().items()}
        c = flat.c
        kw.update(dim=c.dim, degree=c.degree, basis=c.basis, n_agg=c.n_agg, n_faces=c.n_faces, n_rows=c.n_rows, diag_first=1)
        kw["face_sigma"] = -1e3 * np.abs(kw["face_sigma"])
        ctx.set_problem(pa.Problem(**kw))
        ctx.assemble()
        blocks = diag_blocks(_global_matrix(ctx, kw, N), n)
        first = min(P for P in range(len(blocks)) if np.linalg.eigvalsh(blocks[P]).min() <= 0)
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_chebyshev("block_jacobi")
        assert e.value.code == _capi.PDH_EINVAL and ("polytope %d " % first) in str(e.value), (str(e.value), first)
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(np.ones(N))
        assert e.value.code == _capi.PDH_ESTATE
        # more than 64 dofs per polytope: block inner refused, point Jacobi inner solves
        ah4, fe4 = _handler(3, 2, 1, "dgq", 4)
        ctx.set_problem(ah4.flatten(pa.SipVariant.poisson_example(fe4), True, True))
        _kernels(ctx, ("direct", "none"))
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_chebyshev("block_jacobi")
        assert e.value.code == _capi.PDH_EUNSUPPORTED
        ctx.setup_chebyshev("jacobi", degree=3)
        x, info = ctx.solve_cg(ctx.vmult(np.ones(ah4.n_dofs)), rel_tol=1e-12)
        assert np.max(np.abs(x - 1.0)) <= 1e-8, info
    finally:
        ctx.close()
        dev.free()


def test_poisson_example_chebyshev():
    """examples/poisson --device-solve --chebyshev 3 prints the reference's L2 line."""
    exe = os.path.join(ROOT, "examples", "poisson")
    assert os.path.exists(exe), "examples/poisson is built by __graft_entry__.build()"
    out = subprocess.run([exe, "--device-solve", "--chebyshev", "3"], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert gc.golden_lines("poisson.output")[0] == "L2 error:0.00647702"
    assert "L2 error:0.00647702" in out.stdout.splitlines(), out.stdout


def test_headline_solve_with_the_default_chebyshev():
    """64^3 cells, 32 768 polytopes, FE_DGQ(3): set-up with the defaults (block Jacobi, degree 5, range 20, 20 CG steps), b = A x* for
    a random x*, solved to the rel_tol of test_headline_vmult_identities_and_block_jacobi_cg (1e-14); |x - x*| / |x*| <= 1e-8, that
    test's bound."""
    pa = _pa()
    fe = pa.FE_DGQ(3, 3)
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 6)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    ah.initialize_fe_values(4, 4)
    ah.distribute_agglomerated_dofs(fe)
    N = ah.n_dofs
    assert ah.n_agglomerates == 32768
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, False)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(flat)
        _kernels(ctx, ("rows", "terms"))
        ctx.assemble_device()
        xs = np.random.default_rng(21).standard_normal(N)
        b = ctx.vmult(xs)
        ch = ctx.setup_chebyshev()
        assert ch["cg_iterations"] == 20 and ch["degree"] == 5 and ch["inner"] == "block_jacobi" and 1.0 < ch["estimate"] < 4.0, ch
        x, info = ctx.solve_cg(b, rel_tol=1e-14)
        print("headline:", ch, info)
        assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs), info
        assert 0 < info["iterations"] < 20000 and info["residual"] <= 1e-14 * np.linalg.norm(b)
    finally:
        ctx.close()
