"""The solver kernels (csrc/pdh_solve.hip, csrc/pdh_capi_solve.cpp) on the shapes of tests/solve_shape_cases.py: rows longer than 512
entries (row_dot's default loop), more than 64 dofs per polytope in even, odd and whole-multiple-of-64 counts (row groups of k_vmult,
several passes per slot of k_cg_update / k_cheb_update), slot counts that make k_cg_finalise stride, the 64 KB bound of the column set
in LDS from both sides, the stored block inverse entry by entry, and in-place preconditioning.  Every case asserts the property it is
listed for from the flattened arrays before the device is used.

Yardsticks: scipy on the values read back (1e-13 sum_j |a_ij x_j| per row), tests/pcg_ref.py (1e-10, 1e-9), tests/cheb_ref.py and the
long-double block inverse within the constants of solve_shape_cases.py, which were measured on the CPU (100 x the float64-versus-
long-double spread of the yardstick, never below 1e-13)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import cheb_ref as cr
import solve_shape_cases as sc
from pcg_ref import diag_blocks, pcg, preconditioner
from test_gpu_solve import _Device, _check_vmult, _global_matrix, _handler, _kernels

pytestmark = pytest.mark.gpu

LAYOUTS = [True, False]


def _pa():
    import polydeal_amd as pa
    return pa


class _Resident:
    """a case of solve_shape_cases.CASES assembled on the device: context, scipy matrix of the values in HBM, n, N"""

    def __init__(self, cid, diag_first, assemble=True):
        pa = _pa()
        self.ah, self.fe, self.flat = sc.mirror_flat(cid, diag_first)
        self.arr = self.flat.arrays()
        sc.check_property(cid, self.ah, self.fe, self.arr)
        self.n, self.N = self.fe.n_dofs_per_cell, self.ah.n_dofs
        self.ctx = pa.Context(0)
        self.dev = _Device()
        try:
            self.ctx.set_problem(self.flat)
            _kernels(self.ctx)
            if assemble:
                self.ctx.assemble()
                self.A = _global_matrix(self.ctx, self.arr, self.N)
        except Exception:
            self.close()
            raise

    def close(self):
        self.ctx.close()
        self.dev.free()


def _residual_bits(ctx, dev, A, b, x, what):
    """residual_device against b - A x with the bound of test_residual_against_the_values_read_back; the same bits twice"""
    N = len(b)
    d_x, d_b, d_r = dev.put(x), dev.put(b), dev.put(np.full(N, np.nan))
    ctx.residual_device(d_b, d_x, d_r)
    ctx.synchronize()
    res = dev.get(d_r, N)
    scale = abs(A) @ np.abs(x) + np.abs(b)
    bad = np.abs(res - (b - A @ x)) > 1e-13 * scale
    assert not np.any(bad), (what, int(bad.sum()), float(np.max(np.abs(res - (b - A @ x)) / scale)))
    ctx.residual_device(d_b, d_x, d_r)
    ctx.synchronize()
    assert np.array_equal(dev.get(d_r, N), res)


# ---------------------------------------------------------------------------------------------------------------------------------
# A (and E, served side): product and residual
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.VMULT_IDS)
@pytest.mark.parametrize("diag_first", LAYOUTS)
def test_vmult_and_residual_on_long_rows_and_large_elements(cid, diag_first):
    """pdh_vmult against scipy on the values read back, per row within 1e-13 sum_j |a_ij x_j|; pdh_vmult_device and a second call give
    the same bits; pdh_residual_device against b - A x.  lds_cap_in launches k_vmult with 64 000 B of dynamic LDS."""
    R = _Resident(cid, diag_first)
    try:
        rng = np.random.default_rng(1)
        x, b = rng.standard_normal(R.N), rng.standard_normal(R.N)
        y = _check_vmult(R.ctx, R.A, x, (cid, diag_first))
        d_x, d_y = R.dev.put(x), R.dev.put(np.full(R.N, np.nan))
        R.ctx.vmult_device(d_x, d_y)
        R.ctx.synchronize()
        assert np.array_equal(R.dev.get(d_y, R.N), y)
        assert np.array_equal(R.ctx.vmult(x), y)
        _residual_bits(R.ctx, R.dev, R.A, b, x, (cid, diag_first))
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# B: three CG steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.CG3_IDS)
@pytest.mark.parametrize("diag_first", LAYOUTS)
def test_three_cg_steps_against_the_host_loop(cid, diag_first):
    """solve_cg(b, max_iter=3) raises PDH_ENOCONV carrying the iterate: within 1e-10 of pcg_ref's third iterate, and ||r|| within 1e-10
    of its.  Pins the p^T q partials of k_vmult, the multi-pass updates, alpha and beta without paying for convergence.
    Every figure was measured at 2.3e-15 or below except dgq3_grown with block Jacobi: 1.6e-11 / 7.2e-11 (iterate, the two layouts) and
    8.2e-11 / 1.2e-11 (residual).  There the diagonal blocks have cond_2 up to 6e9 (FE_DGQ(3) on the bounding box of an irregular
    agglomerate), and the yardstick itself moves by 1.0e-10 when its numpy.linalg.inv is replaced by the long-double inverse: the
    figures are the conditioning of the blocks, in the device's Cholesky as in NumPy's LU, not a summation order."""
    pa = _pa()
    from polydeal_amd import _capi

    R = _Resident(cid, diag_first)
    try:
        b = sc.rhs(R.N)
        for kind in sc.kinds_of(cid):
            R.ctx.setup_preconditioner(kind)
            with pytest.raises(pa.PdhError) as e:
                R.ctx.solve_cg(b, max_iter=3)
            assert e.value.code == _capi.PDH_ENOCONV and e.value.info["iterations"] == 3, (kind, e.value.info)
            x3, it3, res3 = pcg(R.A, b, preconditioner(R.A, R.n, kind), max_iter=3)
            assert it3 == 3 and np.all(np.isfinite(x3)) and res3 > 1e-13 * np.linalg.norm(b)
            dx = float(np.linalg.norm(e.value.x - x3) / np.linalg.norm(x3))
            dr = abs(e.value.info["residual"] - res3) / res3
            print(cid, diag_first, kind, "iterate %.3e residual %.3e (relative; bound 1e-10)" % (dx, dr))
            assert dx <= 1e-10 and dr <= 1e-10, (kind, dx, dr)
            assert e.value.info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# C: many slots
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.SLOT_IDS)
@pytest.mark.parametrize("diag_first", LAYOUTS)
def test_cg_and_estimate_with_many_slots(cid, diag_first):
    """289 and 1024 slots: every thread of k_cg_finalise adds one, two (some) or four partials.  CG as in
    test_cg_against_spsolve_and_the_host_loop for the three kinds; the Chebyshev estimate, which reads alpha and beta of every step,
    against cheb_ref.estimate within SLOT_EST_TOL."""
    R = _Resident(cid, diag_first)
    try:
        b = sc.rhs(R.N)
        ref = spla.spsolve(R.A.tocsc(), b)
        for kind in ("none", "jacobi", "block_jacobi"):
            R.ctx.setup_preconditioner(kind)
            x, info = R.ctx.solve_cg(b)
            _, it_ref, _ = pcg(R.A, b, preconditioner(R.A, R.n, kind))
            assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), (kind, info)
            assert abs(info["iterations"] - it_ref) <= 1, (kind, info, it_ref)
            assert info["residual"] <= 1e-13 * np.linalg.norm(b) and info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
            x2, info2 = R.ctx.solve_cg(b)
            assert np.array_equal(x, x2) and info == info2, kind
        for kind in ("jacobi", "block_jacobi"):
            info = R.ctx.setup_chebyshev(kind, degree=2)
            est_ref, steps_ref = cr.estimate(R.A, R.n, kind)
            de = abs(info["estimate"] - est_ref) / est_ref
            print(cid, diag_first, kind, "estimate %.15g (ref %.15g, rel %.2e, bound %.3e)" % (info["estimate"], est_ref, de, sc.SLOT_EST_TOL))
            assert info["cg_iterations"] == steps_ref == 20
            assert de <= sc.SLOT_EST_TOL, (kind, info, est_ref)
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# D: Chebyshev applications
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sc.CHEB_IDS)
@pytest.mark.parametrize("diag_first", LAYOUTS)
def test_chebyshev_applications_on_long_rows_and_large_elements(cid, diag_first):
    """Degrees 1, 2, 5 from a zero (pdh_precondition_device) and a non-zero start (pdh_chebyshev_step_device) against cheb_ref.apply
    with the device's lambda_lo / lambda_hi, within SHAPE_Z_TOL |z|_inf."""
    R = _Resident(cid, diag_first)
    try:
        b, x0 = sc.vectors(R.N)
        d_b, d_z = R.dev.put(b), R.dev.put(np.full(R.N, np.nan))
        for kind in sc.cheb_kinds(cid):
            for m in sc.CHEB_DEGREES:
                info = R.ctx.setup_chebyshev(kind, degree=m)
                lo, hi = info["lambda_lo"], info["lambda_hi"]
                R.ctx.precondition_device(d_b, d_z)
                R.ctx.synchronize()
                z = R.dev.get(d_z, R.N)
                ref = cr.apply(R.A, R.n, kind, lo, hi, m, b)
                dz = float(np.max(np.abs(z - ref)) / np.max(np.abs(ref)))
                d_x = R.dev.put(x0)
                R.ctx.chebyshev_step_device(d_b, d_x)
                R.ctx.synchronize()
                ref1 = cr.apply(R.A, R.n, kind, lo, hi, m, b, x0)
                dx = float(np.max(np.abs(R.dev.get(d_x, R.N) - ref1)) / np.max(np.abs(ref1)))
                print(cid, diag_first, kind, m, "zero start %.2e, non-zero start %.2e (bound %.3e)" % (dz, dx, sc.SHAPE_Z_TOL))
                assert dz <= sc.SHAPE_Z_TOL and dx <= sc.SHAPE_Z_TOL, (kind, m, dz, dx)
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# E: the column set of a polytope does not fit 64 KB of LDS
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_of_more_than_8192_entries_are_refused():
    """lds_cap_out (8256 entries in a row): pdh_vmult, pdh_vmult_device, pdh_residual_device, pdh_solve_cg and pdh_setup_chebyshev
    answer PDH_EUNSUPPORTED naming the bound, and the context then serves a smaller problem."""
    pa = _pa()
    from polydeal_amd import _capi

    R = _Resident("lds_cap_out", True)
    try:
        lib, h, N = R.ctx.lib, R.ctx.h, R.N
        v = [R.dev.put(np.ones(N)) for _ in range(3)]
        hx, hy = np.ones(N), np.zeros(N)
        ctl, res = _capi.pdh_cg_control(10, 1e-13, 0.0), _capi.pdh_cg_result()
        cheb = _capi.pdh_chebyshev_control(_capi.PDH_PREC_JACOBI, 2, 20.0, 20, 0.0)
        calls = {
            "pdh_vmult": lambda: lib.pdh_vmult(h, hx.ctypes.data, hy.ctypes.data),
            "pdh_vmult_device": lambda: lib.pdh_vmult_device(h, C.c_void_p(v[0]), C.c_void_p(v[1])),
            "pdh_residual_device": lambda: lib.pdh_residual_device(h, C.c_void_p(v[0]), C.c_void_p(v[1]), C.c_void_p(v[2])),
            "pdh_solve_cg": lambda: lib.pdh_solve_cg(h, C.byref(ctl), C.c_void_p(hx.ctypes.data), C.c_void_p(hy.ctypes.data), C.byref(res)),
            "pdh_setup_chebyshev": lambda: lib.pdh_setup_chebyshev(h, C.byref(cheb), None),
        }
        for name, call in calls.items():
            assert call() == _capi.PDH_EUNSUPPORTED, name
            assert "8192" in lib.pdh_last_error(h).decode(), (name, lib.pdh_last_error(h).decode())
        assert not np.any(hy)
        ah, fe = _handler(2, 8, 2, "dgq", 1)
        flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, True)
        R.ctx.set_problem(flat)
        R.ctx.assemble()
        A = _global_matrix(R.ctx, flat.arrays(), ah.n_dofs)
        _check_vmult(R.ctx, A, np.random.default_rng(2).standard_normal(ah.n_dofs), "after the refusals")
        R.ctx.setup_chebyshev("jacobi", degree=2)
        x, info = R.ctx.solve_cg(R.ctx.vmult(np.ones(ah.n_dofs)))
        assert np.max(np.abs(x - 1.0)) <= 1e-9, info
    finally:
        R.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# F: the stored block inverse
# ---------------------------------------------------------------------------------------------------------------------------------
def _inverse_problem(iid, diag_first):
    """(pdh problem, arrays with rowptr / colind, n, N) of a case of INVERSE_CASES"""
    pa = _pa()
    spec = sc.INVERSE_CASES[iid]
    if spec[0] == "aniso":
        from flatten_oracle import flatten
        from oracle import polydeal_oracle as po

        oah = sc.inverse_oracle_handler(iid)
        kw = flatten(oah, po.variant_poisson_example(oah.fe), diag_first=diag_first)
        return pa.Problem(**kw), kw, oah.fe.n_dofs_per_cell, oah.n_dofs
    if spec[0] == "block":
        ah, fe = _handler(*spec[1:])
        flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    else:
        ah, fe, flat = sc.mirror_flat(spec[1], diag_first)
        sc.check_property(spec[1], ah, fe, flat.arrays())
    return flat, flat.arrays(), fe.n_dofs_per_cell, ah.n_dofs


def _stored_inverse(ctx, dev, n, N):
    """[N / n][n][n]: with r = e_j in every block, z_i = sum_k D[k][i] r_k = D[j][i] and every other term is an exact zero, so n
    applications read every stored entry bit for bit"""
    D = np.zeros((N // n, n, n))
    d_z = dev.put(np.full(N, np.nan))
    for j in range(n):
        r = np.zeros((N // n, n))
        r[:, j] = 1.0
        d_r = dev.put(r.ravel())
        ctx.precondition_device(d_r, d_z)
        ctx.synchronize()
        D[:, j, :] = dev.get(d_z, N).reshape(-1, n)
    return D


@pytest.mark.parametrize("iid", list(sc.INVERSE_CASES))
@pytest.mark.parametrize("diag_first", LAYOUTS)
def test_stored_block_inverse_is_symmetric_and_accurate(iid, diag_first):
    """k_block_inverse promises an exactly symmetric stored inverse (both apply kernels read it by columns): every block equals its
    transpose bit for bit and is within INVERSE_TOL max |D^-1| of the long-double inverse of the block read back.  On the two
    anisotropic meshes block-Jacobi CG then solves against spsolve with the bounds of test_cg_against_spsolve_and_the_host_loop."""
    pa = _pa()
    prob, arr, n, N = _inverse_problem(iid, diag_first)
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(prob)
        _kernels(ctx)
        ctx.assemble()
        A = _global_matrix(ctx, arr, N)
        blocks = diag_blocks(A, n)
        ctx.setup_preconditioner("block_jacobi")
        D = _stored_inverse(ctx, dev, n, N)
        assert np.all(np.isfinite(D))
        assert np.array_equal(D, D.transpose(0, 2, 1))
        ref = cr.batched_inverse(blocks, np.longdouble)
        err = np.max(np.abs(D.astype(np.longdouble) - ref), axis=(1, 2)) / np.max(np.abs(ref), axis=(1, 2))
        print(iid, diag_first, "stored inverse: worst block %.3e of max |D^-1| (bound %.3e)" % (float(err.max()), sc.INVERSE_TOL[iid]))
        assert float(err.max()) <= sc.INVERSE_TOL[iid], (int(err.argmax()), float(err.max()))
        if iid in sc.ANISO_CG_IDS:
            b = sc.rhs(N)
            ref_x = spla.spsolve(A.tocsc(), b)
            x, info = ctx.solve_cg(b)
            _, it_ref, _ = pcg(A, b, preconditioner(A, n, "block_jacobi"))
            cond = float(np.linalg.cond(A.toarray()))
            dx = float(np.linalg.norm(x - ref_x) / np.linalg.norm(ref_x))
            print(iid, diag_first, "cond_2(A) = %.3e, |x - spsolve| / |spsolve| = %.3e" % (cond, dx), info, "reference iterations", it_ref)
            assert dx <= 1e-9, info
            assert abs(info["iterations"] - it_ref) <= 1, (info, it_ref)
            assert info["residual"] <= 1e-13 * np.linalg.norm(b) and info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
    finally:
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# G: aliasing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kinds", [((2, 8, 2, "dgq", 2), ("none", "jacobi", "block_jacobi", ("block_jacobi", 3), ("jacobi", 3))),
                                         ((3, 2, 1, "dgq", 4), ("none", "jacobi", ("jacobi", 3)))], ids=["n9", "n125"])
def test_preconditioning_in_place_and_partial_overlap(shape, kinds):
    """pdh_precondition_device(d, d) gives the bits of the out-of-place call for every kind (Chebyshev of degree 3 over both inner
    kinds; n = 125: two passes per slot); a partial overlap of r and z, either order of the shifted pointer, is PDH_EINVAL;
    pdh_chebyshev_step_device keeps refusing any overlap."""
    pa = _pa()
    from polydeal_amd import _capi

    ah, fe = _handler(*shape)
    N = ah.n_dofs
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), True, True))
        ctx.assemble()
        r = np.random.default_rng(6).standard_normal(N)
        d_r, d_z = dev.put(r), dev.put(np.full(N, np.nan))
        for kind in kinds:
            if isinstance(kind, tuple):
                ctx.setup_chebyshev(kind[0], degree=kind[1])
            else:
                ctx.setup_preconditioner(kind)
            ctx.precondition_device(d_r, d_z)
            ctx.synchronize()
            z = dev.get(d_z, N)
            assert np.array_equal(dev.get(d_r, N), r) and np.all(np.isfinite(z))
            if kind != "none":
                assert not np.array_equal(z, r)
            d_io = dev.put(r)
            ctx.precondition_device(d_io, d_io)
            ctx.synchronize()
            assert np.array_equal(dev.get(d_io, N), z), kind
            for a, b in ((d_io, d_io + 8), (d_io + 8, d_io), (d_io, d_io + 8 * (N - 1)), (d_io + 8 * (N - 1), d_io)):
                assert ctx.lib.pdh_precondition_device(ctx.h, C.c_void_p(a), C.c_void_p(b)) == _capi.PDH_EINVAL, kind
                assert "overlap" in ctx.lib.pdh_last_error(ctx.h).decode()
            ctx.synchronize()
            assert np.array_equal(dev.get(d_io, N), z)  # the refused calls wrote nothing
            if isinstance(kind, tuple):
                for a, b in ((d_io, d_io), (d_io, d_io + 8 * (N - 1)), (d_io + 8 * (N - 1), d_io)):
                    assert ctx.lib.pdh_chebyshev_step_device(ctx.h, C.c_void_p(a), C.c_void_p(b), 1) == _capi.PDH_EINVAL
                    assert "overlap" in ctx.lib.pdh_last_error(ctx.h).decode()
    finally:
        ctx.close()
        dev.free()
