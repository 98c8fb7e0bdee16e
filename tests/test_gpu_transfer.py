"""Level transfers on the device (csrc/pdh_transfer.hip): prolongation and restriction against the dense injection of the oracle, their
accumulating and host-pointer forms, reproducibility, the adjoint identity, the interpolation property of the reference's
distributed_injection_01, pdh_residual_device, the C++ mirror, the argument errors, the two-grid cycle composed of device calls against
its NumPy restatement (tests/twogrid_ref.py), and the headline pair through closed-form properties."""
import ctypes as C

import numpy as np
import pytest

import transfer_cases as tc
from test_gpu_solve import _Device, _global_matrix, _handler

pytestmark = pytest.mark.gpu

TOL = 1e-13  # the project's vmult bound: per row, relative to the sum of the absolute terms


def _pa():
    import polydeal_amd as pa
    return pa


def _within(got, ref, scale, what):
    bad = np.abs(got - ref) > TOL * scale
    worst = float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-300)))
    print("%s: max error / scale = %.3e" % (what, worst))
    assert not np.any(bad), (what, int(bad.sum()), worst)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_transfer_against_the_dense_injection(case):
    pa = _pa()
    from polydeal_amd._capi import Transfer

    c = tc.build(case)
    d, P = c.desc, c.P
    aP = np.abs(P)
    rng = np.random.default_rng(11)
    x, r, y = rng.standard_normal(d.n_coarse_rows), rng.standard_normal(d.n_fine_rows), rng.standard_normal(d.n_fine_rows)
    dst_f, dst_c = rng.standard_normal(d.n_fine_rows), rng.standard_normal(d.n_coarse_rows)
    ctx = pa.Context(0)
    dev = _Device()
    t = None
    try:
        t = Transfer(ctx, d)  # no resident problem
        d_x, d_r, d_y = dev.put(x), dev.put(r), dev.put(y)
        d_f, d_c = dev.put(np.full(d.n_fine_rows, np.nan)), dev.put(np.full(d.n_coarse_rows, np.nan))

        def run(fn, src, dst, n):
            fn(src, dst)
            ctx.synchronize()
            return dev.get(dst, n)
        # prolongation
        Px = run(t.prolongate_device, d_x, d_f, d.n_fine_rows)
        _within(Px, P @ x, aP @ np.abs(x), "prolongate")
        assert np.array_equal(run(t.prolongate_device, d_x, d_f, d.n_fine_rows), Px)
        assert np.array_equal(t.prolongate(x), Px)
        # restriction
        Ptr = run(t.restrict_device, d_r, d_c, d.n_coarse_rows)
        _within(Ptr, P.T @ r, aP.T @ np.abs(r), "restrict")
        assert np.array_equal(run(t.restrict_device, d_r, d_c, d.n_coarse_rows), Ptr)
        assert np.array_equal(t.restrict(r), Ptr)
        # accumulating forms on a random destination, twice from the same start
        runs = []
        for _ in range(2):
            d_df, d_dc = dev.put(dst_f), dev.put(dst_c)
            runs.append((run(t.prolongate_and_add_device, d_x, d_df, d.n_fine_rows), run(t.restrict_and_add_device, d_r, d_dc, d.n_coarse_rows)))
        got_f, got_c = runs[0]
        assert np.array_equal(runs[1][0], got_f) and np.array_equal(runs[1][1], got_c)
        _within(got_f, dst_f + P @ x, np.abs(dst_f) + aP @ np.abs(x), "prolongate_and_add")
        _within(got_c, dst_c + P.T @ r, np.abs(dst_c) + aP.T @ np.abs(r), "restrict_and_add")
        # adjoint identity from device results alone: y^T (P x) = (P^T y)^T x
        Pty = run(t.restrict_device, d_y, d_c, d.n_coarse_rows)
        lhs, rhs = float(y @ Px), float(Pty @ x)
        bound = TOL * (float(np.abs(y) @ (aP @ np.abs(x))) + float((aP.T @ np.abs(y)) @ np.abs(x)))
        print("adjoint: |lhs - rhs| = %.3e, bound %.3e" % (abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound
        # the property of the reference's distributed_injection_01: a coarse interpolant of a degree-p polynomial is reproduced
        f = tc.poly(d.dim, d.degree)
        err = t.prolongate(tc.interpolate(d, "coarse", f)) - tc.interpolate(d, "fine", f)
        print("interpolant: max error = %.3e" % float(np.max(np.abs(err))))
        assert np.max(np.abs(err)) < 5e-13
    finally:
        if t is not None:
            t.close()
        ctx.close()
        dev.free()


def test_mirror_transfer_and_level_transfer():
    """Utils::MGTransferAgglomeration of the C++ mirror (through pdhh_mg_transfer_apply) and levels.level_transfer give the bits of the
    C ABI on the same description; fill_injection_matrix still gives the same matrix."""
    pa = _pa()
    from polydeal_amd.handler import mg_transfer_apply
    from polydeal_amd.levels import level_transfer

    case = ("pair", 3, 2, 4, 2, 2, 0.1)
    c = tc.build(case)
    coarse, fine = c.handlers
    rng = np.random.default_rng(11)
    x, r = rng.standard_normal(coarse.n_dofs), rng.standard_normal(fine.n_dofs)
    dst_f, dst_c = rng.standard_normal(fine.n_dofs), rng.standard_normal(coarse.n_dofs)
    ctx = pa.Context(0)
    t = None
    try:
        t = level_transfer(ctx, coarse, fine)
        Px, Ptr = t.prolongate(x), t.restrict(r)
    finally:
        if t is not None:
            t.close()
        ctx.close()
    _within(Px, c.P @ x, np.abs(c.P) @ np.abs(x), "level_transfer prolongate")
    assert np.array_equal(mg_transfer_apply(coarse, fine, "prolongate", x), Px)
    assert np.array_equal(mg_transfer_apply(coarse, fine, "prolongate_and_add", x, dst_f), dst_f + Px)
    assert np.array_equal(mg_transfer_apply(coarse, fine, "restrict_and_add", r, dst_c), dst_c + Ptr)
    rp, ci, va = pa.fill_injection_matrix(coarse, fine)
    got = np.zeros_like(c.P)
    got[np.repeat(np.arange(len(rp) - 1), fine.n_dofs_per_cell), ci] = va
    assert np.max(np.abs(got - c.P)) <= 1e-12 * np.max(np.abs(c.P))


@pytest.mark.parametrize("dim,cells,basis,p,diag_first", [(2, 8, "dgq", 2, True), (3, 4, "dgp", 3, False), (3, 2, "dgq", 4, True)])
def test_residual_against_the_values_read_back(dim, cells, basis, p, diag_first):
    """r = b - A x with A read back: per row within 1e-13 (sum_j |A_ij x_j| + |b_i|); the same bits twice"""
    pa = _pa()
    ah, fe = _handler(dim, cells, 1 if p == 4 else 2, basis, p)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(flat)
        ctx.assemble()
        A = _global_matrix(ctx, flat.arrays(), ah.n_dofs)
        rng = np.random.default_rng(11)
        x, b = rng.standard_normal(ah.n_dofs), rng.standard_normal(ah.n_dofs)
        d_x, d_b, d_r = dev.put(x), dev.put(b), dev.put(np.full(ah.n_dofs, np.nan))
        ctx.residual_device(d_b, d_x, d_r)
        ctx.synchronize()
        res = dev.get(d_r, ah.n_dofs)
        _within(res, b - A @ x, abs(A) @ np.abs(x) + np.abs(b), "residual")
        ctx.residual_device(d_b, d_x, d_r)
        ctx.synchronize()
        assert np.array_equal(dev.get(d_r, ah.n_dofs), res)
    finally:
        ctx.close()
        dev.free()


def test_state_and_argument_errors():
    pa = _pa()
    from polydeal_amd import _capi

    d = tc.build(("raw", "uneven")).desc
    ctx = pa.Context(0)
    dev = _Device()
    t = None
    try:
        # residual without a resident problem
        assert ctx.lib.pdh_residual_device(ctx.h, C.c_void_p(8), C.c_void_p(16), C.c_void_p(24)) == _capi.PDH_ESTATE
        # FE_AggloDGP has no support points
        bad = _capi.TransferDesc(dim=d.dim, degree=d.degree, basis=_capi.PDH_BASIS_AGGLODGP, fine_bbox=d.fine_bbox, coarse_bbox=d.coarse_bbox,
                                 fine_dof_offset=d.fine_dof_offset, coarse_dof_offset=d.coarse_dof_offset, parent=d.parent)
        with pytest.raises(pa.PdhError) as e:
            _capi.Transfer(ctx, bad)
        assert e.value.code == _capi.PDH_EUNSUPPORTED
        h = C.c_void_p()
        assert ctx.lib.pdh_transfer_create(ctx.h, None, C.byref(h)) == _capi.PDH_EINVAL and not h.value
        assert ctx.lib.pdh_transfer_create(None, C.byref(d.c), C.byref(h)) == _capi.PDH_EINVAL
        t = _capi.Transfer(ctx, d)
        lib = ctx.lib
        d_c, d_f = dev.put(np.zeros(d.n_coarse_rows)), dev.put(np.zeros(d.n_fine_rows))
        entries = (lib.pdh_prolongate_device, lib.pdh_prolongate_and_add_device, lib.pdh_restrict_device, lib.pdh_restrict_and_add_device)
        for fn in entries:
            assert fn(None, C.c_void_p(d_c), C.c_void_p(d_f)) == _capi.PDH_EINVAL
            assert fn(t.h, None, C.c_void_p(d_f)) == _capi.PDH_EINVAL
            assert fn(t.h, C.c_void_p(d_c), None) == _capi.PDH_EINVAL
            assert fn(t.h, C.c_void_p(d_f), C.c_void_p(d_f)) == _capi.PDH_EINVAL  # aliasing
            assert "overlap" in lib.pdh_last_error(ctx.h).decode()
        # the last entry of the fine vector inside the coarse range, either order of the arguments
        last = d_f + 8 * (d.n_fine_rows - 1)
        assert lib.pdh_prolongate_device(t.h, C.c_void_p(last), C.c_void_p(d_f)) == _capi.PDH_EINVAL
        assert lib.pdh_restrict_device(t.h, C.c_void_p(d_f), C.c_void_p(last)) == _capi.PDH_EINVAL
        hf = np.zeros(d.n_fine_rows)
        assert lib.pdh_prolongate(t.h, C.c_void_p(hf.ctypes.data), C.c_void_p(hf.ctypes.data)) == _capi.PDH_EINVAL
        assert lib.pdh_restrict(t.h, None, C.c_void_p(hf.ctypes.data)) == _capi.PDH_EINVAL
        # residual: null pointers and aliasing on a resident problem
        ah, fe = _handler(2, 8, 2, "dgq", 1)
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), True, True))
        ctx.assemble()
        v, w = dev.put(np.zeros(ah.n_dofs)), dev.put(np.zeros(ah.n_dofs))
        assert lib.pdh_residual_device(ctx.h, None, C.c_void_p(v), C.c_void_p(w)) == _capi.PDH_EINVAL
        assert lib.pdh_residual_device(ctx.h, C.c_void_p(v), C.c_void_p(w), C.c_void_p(w)) == _capi.PDH_EINVAL
        assert lib.pdh_residual_device(ctx.h, C.c_void_p(w), C.c_void_p(v), C.c_void_p(w)) == _capi.PDH_EINVAL
        # the transfer outlives a change of its context's problem
        assert np.max(np.abs(t.prolongate(np.ones(d.n_coarse_rows)) - 1.0)) <= 1e-14  # (the Lagrange polynomials sum to one)
    finally:
        if t is not None:
            t.close()
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# two-grid cycle composed of device calls
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", tc.TWOGRID_PAIRS, ids=lambda p: "%dD_lg%d_c%d_f%d_p%d" % p)
def test_two_grid_cycle_against_the_numpy_restatement(pair):
    """Both levels assembled on the device in two contexts (SipVariant.poisson_example, ascending layout), Chebyshev(block Jacobi,
    degree 3) smoothing, block-Jacobi CG as the coarse solver.  After each of three cycles from x = 0, x equals the restatement's
    (smoother: cheb_ref.apply with the device's lambda_lo / hi, P from the oracle, dense coarse solve) within
    |x|_inf (max(1e-13, 100 spread) + 10 cond_2(A_c) coarse_rel_tol).  The restatement's residual falls below 0.05 of its start within
    twelve cycles, and the device's after twelve, by residual_device, is within a factor of two of it."""
    pa = _pa()
    import twogrid_ref as tg
    from polydeal_amd.levels import level_transfer, two_grid_cycle_device

    dim, lg, bc, bf, p = pair
    coarse_rel_tol = 1e-13
    (coarse, fine), oracles = tc.handler_pair(dim, lg, bc, bf, p, 0.0)
    fe = pa.FE_DGQ(dim, p)
    n = fe.n_dofs_per_cell
    from oracle import polydeal_oracle as po
    P = po.fill_injection_matrix(*oracles)
    ctx_f, ctx_c = pa.Context(0), pa.Context(0)
    dev = _Device()
    t = None
    try:
        mats = []
        for ctx, ah in ((ctx_f, fine), (ctx_c, coarse)):
            flat = ah.flatten(pa.SipVariant.poisson_example(fe), False, True)
            ctx.set_problem(flat)
            ctx.assemble()
            mats.append(_global_matrix(ctx, flat.arrays(), ah.n_dofs))
        Af, Ac = mats
        info = ctx_f.setup_chebyshev("block_jacobi", degree=tc.TWOGRID_DEGREE)
        ctx_c.setup_preconditioner("block_jacobi")
        t = level_transfer(ctx_f, coarse, fine)
        lo, hi = info["lambda_lo"], info["lambda_hi"]
        cond = float(np.linalg.cond(Ac.toarray()))
        tol = tc.TWOGRID_TOL + 10.0 * cond * coarse_rel_tol
        b = tc.twogrid_rhs(fine.n_dofs)
        d_b, d_x, d_r = dev.put(b), dev.put(np.zeros(fine.n_dofs)), dev.put(np.zeros(fine.n_dofs))
        d_rc, d_ec = dev.put(np.zeros(coarse.n_dofs)), dev.put(np.zeros(coarse.n_dofs))
        x_ref = np.zeros(fine.n_dofs)
        for cyc in range(12):
            two_grid_cycle_device(ctx_f, ctx_c, t, d_b, d_x, d_r, d_rc, d_ec, coarse_rel_tol=coarse_rel_tol)
            ctx_f.synchronize()
            x_ref = tg.cycle(Af, Ac, n, P, lo, hi, tc.TWOGRID_DEGREE, b, x_ref)
            if cyc < 3:
                x = dev.get(d_x, fine.n_dofs)
                err = float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)))
                print("cycle %d: |x - x_ref|_inf / |x_ref|_inf = %.3e (bound %.3e, cond(A_c) = %.3e)" % (cyc + 1, err, tol, cond))
                assert err <= tol, (cyc, err, tol)
        ref_res = tg.residual_norm(Af, b, x_ref)
        assert ref_res < 0.05 * np.linalg.norm(b), (ref_res, float(np.linalg.norm(b)))
        ctx_f.residual_device(d_b, d_x, d_r)
        ctx_f.synchronize()
        dev_res = float(np.linalg.norm(dev.get(d_r, fine.n_dofs)))
        print("residual after 12 cycles: device %.6e restatement %.6e start %.6e" % (dev_res, ref_res, float(np.linalg.norm(b))))
        assert 0.5 * ref_res <= dev_res <= 2.0 * ref_res
    finally:
        if t is not None:
            t.close()
        ctx_f.close()
        ctx_c.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# the headline pair
# ---------------------------------------------------------------------------------------------------------------------------------
def test_headline_pair_interpolant_and_column_sums():
    """32^3 fine polytopes under 16^3 coarse ones, FE_DGQ(3), as a raw description (no handlers, no matrices): the prolongated coarse
    interpolant of the cubic equals the fine interpolant within 5e-13, and the restriction of the all-ones fine vector equals the column
    sums of P - from the 1-D matrices on the host - within 1e-13 sum_i |P_ij|."""
    pa = _pa()
    from polydeal_amd._capi import Transfer
    from oracle.polydeal_oracle import gauss_lobatto_nodes

    d = tc.headline_description()
    n, n1d = d.n, d.degree + 1
    unit = gauss_lobatto_nodes(d.degree)[tc.multi_index(3, d.degree)]  # [n][3]
    f = tc.poly(3, d.degree)

    def interpolant(bbox):
        x = bbox[:, None, 0, :] + unit[None] * (bbox[:, None, 1, :] - bbox[:, None, 0, :])  # [N][n][3]; offsets are contiguous
        return f(x.reshape(-1, 3))
    B = d.matrices_1d()  # [n_fine][3][i][j]
    digits = tc.multi_index(3, d.degree)

    def column_sums(M):  # sum over the rows of every block: prod_c sum_i M_c[i][j_c]
        s = M.sum(axis=2)  # [n_fine][3][j]
        per_child = s[:, 0, digits[:, 0]] * s[:, 1, digits[:, 1]] * s[:, 2, digits[:, 2]]  # [n_fine][n]
        out = np.zeros((d.n_coarse, n))
        np.add.at(out, d.parent, per_child)
        return out.ravel()
    ctx = pa.Context(0)
    t = None
    try:
        t = Transfer(ctx, d)
        err = t.prolongate(interpolant(d.coarse_bbox)) - interpolant(d.fine_bbox)
        print("headline interpolant: max error = %.3e" % float(np.max(np.abs(err))))
        assert np.max(np.abs(err)) < 5e-13
        got = t.restrict(np.ones(d.n_fine_rows))
        _within(got, column_sums(B), column_sums(np.abs(B)), "headline column sums")
        assert np.array_equal(t.restrict(np.ones(d.n_fine_rows)), got)
    finally:
        if t is not None:
            t.close()
        ctx.close()
    assert n1d == 4 and d.n_fine == 32768 and d.n_coarse == 4096
