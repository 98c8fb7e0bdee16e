"""p-transfers on the device (csrc/pdh_ptransfer.hip): prolongation and restriction between two degrees on the same polytopes against the
dense injection built from the oracle (tests/pmg_ref.py), on raw descriptions with permuted polytopes and gaps in the dof ranges: the four
device entries and the two host-pointer forms, the accumulating forms on a non-zero destination, untouched gap rows, the adjoint identity,
reproducibility, the argument errors and the refusal of the Galerkin product.  FE_DGQ within 1e-13 of the sum of absolute terms per row,
FE_AggloDGP to the bit.  Cases: tests/ptransfer_cases.py."""
import numpy as np
import pytest

import ptransfer_cases as pc
from test_gpu_solve import _Device

pytestmark = pytest.mark.gpu

TOL = 1e-13  # the bound of the h-transfer tests: per row, relative to the sum of the absolute terms


def _pa():
    import polydeal_amd as pa
    return pa


def _check(got, ref, scale, what, exact):
    if exact:
        assert np.array_equal(got, ref), what
        return
    worst = float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-300)))
    print("%s: max error / scale = %.3e" % (what, worst))
    assert not np.any(np.abs(got - ref) > TOL * scale), (what, worst)


@pytest.mark.parametrize("count", pc.RAW_COUNTS)
@pytest.mark.parametrize("case", pc.RAW_PAIRS, ids=pc.raw_id)
def test_ptransfer_against_the_dense_injection(case, count):
    pa = _pa()
    from polydeal_amd._capi import Transfer

    dim, basis, q, p = case
    d = pc.raw_desc(dim, basis, q, p, count)
    P = pc.raw_dense(dim, basis, q, p, d)
    aP = np.abs(P)
    exact = basis == "dgp"
    in_f, in_c = np.zeros(d.n_fine_rows, dtype=bool), np.zeros(d.n_coarse_rows, dtype=bool)  # rows that belong to a polytope
    for fo, co in zip(d.fine_dof_offset, d.coarse_dof_offset):
        in_f[fo:fo + d.n_f], in_c[co:co + d.n_c] = True, True
    assert in_f.sum() == count * d.n_f and in_c.sum() == count * d.n_c and not in_f.all() and not in_c.all()
    assert not np.any(aP[~in_f]) and not np.any(aP[:, ~in_c]) and np.all(aP.sum(axis=0)[in_c] > 0)
    rng = np.random.default_rng(11)
    x, r, y = rng.standard_normal(d.n_coarse_rows), rng.standard_normal(d.n_fine_rows), rng.standard_normal(d.n_fine_rows)
    old_f, old_c = rng.standard_normal(d.n_fine_rows), rng.standard_normal(d.n_coarse_rows)
    ctx = pa.Context(0)
    dev = _Device()
    t = None
    try:
        t = Transfer(ctx, d)  # no resident problem
        d_x, d_r, d_y = dev.put(x), dev.put(r), dev.put(y)

        def run(fn, src, start, n):
            dst = dev.put(start)
            fn(src, dst)
            ctx.synchronize()
            return dev.get(dst, n)
        # prolongation: the device entry leaves the gap rows as they were, the host-pointer form returns zeros there
        Px = run(t.prolongate_device, d_x, old_f, d.n_fine_rows)
        assert np.array_equal(Px[~in_f], old_f[~in_f])
        _check(Px[in_f], (P @ x)[in_f], (aP @ np.abs(x))[in_f], "prolongate", exact)
        assert np.array_equal(run(t.prolongate_device, d_x, old_f, d.n_fine_rows), Px)
        host = t.prolongate(x)
        assert np.array_equal(host[in_f], Px[in_f]) and not np.any(host[~in_f])
        # restriction
        Ptr = run(t.restrict_device, d_r, old_c, d.n_coarse_rows)
        assert np.array_equal(Ptr[~in_c], old_c[~in_c])
        _check(Ptr[in_c], (P.T @ r)[in_c], (aP.T @ np.abs(r))[in_c], "restrict", exact)
        assert np.array_equal(run(t.restrict_device, d_r, old_c, d.n_coarse_rows), Ptr)
        host = t.restrict(r)
        assert np.array_equal(host[in_c], Ptr[in_c]) and not np.any(host[~in_c])
        # accumulating forms on a non-zero destination, twice from the same start
        got_f = run(t.prolongate_and_add_device, d_x, old_f, d.n_fine_rows)
        got_c = run(t.restrict_and_add_device, d_r, old_c, d.n_coarse_rows)
        assert np.array_equal(run(t.prolongate_and_add_device, d_x, old_f, d.n_fine_rows), got_f)
        assert np.array_equal(run(t.restrict_and_add_device, d_r, old_c, d.n_coarse_rows), got_c)
        assert np.array_equal(got_f[~in_f], old_f[~in_f]) and np.array_equal(got_c[~in_c], old_c[~in_c])
        _check(got_f, old_f + P @ x, np.abs(old_f) + aP @ np.abs(x), "prolongate_and_add", exact)
        _check(got_c, old_c + P.T @ r, np.abs(old_c) + aP.T @ np.abs(r), "restrict_and_add", exact)
        if exact:  # the fine dofs outside the image of an index map are left alone
            image = aP.sum(axis=1) > 0
            assert image.sum() == count * d.n_c and np.array_equal(got_f[~image], old_f[~image])
        # adjoint identity from device results alone: y^T (P x) = (P^T y)^T x over the rows of the polytopes
        Pty = run(t.restrict_device, d_y, np.zeros(d.n_coarse_rows), d.n_coarse_rows)
        lhs, rhs = float(y[in_f] @ Px[in_f]), float(Pty @ x)
        bound = TOL * (float(np.abs(y) @ (aP @ np.abs(x))) + float((aP.T @ np.abs(y)) @ np.abs(x)))
        print("adjoint: |lhs - rhs| = %.3e, bound %.3e" % (abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound
    finally:
        if t is not None:
            t.close()
        ctx.close()
        dev.free()


@pytest.mark.parametrize("basis", ["dgq", "dgp"])
def test_argument_errors_and_the_galerkin_refusal(basis):
    pa = _pa()
    from polydeal_amd import _capi
    from polydeal_amd._capi import Transfer

    d = pc.raw_desc(3, basis, 1, 2, 7)
    ctx, coarse = pa.Context(0), pa.Context(0)
    dev = _Device()
    t = None
    try:
        t = Transfer(ctx, d)
        d_c, d_f = dev.put(np.zeros(d.n_coarse_rows)), dev.put(np.zeros(d.n_fine_rows + d.n_coarse_rows))
        for fn in (t.prolongate_device, t.prolongate_and_add_device):
            for args in ((0, d_f), (d_c, 0), (d_f + 8, d_f)):
                with pytest.raises(pa.PdhError) as ei:
                    fn(*args)
                assert ei.value.code == _capi.PDH_EINVAL
        for fn in (t.restrict_device, t.restrict_and_add_device):
            for args in ((0, d_c), (d_f, 0), (d_f, d_f + 8 * d.n_fine_rows - 8)):
                with pytest.raises(pa.PdhError) as ei:
                    fn(*args)
                assert ei.value.code == _capi.PDH_EINVAL
        with pytest.raises(pa.PdhError) as ei:
            t.galerkin_device(coarse)
        assert ei.value.code == _capi.PDH_EUNSUPPORTED and "re-assembled" in str(ei.value)
    finally:
        if t is not None:
            t.close()
        coarse.close()
        ctx.close()
        dev.free()
