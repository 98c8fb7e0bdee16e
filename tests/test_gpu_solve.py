"""Solving with the resident matrix (csrc/pdh_solve.hip): y = A x against scipy.sparse on the values copied back, the point / block
Jacobi preconditioners against NumPy, conjugate gradients against a direct solve and the NumPy restatement of examples/host_solver.h
(tests/pcg_ref.py), the reference's printed L2 error with the solve on the GPU, and the headline problem through closed-form
identities.  Every case asserts which set-up path and row kernel served it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import aniso_meshes as am
from device_buffers import Device as _Device
import golden_cases as gc
from pcg_ref import diag_blocks, pcg, preconditioner

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pa():
    import polydeal_amd as pa
    return pa


def _kernels(ctx, want=None):
    """(algorithm, row kernel) of the resident problem; AUTO reports 'rows' exactly when a row kernel is built"""
    used, kern = ctx.algorithm_in_use(), ctx.rows_kernel_in_use()
    assert (used == "rows") == (kern != "none"), (used, kern)
    if want is not None:
        assert (used, kern) == want, (used, kern, want)
    return used, kern


def _handler(dim, cells, per, basis, p, kind="block", grid=None):
    pa = _pa()
    if grid is None:
        lg = cells.bit_length() - 1
        grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg) if (1 << lg) == cells else \
            pa.BackgroundGrid.subdivided_hyper_cube(dim, cells, 0.0, 1.0)
    ah = pa.AgglomerationHandler(grid)
    if kind == "block":
        ah.define_block_agglomerates(per)
    else:
        ah.define_grown_agglomerates(per ** dim, seed=cells)
    fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah, fe


def _global_matrix(ctx, arr, n_rows):
    """scipy CSR of the owned rows as they stand in HBM, columns in the global numbering (col_offset mapped back)"""
    vals = ctx.values()
    rp = np.asarray(arr["rowptr"], dtype=np.int64)
    ci = np.asarray(arr["colind"], dtype=np.int64)[rp[0]:rp[-1]]
    if arr.get("col_offset") is not None:
        n = ctx.stats()["dofs_per_cell"]
        co, do = np.asarray(arr["col_offset"]), np.asarray(arr["dof_offset"])
        l2g = np.zeros(int(co.max()) + n, dtype=np.int64)
        for a in range(len(co)):
            l2g[co[a]:co[a] + n] = do[a] + np.arange(n)
        ci = l2g[ci]
    return sp.csr_matrix((vals, ci, rp - rp[0]), shape=(len(rp) - 1, n_rows))


def _check_vmult(ctx, A, x, what=""):
    """y = A x for a random x, per row within 1e-13 of sum_j |A_ij x_j|"""
    y = ctx.vmult(x)
    ref = A @ x
    scale = abs(A) @ np.abs(x)
    bad = np.abs(y - ref) > 1e-13 * scale
    assert not np.any(bad), (what, int(bad.sum()), float(np.max(np.abs(y - ref) / np.maximum(scale, 1e-300))))
    return y


VMULT_CASES = [
    # (dim, cells per axis, polytope block, basis, degree, agglomerates, expected (algorithm, row kernel) or None)
    (2, 8, 2, "dgq", 1, "block", None),         # n = 4
    (3, 4, 2, "dgq", 1, "block", None),         # n = 8
    (3, 4, 2, "dgp", 2, "block", None),         # n = 10
    (3, 4, 2, "dgp", 3, "block", None),         # n = 20
    (3, 4, 2, "dgq", 2, "block", None),         # n = 27
    (3, 4, 2, "dgq", 3, "block", ("rows", "terms")),  # n = 64
    (3, 2, 1, "dgq", 4, "block", ("direct", "none")),  # n = 125: 64 x 64 tiles, rows of up to 4 x 125 entries
    (2, 16, 2, "dgp", 2, "grown", None),        # METIS-like: many neighbours of several sizes
    (3, 6, 2, "dgq", 2, "grown", None),
    (3, 2, 2, "dgq", 3, "block", None),         # ONE polytope, no neighbours
]


@pytest.mark.parametrize("case", VMULT_CASES, ids=lambda c: "%dD_c%d_b%d_%s%d_%s" % c[:6])
@pytest.mark.parametrize("diag_first", [True, False])
def test_vmult_parity(case, diag_first):
    """pdh_vmult against scipy on the values copied back, both layouts; the device-pointer entry gives the same bits on pdh_stream();
    the second problem of a reused context equals a fresh context."""
    pa = _pa()
    dim, cells, per, basis, p, kind, want = case
    ah, fe = _handler(dim, cells, per, basis, p, kind)
    if case[1:3] == (2, 2):
        assert ah.n_agglomerates == 1
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    arr = flat.arrays()
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(flat)
        _kernels(ctx, want)
        ctx.assemble()
        A = _global_matrix(ctx, arr, ah.n_dofs)
        x = np.random.default_rng(1).standard_normal(ah.n_dofs)
        y = _check_vmult(ctx, A, x, case)
        d_x, d_y = dev.put(x), dev.put(np.full(ah.n_dofs, np.nan))
        ctx.vmult_device(d_x, d_y)
        ctx.synchronize()
        assert np.array_equal(dev.get(d_y, ah.n_dofs), y)
        # the same context on a second problem (the 2-D one of the first case, or a 3-D one), then this one again
        ah2, fe2 = _handler(3, 4, 2, "dgp", 1) if dim == 2 else _handler(2, 8, 2, "dgq", 2)
        flat2 = ah2.flatten(pa.SipVariant.poisson_example(fe2), True, True)
        ctx.set_problem(flat2)
        ctx.assemble()
        x2 = np.random.default_rng(2).standard_normal(ah2.n_dofs)
        _check_vmult(ctx, _global_matrix(ctx, flat2.arrays(), ah2.n_dofs), x2, "second problem")
        ctx.set_problem(flat)
        ctx.assemble()
        assert np.array_equal(ctx.vmult(x), y)
    finally:
        ctx.close()
        dev.free()


@pytest.mark.parametrize("name", ["rect124", "graded", "offset_far", "pinwheel", "rect2d", "rect124_2"])
def test_vmult_on_anisotropic_meshes(name):
    """aniso_meshes.py: non-cubic cells, graded axes, far origins, pinwheel agglomerates - described through the oracle."""
    pa = _pa()
    from flatten_oracle import flatten
    from oracle import polydeal_oracle as po

    dim = am.MESHES[name][0]
    p = 1 if name == "rect124_2" else 2
    fe = (po.FE_DGQ(3, 4) if name == "rect124_2" else po.FE_AggloDGP(dim, p))
    oah = am.oracle_handler(name, fe, fe.degree + 1)
    for diag_first in (True, False):
        kw = flatten(oah, po.variant_poisson_example(fe), diag_first=diag_first)
        ctx = pa.Context(0)
        try:
            ctx.set_problem(pa.Problem(**kw))
            used, _ = _kernels(ctx)
            if name == "rect124_2":
                assert used == "direct"
            ctx.assemble()
            A = _global_matrix(ctx, kw, oah.n_dofs)
            _check_vmult(ctx, A, np.random.default_rng(4).standard_normal(oah.n_dofs), (name, diag_first))
        finally:
            ctx.close()


def test_vmult_row_ranges_rank_local_epetra_and_cartesian():
    """A row range of a global description, rank-local descriptions (global x, owned rows out) in both layouts and in Epetra column
    order (col_offset: ghost blocks behind the owned ones), and the Cartesian description of the same problem."""
    pa = _pa()
    from polydeal_amd.partition import row_range

    ah, fe = _handler(3, 8, 2, "dgq", 2)
    var = pa.SipVariant.poisson_example(fe)
    n, nA, N = fe.n_dofs_per_cell, ah.n_agglomerates, ah.n_dofs
    x = np.random.default_rng(5).standard_normal(N)
    world = 3
    splits = [row_range(nA, n, r, world)[0] for r in range(world)] + [N]
    ctx = pa.Context(0)
    try:
        gflat = ah.flatten(var, True, True)
        ctx.set_problem(gflat)
        _kernels(ctx, ("rows", "terms"))
        ctx.assemble()
        y_all = _check_vmult(ctx, _global_matrix(ctx, gflat.arrays(), N), x, "global")
        for r in range(world):
            r0, r1 = splits[r], splits[r + 1]
            ctx.set_problem(gflat, r0, r1)
            _kernels(ctx)
            ctx.assemble()
            y = _check_vmult(ctx, _global_matrix(ctx, {"rowptr": gflat.arrays()["rowptr"][r0:r1 + 1],
                                                       "colind": gflat.arrays()["colind"]}, N), x, ("range", r))
            assert np.max(np.abs(y - y_all[r0:r1])) <= 1e-12 * np.max(np.abs(y_all))
            for diag_first, epetra in ((True, False), (False, False), (False, True)):
                loc = ah.flatten_local(var, r0, r1, diag_first, True, row_splits=splits, epetra_columns=epetra)
                assert loc.c.local == 1
                ctx.set_problem(loc, r0, r1)
                _kernels(ctx)
                ctx.assemble()
                la = loc.arrays()
                if epetra:
                    assert la.get("col_offset") is not None
                _check_vmult(ctx, _global_matrix(ctx, la, N), x, ("local", r, diag_first, epetra))
        cf = ah.flatten_cartesian(var, True, True)
        assert cf.cartesian
        ctx.set_problem(cf)
        _kernels(ctx, ("rows", "terms"))
        ctx.assemble()
        yc = _check_vmult(ctx, _global_matrix(ctx, cf.arrays(), N), x, "cartesian")
        assert np.max(np.abs(yc - y_all)) <= 1e-12 * np.max(np.abs(y_all))
    finally:
        ctx.close()


def test_vmult_refuses_overlap_and_needs_a_problem():
    pa = _pa()
    from polydeal_amd import _capi

    ctx = pa.Context(0)
    dev = _Device()
    try:
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_preconditioner("jacobi")
        assert e.value.code == _capi.PDH_ESTATE
        assert ctx.lib.pdh_vmult_device(ctx.h, C.c_void_p(8), C.c_void_p(16)) == _capi.PDH_ESTATE
        ah, fe = _handler(2, 8, 2, "dgq", 1)
        ctx.set_problem(ah.flatten(pa.SipVariant.poisson_example(fe), True, True))
        ctx.assemble()
        d = dev.put(np.zeros(ah.n_dofs))
        assert ctx.lib.pdh_vmult_device(ctx.h, C.c_void_p(d), C.c_void_p(d)) == _capi.PDH_EINVAL
        assert ctx.lib.pdh_vmult_device(ctx.h, C.c_void_p(d), C.c_void_p(d + 8 * (ah.n_dofs - 1))) == _capi.PDH_EINVAL
        h = np.zeros(ah.n_dofs)
        assert ctx.lib.pdh_vmult(ctx.h, h.ctypes.data, h.ctypes.data) == _capi.PDH_EINVAL
        assert "overlap" in ctx.lib.pdh_last_error(ctx.h).decode()
    finally:
        ctx.close()
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# preconditioners
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,cells,basis,p,diag_first", [(2, 8, "dgq", 2, True), (3, 4, "dgq", 3, False), (3, 4, "dgp", 3, True)])
def test_preconditioners_against_numpy(dim, cells, basis, p, diag_first):
    """z = P^-1 r: block Jacobi against numpy.linalg.solve per diagonal block, point Jacobi against r / diag(A); then the values
    change (re-assembly) and both the apply and the solver refuse the stale set-up."""
    pa = _pa()
    from polydeal_amd import _capi

    ah, fe = _handler(dim, cells, 2, basis, p)
    n = fe.n_dofs_per_cell
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(flat)
        _kernels(ctx)
        ctx.assemble()
        A = _global_matrix(ctx, flat.arrays(), ah.n_dofs)
        r = np.random.default_rng(6).standard_normal(ah.n_dofs)
        d_r, d_z = dev.put(r), dev.put(np.full(ah.n_dofs, np.nan))
        blocks = diag_blocks(A, n)
        ctx.setup_preconditioner("block_jacobi")
        ctx.precondition_device(d_r, d_z)
        ctx.synchronize()
        z = dev.get(d_z, ah.n_dofs).reshape(-1, n)
        want = np.linalg.solve(blocks, r.reshape(-1, n)[..., None])[..., 0]
        err = np.linalg.norm(z - want, axis=1) / np.linalg.norm(want, axis=1)
        assert err.max() <= 1e-11, float(err.max())
        ctx.setup_preconditioner(_capi.PDH_PREC_JACOBI)
        ctx.precondition_device(d_r, d_z)
        ctx.synchronize()
        zj = dev.get(d_z, ah.n_dofs)
        assert np.max(np.abs(zj - r / A.diagonal()) / np.abs(r / A.diagonal())) <= 1e-15
        ctx.setup_preconditioner("none")
        ctx.precondition_device(d_r, d_z)
        ctx.synchronize()
        assert np.array_equal(dev.get(d_z, ah.n_dofs), r)
        # stale set-up
        ctx.setup_preconditioner("block_jacobi")
        ctx.assemble_device()
        with pytest.raises(pa.PdhError) as e:
            ctx.precondition_device(d_r, d_z)
        assert e.value.code == _capi.PDH_ESTATE
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(r)
        assert e.value.code == _capi.PDH_ESTATE
        ctx.setup_preconditioner("block_jacobi")
        ctx.precondition_device(d_r, d_z)
        ctx.synchronize()
    finally:
        ctx.close()
        dev.free()


def test_preconditioner_failures():
    """A large negative penalty makes diagonal blocks indefinite: PDH_EINVAL naming the first such polytope (and the solver refuses
    the failed set-up); block Jacobi with more than 64 dofs per polytope: PDH_EUNSUPPORTED (point Jacobi works there)."""
    pa = _pa()
    from polydeal_amd import _capi

    ah, fe = _handler(2, 8, 2, "dgq", 2)
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), True, True)
    kw = {k: (None if v is None else np.array(v)) for k, v in flat.arrays().items()}
    c = flat.c
    kw.update(dim=c.dim, degree=c.degree, basis=c.basis, n_agg=c.n_agg, n_faces=c.n_faces, n_rows=c.n_rows, diag_first=1)
    kw["face_sigma"] = -1e3 * np.abs(kw["face_sigma"])
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw))
        _kernels(ctx)
        ctx.assemble()
        A = _global_matrix(ctx, kw, ah.n_dofs)
        blocks = diag_blocks(A, fe.n_dofs_per_cell)
        first = min(P for P in range(len(blocks)) if np.linalg.eigvalsh(blocks[P]).min() <= 0)
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_preconditioner("block_jacobi")
        assert e.value.code == _capi.PDH_EINVAL and ("polytope %d " % first) in str(e.value), (str(e.value), first)
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(np.ones(ah.n_dofs))
        assert e.value.code == _capi.PDH_ESTATE
        ah4, fe4 = _handler(3, 2, 1, "dgq", 4)
        ctx.set_problem(ah4.flatten(pa.SipVariant.poisson_example(fe4), True, True))
        _kernels(ctx, ("direct", "none"))
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.setup_preconditioner("block_jacobi")
        assert e.value.code == _capi.PDH_EUNSUPPORTED
        ctx.setup_preconditioner("jacobi")
        x, info = ctx.solve_cg(ctx.vmult(np.ones(ah4.n_dofs)), rel_tol=1e-12)
        assert np.max(np.abs(x - 1.0)) <= 1e-8, info
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# conjugate gradients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,cells,basis,p,diag_first", [(2, 16, "dgq", 1, True), (2, 8, "dgp", 3, False), (3, 4, "dgq", 2, True),
                                                         (3, 4, "dgp", 3, False)])
def test_cg_against_spsolve_and_the_host_loop(dim, cells, basis, p, diag_first):
    """Every preconditioner: x within 1e-9 of spsolve, iterations within one of tests/pcg_ref.py, residual within the bound; the
    device entry gives the same bits; x0 = exact takes no iteration, b = 0 gives x = 0; max_iter too small raises PDH_ENOCONV with
    the last iterate; two solves are bit-identical."""
    pa = _pa()
    from polydeal_amd import _capi

    ah, fe = _handler(dim, cells, 2, basis, p)
    n, N = fe.n_dofs_per_cell, ah.n_dofs
    flat = ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)
    ctx = pa.Context(0)
    dev = _Device()
    try:
        ctx.set_problem(flat)
        _kernels(ctx)
        ctx.assemble()
        A = _global_matrix(ctx, flat.arrays(), N)
        b = np.random.default_rng(8).standard_normal(N)
        ref = spla.spsolve(A.tocsc(), b)
        for kind in ("none", "jacobi", "block_jacobi"):
            ctx.setup_preconditioner(kind)
            x, info = ctx.solve_cg(b)
            _, it_ref, _ = pcg(A, b, preconditioner(A, n, kind))
            assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref), (kind, info)
            assert abs(info["iterations"] - it_ref) <= 1, (kind, info, it_ref)
            assert info["residual"] <= 1e-13 * np.linalg.norm(b) and info["residual0"] == pytest.approx(np.linalg.norm(b), rel=1e-13)
            x2, info2 = ctx.solve_cg(b)
            assert np.array_equal(x, x2) and info == info2, kind
            d_b, d_x = dev.put(b), dev.put(np.zeros(N))
            assert ctx.solve_cg_device(d_b, d_x) == info
            assert np.array_equal(dev.get(d_x, N), x)
        # exact initial guess: b = A x* by the same kernel, so r = 0 exactly
        xs = np.random.default_rng(9).standard_normal(N)
        x, info = ctx.solve_cg(ctx.vmult(xs), x0=xs)
        assert info["iterations"] == 0 and np.array_equal(x, xs)
        x, info = ctx.solve_cg(np.zeros(N))
        assert info["iterations"] == 0 and not np.any(x)
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(b, max_iter=3)
        assert e.value.code == _capi.PDH_ENOCONV and e.value.info["iterations"] == 3
        x3, it3, _ = pcg(A, b, preconditioner(A, n, "block_jacobi"), max_iter=3)
        assert np.linalg.norm(e.value.x - x3) <= 1e-10 * np.linalg.norm(x3)
        assert e.value.info["residual"] > 1e-13 * np.linalg.norm(b)
        # abs_tol: a loose absolute bound stops early
        _, info = ctx.solve_cg(b, abs_tol=1e-3 * np.linalg.norm(b), rel_tol=0.0)
        assert info["residual"] <= 1e-3 * np.linalg.norm(b) and info["iterations"] < it_ref
        # overlapping b and x
        assert ctx.lib.pdh_solve_cg_device(ctx.h, C.byref(_capi.pdh_cg_control(10, 1e-13, 0.0)), C.c_void_p(d_b), C.c_void_p(d_b),
                                           C.byref(_capi.pdh_cg_result())) == _capi.PDH_EINVAL
    finally:
        ctx.close()
        dev.free()


def test_cg_needs_all_rows_in_one_context():
    """Row ranges, rank-local descriptions and the ghost-block exchange: PDH_EUNSUPPORTED with a reason (vmult still works)."""
    pa = _pa()
    from polydeal_amd import _capi
    from polydeal_amd.partition import row_range

    ah, fe = _handler(3, 4, 2, "dgq", 1)
    var = pa.SipVariant.poisson_example(fe)
    n, nA, N = fe.n_dofs_per_cell, ah.n_agglomerates, ah.n_dofs
    splits = [row_range(nA, n, r, 2)[0] for r in range(2)] + [N]
    ctx = pa.Context(0)
    try:
        gflat = ah.flatten(var, True, True)
        for prob, rows in ((gflat, (0, splits[1])), (ah.flatten_local(var, splits[1], N, True, True, row_splits=splits), (splits[1], N))):
            ctx.set_problem(prob, *rows)
            _kernels(ctx)
            ctx.assemble()
            ctx.vmult(np.ones(N))
            with pytest.raises(pa.PdhError) as e:
                ctx.solve_cg(np.ones(N))
            assert e.value.code == _capi.PDH_EUNSUPPORTED and "all rows" in str(e.value)
        ctx.set_exchange_mode("ghost")
        ctx.set_problem(ah.flatten_local(var, 0, splits[1], True, True, row_splits=splits), 0, splits[1])
        _kernels(ctx)
        ctx.assemble()
        with pytest.raises(pa.PdhError) as e:
            ctx.solve_cg(np.ones(N))
        assert e.value.code == _capi.PDH_EUNSUPPORTED and "EXCHANGE_GHOST" in str(e.value)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's pipeline: 'L2 error:0.00647702' with matrix, right-hand side, SOLVE and evaluation on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_poisson_output_L2_error_solved_on_gpu():
    pa = _pa()
    from flatten_oracle import flatten
    from test_oracle_golden import _poisson_test_setup

    grid, ah, var = _poisson_test_setup()
    kw = flatten(ah, var, diag_first=False)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw))
        _kernels(ctx)
        ctx.assemble_device()
        pi = np.pi
        xq = kw["vq_x"]
        b = ctx.assemble_rhs(8 * pi * pi * np.sin(2 * pi * xq[0]) * np.sin(2 * pi * xq[1]), None)
        ctx.setup_preconditioner("block_jacobi")
        u, info = ctx.solve_cg(b)
        assert info["residual"] <= 1e-13 * np.linalg.norm(b)
        cells = [ah.get_agglomerate(P) for P in range(ah.n_agglomerates)]
        pt_ptr = np.concatenate([[0], np.cumsum([4 * len(c) for c in cells])])
        pts = np.concatenate([grid.vertices[c] for cs in cells for c in cs]).T
        uv = pa.interpolate_to_points(ctx, u, pt_ptr, pts).reshape(-1, 4)
    finally:
        ctx.close()
    V = np.stack([grid.vertices[c] for cs in cells for c in cs])
    mid = V.mean(axis=1)
    h2 = (V[:, 1, 0] - V[:, 0, 0]) * (V[:, 2, 1] - V[:, 0, 1])
    err = np.sqrt(np.sum(h2 * (uv.mean(axis=1) - np.sin(2 * pi * mid[:, 0]) * np.sin(2 * pi * mid[:, 1])) ** 2))
    assert "L2 error:" + gc.fmt(err) == gc.golden_lines("poisson.output")[0]


def test_poisson_example_device_solve():
    """examples/poisson --device-solve: the reference's case prints its L2 line, then the t3.msh p-convergence runs with the
    device solver and still converges (exit status 0)."""
    exe = os.path.join(ROOT, "examples", "poisson")
    assert os.path.exists(exe), "examples/poisson is built by __graft_entry__.build()"
    out = subprocess.run([exe, "--device-solve", os.path.join(ROOT, "tests", "golden", "t3.msh")], capture_output=True, text=True,
                         timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert gc.golden_lines("poisson.output")[0] in lines, out.stdout
    assert sum(l.startswith("Error (L2): ") for l in lines) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the headline problem
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diag_first", [True, False])
def test_headline_vmult_identities_and_block_jacobi_cg(diag_first):
    """64^3 cells, 32 768 polytopes, FE_DGQ(3), 914 M non-zeros: x^T (A x) gives the closed-form SIP identities (x = 1: sigma |dOmega|;
    x = nodal interpolant of x_c: -|Omega| + sigma int_dOmega x_c^2), sum vmult(1) equals the checksum's sum, and block-Jacobi CG on
    b = A x* recovers the interpolant x* of a smooth function to 1e-8."""
    pa = _pa()
    from oracle.polydeal_oracle import gauss_lobatto_nodes

    fe = pa.FE_DGQ(3, 3)
    grid = pa.BackgroundGrid.hyper_cube_refined(3, 0.0, 1.0, 6)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(2)
    ah.initialize_fe_values(4, 4)
    ah.distribute_agglomerated_dofs(fe)
    var = pa.SipVariant.poisson_example(fe)
    n, nA, p, N = fe.n_dofs_per_cell, ah.n_agglomerates, fe.degree, ah.n_dofs
    assert nA == 32768
    sigma = var.penalty_constant / ah.diameter(0)
    nodes = gauss_lobatto_nodes(p)
    blo, bhi = np.zeros((nA, 3)), np.zeros((nA, 3))
    off = np.zeros(nA, dtype=np.int64)
    for P in range(nA):
        blo[P], bhi[P] = ah.bbox(P)
        off[P] = ah.dof_indices(P)[0]
    idx = off[:, None] + np.arange(n)[None, :]
    digit = [(np.arange(n) // (p + 1) ** c) % (p + 1) for c in range(3)]
    xc = [blo[:, c:c + 1] + nodes[digit[c]][None, :] * (bhi - blo)[:, c:c + 1] for c in range(3)]  # nodal coordinates [nA][n]
    flat = ah.flatten(var, diag_first, False)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(flat)
        _kernels(ctx, ("rows", "terms") if diag_first else None)
        ctx.assemble_device()
        one = np.ones(N)
        y1 = ctx.vmult(one)
        q1 = math.fsum(y1)
        assert abs(q1 - 6.0 * sigma) <= 1e-11 * 6.0 * sigma, (q1, 6.0 * sigma)
        cs = ctx.checksum()
        assert abs(q1 - cs["sum"]) <= 1e-12 * abs(cs["sum"]), (q1, cs)
        for c in range(3):
            v = np.zeros(N)
            v[idx] = xc[c]
            qx = math.fsum(v * ctx.vmult(v))
            ex = -1.0 + sigma * (1.0 + 4.0 / 3.0)
            assert abs(qx - ex) <= 1e-11 * abs(ex), (c, qx, ex)
        xs = np.zeros(N)
        xs[idx] = np.sin(np.pi * xc[0]) * np.cos(0.5 * np.pi * xc[1]) * (1.0 + xc[2] ** 2)
        b = ctx.vmult(xs)
        ctx.setup_preconditioner("block_jacobi")
        x, info = ctx.solve_cg(b, rel_tol=1e-14)
        assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs), info
        assert 0 < info["iterations"] < 20000 and info["residual"] <= 1e-14 * np.linalg.norm(b)
    finally:
        ctx.close()
