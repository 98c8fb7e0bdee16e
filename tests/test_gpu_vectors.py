"""The vector kernels against the oracle, per polytope (tests/parity.py: assert_vector_parity): the right-hand side (k_rhs), u_h and
grad u_h at points (k_eval), the error sums of PolyUtils::compute_global_error (k_eval, error mode), basis values on boxes (k_shape)
and the checksum of the resident values (k_checksum).  They reach the caller's arrays through maps built at set-up (vq_src, ap_src,
the boundary range bd_rng of every slot, own_agg / own_row / by_agg), so every set-up path is paired with them: points, row ranges,
rank-local descriptions, the Cartesian description, a context that held other problems, and the device-pointer entry points.
Every case asserts which set-up path and row kernel served it."""
import ctypes as C
import math

import numpy as np
import pytest

import aniso_meshes as am
from flatten_oracle import flatten
from oracle import polydeal_oracle as po
from parity import assert_parity, assert_vector_parity, dof_segments, oracle_evaluate, point_segments, shape_value_scale

pytestmark = pytest.mark.gpu


def fn_f(x):
    return np.sin(2.0 * x[:, 0]) + x[:, 1] ** 2 + x[:, -1]


def fn_g(x):
    return 1.0 + x[:, 0] * x[:, 1] - 0.5 * x[:, -1]


def fn_exact(x):
    return np.sin(1.3 * x[:, 0]) * np.cos(0.7 * x[:, 1]) + x[:, -1] ** 2


def fn_exact_grad(x):
    g = np.zeros_like(x)
    g[:, 0] = 1.3 * np.cos(1.3 * x[:, 0]) * np.cos(0.7 * x[:, 1])
    g[:, 1] = -0.7 * np.sin(1.3 * x[:, 0]) * np.sin(0.7 * x[:, 1])
    g[:, -1] += 2 * x[:, -1]
    return g


def _fe(basis, dim, p):
    return (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)


def _oracle(grid, groups, fe, nq):
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    ah.initialize_fe_values(nq, nq)
    ah.distribute_agglomerated_dofs(fe)
    return ah


def _xy(a, dim):
    return np.asarray(a, dtype=np.float64).reshape(dim, -1)


def _kernels(ctx):
    """(algorithm, row kernel) of the resident problem, checked for consistency: AUTO reports 'rows' exactly when a row kernel is built"""
    used, kern = ctx.algorithm_in_use(), ctx.rows_kernel_in_use()
    assert (used == "rows") == (kern != "none"), (used, kern)
    return used, kern


def oracle_rhs(oah, var, key, f, g):
    """(rhs, its per-entry scale) of the oracle, kept on the handler (several descriptions of one problem are checked against it)"""
    cache = oah.__dict__.setdefault("_rhs_cache", {})
    k = (key, var.name)
    if k not in cache:
        cache[k] = (po.assemble_rhs(oah, var, f, g), po.assemble_rhs(oah, var, f, g, absolute=True))
    return cache[k]


def check_vectors(ctx, oah, var, arr, pts=None, rows=None, glob=None, u=None, what=""):
    """rhs (f and g, f only, g only, neither), u_h with and without gradients, and the error sums of the description `arr` resident in
    `ctx` (rows [r0, r1)) against the oracle handler `oah`, per polytope.  pts: the arrays that hold the points (a Cartesian description
    has none: those of the equivalent points description); glob: oracle polytope of every polytope of the description (rank-local).
    Contracts: g is read on boundary points only (NaN elsewhere changes nothing), f on owned polytopes only.  Returns the results."""
    dim, n = oah.grid.dim, oah.fe.n_dofs_per_cell
    pts = arr if pts is None else pts
    r0, r1 = (0, oah.n_dofs) if rows is None else rows
    off = np.asarray(arr["dof_offset"], dtype=np.int64)
    nA = len(off)
    glob = np.arange(nA) if glob is None else np.asarray(glob)
    owned = (off >= r0) & (off < r1)
    vq_ptr = np.asarray(arr["vq_ptr"], dtype=np.int64)
    vx, vw = _xy(pts["vq_x"], dim), np.asarray(pts["vq_w"], dtype=np.float64)
    vseg = point_segments(vq_ptr)
    fvol = fn_f(vx.T)
    if arr.get("fq_ptr") is not None and len(arr["fq_ptr"]) > 1:
        fx = _xy(pts["fq_x"], dim)
        bpt = np.asarray(arr["face_out"])[point_segments(arr["fq_ptr"])] < 0
        gb = np.where(bpt, fn_g(fx.T), 0.0)
        g_nan = np.where(bpt, gb, np.nan)
    else:
        gb = g_nan = np.zeros(0)
    seg = dof_segments(r1 - r0, n)
    out = {}
    for key, f, g in (("fg", fn_f, fn_g), ("f", fn_f, None), ("g", None, fn_g)):
        got = ctx.assemble_rhs(fvol if f else None, gb if g else None)
        ref, sc = oracle_rhs(oah, var, key, f, g)
        ref, sc = ref[r0:r1], sc[r0:r1]
        assert_vector_parity(got, ref, seg, sc, what="%s rhs %s" % (what, key))
        out["rhs_" + key] = got
    assert not np.any(ctx.assemble_rhs(None, None))
    # g_bdry is read on boundary faces only; f_vol on the owned polytopes only
    assert np.array_equal(ctx.assemble_rhs(fvol, g_nan), out["rhs_fg"]), what
    assert np.array_equal(ctx.assemble_rhs(np.where(owned[vseg], fvol, np.nan), gb), out["rhs_fg"]), what

    u = np.random.default_rng(7).standard_normal(oah.n_dofs) if u is None else u
    uh, gh = ctx.evaluate(u[r0:r1], vq_ptr, vx, want_grad=True)
    uv = ctx.evaluate(u[r0:r1], vq_ptr, vx)
    mask = owned[vseg]
    assert np.array_equal(uh[mask], uv[mask]) and not np.any(uh[~mask]) and not np.any(uv[~mask]) and not np.any(gh[:, ~mask])
    ev = [oracle_evaluate(oah, u, glob[a], vx[:, vq_ptr[a]:vq_ptr[a + 1]].T) for a in range(nA) if owned[a]]
    if ev:
        pseg = point_segments(np.concatenate([[0], np.cumsum([len(e[0]) for e in ev])]))
        assert_vector_parity(uh[mask], np.concatenate([e[0] for e in ev]), pseg, np.concatenate([e[2] for e in ev]), what=what + " u_h")
        assert_vector_parity(gh[:, mask].T, np.concatenate([e[1] for e in ev]), pseg, np.concatenate([e[3] for e in ev]),
                             what=what + " grad u_h")
    eu, eg = fn_exact(vx.T), fn_exact_grad(vx.T).T
    s = ctx.global_error_sums(u[r0:r1], vq_ptr, vx, vw, eu, eg)
    if ev:
        ru, rg = np.concatenate([e[0] for e in ev]), np.concatenate([e[1] for e in ev]).T
        rl2 = math.fsum(vw[mask] * (eu[mask] - ru) ** 2)
        rh1 = math.fsum(vw[mask] * np.sum((eg[:, mask] - rg) ** 2, axis=0))
        assert abs(s[0] - rl2) <= 1e-12 * rl2 and abs(s[1] - rh1) <= 1e-12 * rh1, (what, s, rl2, rh1)
    else:
        assert s == (0.0, 0.0)
    out.update(u=uh[mask], grad=gh[:, mask], err=s)
    return out


def run_oracle_case(oah, var, kw, rows=None):
    import polydeal_amd as pa

    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw), *(rows or ()))
        kern = _kernels(ctx)
        out = check_vectors(ctx, oah, var, kw, rows=rows)
    finally:
        ctx.close()
    return kern, out


def hull_spans_interior(kw):
    """Does some polytope list an interior face between two of its boundary faces?  Then its packed boundary points are not one run,
    and the boundary range of the rhs kernel (ensure_ap_src: the hull of the runs) covers interior points too."""
    fi, fo = np.asarray(kw["face_in"]), np.asarray(kw["face_out"])
    for a in range(len(kw["dof_offset"])):
        mine = np.nonzero((fi == a) | (fo == a))[0]
        bd = np.nonzero(fo[mine] < 0)[0]
        if len(bd) >= 2 and np.any(fo[mine[bd[0]:bd[-1]]] >= 0):
            return True
    return False


def split_boundary_face(kw, P):
    """The same problem with the boundary face of polytope P described as two faces, one listed second and one last: P's boundary points
    then form two runs with all of P's interior faces between them (a caller may describe a polytopal face in pieces).  An interior face
    comes first, so that the caller's face point 0 is an interior one (a kernel that reads g there and multiplies by 0 reads NaN)."""
    fi, fo, fp = np.asarray(kw["face_in"]), np.asarray(kw["face_out"]), np.asarray(kw["fq_ptr"])
    b = int(np.nonzero((fi == P) & (fo < 0))[0][0])
    s, e = int(fp[b]), int(fp[b + 1])
    m = s + (e - s) // 2
    x = int(np.nonzero(fo >= 0)[0][0])
    pieces = ([(x, fp[x], fp[x + 1]), (b, s, m)] + [(f, fp[f], fp[f + 1]) for f in range(len(fi)) if f not in (b, x)] + [(b, m, e)])
    idx = np.concatenate([np.arange(x, y) for _, x, y in pieces])
    faces = [f for f, _, _ in pieces]
    out = dict(kw)
    out.update(n_faces=len(faces), face_in=fi[faces], face_out=fo[faces], face_sigma=np.asarray(kw["face_sigma"])[faces],
               fq_ptr=np.concatenate([[0], np.cumsum([y - x for _, x, y in pieces])]),
               fq_x=np.asarray(kw["fq_x"])[:, idx], fq_n=np.asarray(kw["fq_n"])[:, idx], fq_w=np.asarray(kw["fq_w"])[idx],
               fq_w_out=np.asarray(kw["fq_w_out"])[idx])
    return out


def _size_ratio_handler(fe, r, lg):
    """one r^3-cell polytope among single cells (test_moment_form_with_neighbours_of_very_different_size)"""
    grid = po.hyper_cube_refined(3, 0.0, 1.0, lg)
    big = sorted(int(grid.ijk_to_cell[(i, j, k)]) for i in range(r) for j in range(r) for k in range(r))
    sb = set(big)
    return _oracle(grid, [big] + [[c] for c in range(grid.n_cells) if c not in sb], fe, fe.degree + 1)


def _random_handler(dim, lg, n_seeds, fe, seed, disc):
    from test_gpu_parity import random_agglomeration

    rng = np.random.default_rng(seed)
    grid = po.hyper_cube_refined(dim, -1.0, 1.0, lg).distort(0.2, seed=seed)
    groups = random_agglomeration(grid, n_seeds, rng, disc)
    return _oracle(grid, [groups[k] for k in rng.permutation(len(groups))], fe, fe.degree + 1)


def _mesh_case(name, basis, p):
    if name.startswith("ratio"):
        r = int(name[5:])
        return _size_ratio_handler(_fe(basis, 3, p), r, {2: 2, 4: 3, 8: 4}[r])
    if name in am.MESHES:
        fe = _fe(basis, am.MESHES[name][0], p)
        return am.oracle_handler(name, fe, p + 1)
    if name.startswith("random"):
        dim = int(name[6])
        return _random_handler(dim, 3 if dim == 2 else 2, 9, _fe(basis, dim, p), 21 + dim, True)
    if name.startswith("single"):
        dim = int(name[6])
        grid = po.hyper_cube_refined(dim, 0.0, 1.0, 2 if dim == 2 else 1)
        return _oracle(grid, [list(range(grid.n_cells))], _fe(basis, dim, p), p + 1)
    raise KeyError(name)


# (mesh, basis, degree, row kernel the planner grants: tests/test_anisotropic_cpu.py pins the selection on these meshes)
MESH_CASES = [
    ("ratio2", "dgq", 3), ("ratio4", "dgq", 3), ("ratio8", "dgq", 1), ("ratio4", "dgp", 2),
    ("graded", "dgq", 3), ("graded", "dgp", 3), ("offset_far", "dgq", 2), ("offset_far", "dgq", 3), ("pinwheel", "dgp", 3),
    ("pinwheel", "dgq", 3), ("random2", "dgq", 2), ("random3", "dgq", 3), ("random3", "dgp", 2), ("single2", "dgp", 4),
    ("single3", "dgq", 3), ("single3", "dgp", 2), ("rect2d", "dgq", 3), ("offset2d", "dgp", 5),
]


@pytest.mark.parametrize("mesh,basis,p", MESH_CASES)
def test_vectors_on_meshes_with_small_polytopes(mesh, basis, p):
    """Polytopes of very different size, graded and far-offset cells, slabs, random (disconnected) agglomerates, one polytope, 2-D: rhs,
    u_h, grad u_h per polytope and the error sums, globally and on the second half of the rows."""
    oah = _mesh_case(mesh, basis, p)
    var = po.variant_poisson_example(oah.fe)
    kw = flatten(oah, var)
    assert not hull_spans_interior(kw)  # the oracle describes all boundary sub-faces of a polytope as one face
    if oah.grid.dim == 3:
        rt, wt, rr, wr = am.kernel_selection(kw)
        want = "terms" if rt == 1 else ("rows" if rr == 1 else "none")
    else:
        want = "none"
    (used, kern), _ = run_oracle_case(oah, var, kw)
    assert (kern if kern in ("terms", "none") else "rows") == want, (kern, want)
    if oah.grid.dim == 2:
        assert used == "direct"
    n = oah.fe.n_dofs_per_cell
    r0 = (oah.n_agglomerates // 2) * n
    if r0:
        run_oracle_case(oah, var, kw, rows=(r0, oah.n_dofs))


@pytest.mark.parametrize("dim,basis,p", [(3, "dgq", 2), (3, "dgq", 3), (3, "dgp", 3), (2, "dgq", 2)])
def test_boundary_runs_separated_by_interior_faces(dim, basis, p):
    """A polytope whose boundary is described as two faces, listed first and last: its packed boundary points are two runs with interior
    points between them, and the rhs kernel's boundary range spans those.  The interior points there carry no datum: g = NaN at every
    interior-face point changes nothing, and rhs and matrix equal the oracle's."""
    import polydeal_amd as pa

    oah = _random_handler(dim, 3 if dim == 2 else 2, 9, _fe(basis, dim, p), 31, True)
    var = po.variant_poisson_example(oah.fe)
    kw = flatten(oah, var)
    P = max(a for a in range(oah.n_agglomerates) if np.any((np.asarray(kw["face_in"]) == a) & (np.asarray(kw["face_out"]) < 0)))
    sk = split_boundary_face(kw, P)
    assert hull_spans_interior(sk) and not hull_spans_interior(kw)
    rp, ci, ref = po.assemble_csr(oah, var)
    for rows in (None, (oah.dof_offset[P], oah.n_dofs)):
        ctx = pa.Context(0)
        try:
            ctx.set_problem(pa.Problem(**sk), *(rows or ()))
            _kernels(ctx)
            if rows is None:
                assert_parity(ctx.assemble(), ref, rp, ci, oah.fe.n_dofs_per_cell, what="split boundary face")
            check_vectors(ctx, oah, var, sk, rows=rows, what="split boundary face")
        finally:
            ctx.close()


ELEMENTS = ([(2, "dgq", p) for p in range(8)] + [(2, "dgp", p) for p in range(1, 8)] +
            [(3, "dgq", p) for p in range(8)] + [(3, "dgp", p) for p in range(1, 8)])


@pytest.mark.parametrize("dim,basis,p", ELEMENTS)
def test_every_instantiated_element(dim, basis, p):
    """k_rhs, k_eval (value, value + gradient, error sums) and k_shape for every (dim, basis, degree) instantiated: 3-D FE_DGQ(3) takes
    the MFMA volume loop of k_rhs, FE_AggloDGP(3) its subset of the same 64 sums; n > 64 runs in several waves per polytope."""
    import polydeal_amd as pa

    fe = _fe(basis, dim, p)
    grid = po.hyper_cube_refined(dim, 0.0, 1.0, 2 if dim == 2 else 1).distort(0.1, seed=p)
    if dim == 2:
        groups = po.block_agglomerates(grid, 2)
    elif fe.n_dofs_per_cell > 64:  # a 2 x 2 x 1 polytope beside four single cells
        groups = [[0, 1, 2, 3]] + [[c] for c in range(4, 8)]
    else:
        groups = po.block_agglomerates(grid, 1)
    oah = _oracle(grid, groups, fe, p + 1)
    var = po.variant_poisson_example(fe) if p else po.SipVariant("p0", 10.0, "id", "diameter_in")
    kw = flatten(oah, var)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw))
        _kernels(ctx)
        check_vectors(ctx, oah, var, kw, what="%dD %s(%d)" % (dim, fe.name, p))
        check_shape_values(ctx, oah, *_sub_cell_and_random_points(oah, np.random.default_rng(p)))
    finally:
        ctx.close()


def _sub_cell_and_random_points(oah, rng, counts=(0, 1, 64, 65)):
    """Per polytope: the vertices of its cells (centred box coordinate exactly -0.5 / +0.5 on the box faces, as
    interpolate_to_fine_grid evaluates) followed by random points of its box; the first polytopes get exactly `counts` points so that
    the chunks of 64 points end everywhere."""
    dim = oah.grid.dim
    pts = []
    for P in range(oah.n_agglomerates):
        lo, hi = oah.bboxes[P]
        V = np.concatenate([oah.grid.vertices[c] for c in oah.get_agglomerate(P)])
        R = lo + rng.random((40, dim)) * (hi - lo)
        x = np.concatenate([V, R])
        if P < len(counts):
            k = counts[P]
            x = np.concatenate([x] * (k // len(x) + 1))[:k]
        pts.append(x)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int64)
    return ptr, np.concatenate(pts).T.copy()


def check_shape_values(ctx, oah, ptr, X, boxes=None):
    """pdh_shape_values of the handler's element on its bounding boxes at the points X [dim][N] (ptr: per box) against the oracle per
    (box, function); and pdh_evaluate at the same points per polytope."""
    fe, dim = oah.fe, oah.grid.dim
    nb = oah.n_agglomerates
    bbox = np.array([np.concatenate(oah.bboxes[P]) for P in range(nb)])
    got = ctx.shape_values(dim, fe.degree, fe.basis_id, bbox, ptr, X)
    unit = [oah.real_to_unit(P, X[:, ptr[P]:ptr[P + 1]].T) for P in range(nb)]
    ref = np.concatenate([fe.shape(t)[0] for t in unit])
    sc = np.concatenate([shape_value_scale(fe, t) for t in unit])
    assert got.shape == ref.shape
    # per (box, function): the largest |phi_j| over the box's points where the 1-D factors have no root there, else the terms' scale
    assert_vector_parity(got, ref, point_segments(ptr), np.maximum(np.abs(ref), sc), what="shape values %s(%d)" % (fe.name, fe.degree))
    return got


@pytest.mark.parametrize("dim,basis,p", [(3, "dgq", 3), (3, "dgp", 3), (3, "dgq", 1), (2, "dgq", 4), (3, "dgq", 5), (2, "dgp", 7)])
def test_sub_cell_vertices_random_points_and_chunk_edges(dim, basis, p):
    """pdh_evaluate and pdh_shape_values at the points they are used with beyond the quadrature: every sub-cell vertex (on the box faces the
    centred coordinate is exactly +-0.5) and random interior points; polytopes with 0, 1, 64 and 65 points."""
    import polydeal_amd as pa

    fe = _fe(basis, dim, p)
    grid = po.hyper_cube_refined(dim, 0.0, 1.0, 2).distort(0.1, seed=4)
    oah = _oracle(grid, po.block_agglomerates(grid, 2), fe, p + 1)
    ptr, X = _sub_cell_and_random_points(oah, np.random.default_rng(9))
    assert list(np.diff(ptr)[:4]) == [0, 1, 64, 65]
    var = po.variant_poisson_example(fe)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**flatten(oah, var)))
        check_shape_values(ctx, oah, ptr, X)
        u = np.random.default_rng(3).standard_normal(oah.n_dofs)
        uh, gh = ctx.evaluate(u, ptr, X, want_grad=True)
        ev = [oracle_evaluate(oah, u, P, X[:, ptr[P]:ptr[P + 1]].T) for P in range(oah.n_agglomerates)]
        seg = point_segments(ptr)
        assert_vector_parity(uh, np.concatenate([e[0] for e in ev]), seg, np.concatenate([e[2] for e in ev]), what="u_h")
        assert_vector_parity(gh.T, np.concatenate([e[1] for e in ev]), seg, np.concatenate([e[3] for e in ev]), what="grad u_h")
        assert np.array_equal(ctx.evaluate(u, ptr, X), uh)
    finally:
        ctx.close()


def test_shape_values_cache_follows_the_element():
    """pdh_shape_values caches the multi-index table of the last (dim, degree, basis): called in a row on one context with different
    elements, every result matches the oracle (and a fresh context's, bit for bit)."""
    import polydeal_amd as pa

    seq = [(3, "dgq", 3), (3, "dgp", 3), (2, "dgp", 3), (2, "dgq", 3), (3, "dgq", 7), (3, "dgp", 7), (3, "dgq", 3), (2, "dgq", 0)]
    ctx = pa.Context(0)
    try:
        for dim, basis, p in seq:
            fe = _fe(basis, dim, p)
            grid = po.hyper_cube_refined(dim, 0.0, 1.0, 1 if dim == 3 else 2)
            oah = _oracle(grid, po.block_agglomerates(grid, 1), fe, 1)
            ptr, X = _sub_cell_and_random_points(oah, np.random.default_rng(p + dim), counts=(3, 0, 70))
            got = check_shape_values(ctx, oah, ptr, X)
            fresh = pa.Context(0)
            try:
                bbox = np.array([np.concatenate(oah.bboxes[P]) for P in range(oah.n_agglomerates)])
                assert np.array_equal(fresh.shape_values(dim, p, fe.basis_id, bbox, ptr, X), got)
            finally:
                fresh.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Set-up paths: points (global, row range), rank-local points, Cartesian (global, rank-local) - the product mirror describes the
# problem, the oracle rebuilds the same agglomerates
# ---------------------------------------------------------------------------------------------------------------------------------
def _mirror_problem(cells, per, basis, p, kind="block"):
    import polydeal_amd as pa

    grid = pa.BackgroundGrid.subdivided_hyper_cube(3, cells, 0.0, 1.0)
    ah = pa.AgglomerationHandler(grid)
    if kind == "block":
        ah.define_block_agglomerates(per)
    else:
        ah.define_grown_agglomerates(per, seed=cells)
    fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(3, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    og = po.subdivided_hyper_cube(3, cells, 0.0, 1.0)
    groups = []
    for P in range(ah.n_agglomerates):
        c_ = ah.get_agglomerate(P)
        groups.append([c_[-1]] + c_[:-1])
    oah = _oracle(og, groups, _fe(basis, 3, p), p + 1)
    return ah, fe, oah


@pytest.mark.parametrize("cells,per,kind,basis,p", [(4, 2, "block", "dgq", 3), (6, 6, "grown", "dgq", 2), (4, 2, "block", "dgp", 3),
                                                    (6, 6, "grown", "dgp", 1)])
def test_every_set_up_path(cells, per, kind, basis, p):
    """rhs, u_h and the error sums after every set-up path, per polytope against the oracle: a points description (global and on a row
    range), rank-local points descriptions, the Cartesian description (global and rank-local; f and g sampled at the points of the
    equivalent points description).  Cartesian and points results agree to 1e-13."""
    import polydeal_amd as pa
    from polydeal_amd.partition import row_range

    ah, fe, oah = _mirror_problem(cells, per, basis, p, kind)
    var = pa.SipVariant.poisson_example(fe)
    ovar = po.variant_poisson_example(oah.fe)
    n, nA = fe.n_dofs_per_cell, ah.n_agglomerates
    splits = [row_range(nA, n, r, 2)[0] for r in range(2)] + [ah.n_dofs]
    pf = ah.flatten(var, True, True)
    cf = ah.flatten_cartesian(var, True, True)
    assert cf.cartesian and cf.c.vq_x is None and not pf.cartesian
    pa_, ca = pf.arrays(), cf.arrays()
    for key in ("dof_offset", "vq_ptr", "face_in", "face_out", "fq_ptr", "face_sigma"):
        assert np.array_equal(ca[key], pa_[key]), key
    res = {}
    for name, view, arr, pts, rows, glob in (
            ("points", pf, pa_, None, None, None), ("points rows", pf, pa_, None, (splits[1], splits[2]), None),
            ("cartesian", cf, ca, pa_, None, None)):
        ctx = pa.Context(0)
        try:
            ctx.set_problem(view, *(rows or ()))
            used, kern = _kernels(ctx)
            if name == "cartesian":
                assert used == "rows" and kern == "terms"
            res[name] = check_vectors(ctx, oah, ovar, arr, pts=pts, rows=rows, glob=glob, what=name)
        finally:
            ctx.close()
    for r in range(2):
        r0, r1 = splits[r], splits[r + 1]
        loc = ah.flatten_local(var, r0, r1, True, True, row_splits=splits)
        cloc = ah.flatten_cartesian(var, True, False, r0, r1, splits)
        la, cla = loc.arrays(), cloc.arrays()
        assert loc.c.local == 1 and cloc.cartesian
        for key in ("dof_offset", "vq_ptr", "fq_ptr", "face_in", "face_out"):
            assert np.array_equal(la[key], cla[key]), key
        glob = loc.local_of()
        for name, view, pts in (("rank-local points", loc, None), ("rank-local cartesian", cloc, la)):
            ctx = pa.Context(0)
            try:
                ctx.set_problem(view, r0, r1)
                used, kern = _kernels(ctx)
                if "cartesian" in name:
                    assert used == "rows" and kern == "terms"
                res["%s %d" % (name, r)] = check_vectors(ctx, oah, ovar, la if pts is None else cla, pts=pts, rows=(r0, r1), glob=glob,
                                                         what="%s %d" % (name, r))
            finally:
                ctx.close()
        a, b = res["rank-local points %d" % r], res["rank-local cartesian %d" % r]
        for key in ("rhs_fg", "rhs_f", "rhs_g", "u"):
            assert np.max(np.abs(a[key] - b[key])) <= 1e-13 * np.max(np.abs(a[key])), (r, key)
    a, b = res["points"], res["cartesian"]
    for key in ("rhs_fg", "rhs_f", "rhs_g", "u", "grad"):
        assert np.max(np.abs(a[key] - b[key])) <= 1e-13 * np.max(np.abs(a[key])), key
    assert abs(a["err"][0] - b["err"][0]) <= 1e-13 * a["err"][0] and abs(a["err"][1] - b["err"][1]) <= 1e-13 * a["err"][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# Device-pointer entry points: bit-identical to the host entry points on the same problem
# ---------------------------------------------------------------------------------------------------------------------------------
class _Device:
    """Device buffers through the HIP runtime the library runs on (the way Context.poison_values writes), freed by free()."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        self.bufs.append(p.value)
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), a.nbytes, 1) == 0
        return p.value

    def get(self, ptr, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(C.c_void_p(p))
        self.bufs = []


@pytest.mark.parametrize("basis,p,rows", [("dgq", 3, False), ("dgq", 3, True), ("dgp", 2, True), ("dgq", 5, False)])
def test_device_pointer_entry_points(basis, p, rows):
    """pdh_assemble_rhs_device (with and without each of d_f_vol / d_g_bdry), pdh_evaluate_device (with and without gradients),
    pdh_global_error_device and pdh_shape_values_device give what their host entry points give, bit for bit; on a row range the outputs
    of polytopes not owned (pre-filled with NaN) are left alone."""
    import polydeal_amd as pa

    fe = _fe(basis, 3, p)
    grid = po.hyper_cube_refined(3, 0.0, 1.0, 2 if p <= 3 else 1).distort(0.1, seed=2)
    oah = _oracle(grid, po.block_agglomerates(grid, 2 if p <= 3 else 1), fe, p + 1)
    var = po.variant_poisson_example(fe)
    kw = flatten(oah, var)
    n = fe.n_dofs_per_cell
    r0, r1 = ((oah.n_agglomerates // 3) * n, oah.n_dofs) if rows else (0, oah.n_dofs)
    dev = _Device()
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw), r0, r1)
        _kernels(ctx)
        vx, fx = np.asarray(kw["vq_x"]), np.asarray(kw["fq_x"])
        fv, gb = fn_f(vx.T), fn_g(fx.T)
        d_f, d_g = dev.put(fv), dev.put(gb)
        for use_f, use_g in ((1, 1), (1, 0), (0, 1), (0, 0)):
            want = ctx.assemble_rhs(fv if use_f else None, gb if use_g else None)
            d_rhs = dev.put(np.full(r1 - r0, np.nan))
            ctx.assemble_rhs_device(d_f if use_f else None, d_g if use_g else None, d_rhs)
            ctx.synchronize()
            assert np.array_equal(dev.get(d_rhs, r1 - r0), want), (use_f, use_g)
        u = np.random.default_rng(1).standard_normal(oah.n_dofs)[r0:r1]
        ptr, N = np.asarray(kw["vq_ptr"], dtype=np.int64), vx.shape[1]
        d_sol, d_ptr, d_pts = dev.put(u), dev.put(ptr), dev.put(vx)
        owned = ctx.owned_point_mask(ptr)
        assert np.any(owned) and (np.any(~owned) == rows)
        for grad in (False, True):
            want = ctx.evaluate(u, ptr, vx, want_grad=grad)
            d_out = dev.put(np.full(N, np.nan))
            d_gr = dev.put(np.full((3, N), np.nan)) if grad else None
            ctx.evaluate_device(d_sol, d_ptr, d_pts, N, d_out, d_gr)
            ctx.synchronize()
            hu = dev.get(d_out, N)
            wu = want[0] if grad else want
            assert np.array_equal(hu[owned], wu[owned]) and np.all(np.isnan(hu[~owned])), grad
            if grad:
                hg = dev.get(d_gr, (3, N))
                assert np.array_equal(hg[:, owned], want[1][:, owned]) and np.all(np.isnan(hg[:, ~owned]))
        w, eu, eg = np.asarray(kw["vq_w"]), fn_exact(vx.T), fn_exact_grad(vx.T).T
        want = ctx.global_error_sums(u, ptr, vx, w, eu, eg)
        got = ctx.global_error_sums_device(d_sol, d_ptr, d_pts, N, dev.put(w), dev.put(eu), dev.put(eg))
        assert got == want and want[0] > 0
        bptr, X = _sub_cell_and_random_points(oah, np.random.default_rng(2))
        bbox = np.array([np.concatenate(oah.bboxes[P]) for P in range(oah.n_agglomerates)])
        want = ctx.shape_values(3, p, fe.basis_id, bbox, bptr, X)
        d_vals = dev.put(np.full((X.shape[1], n), np.nan))
        rc = ctx.lib.pdh_shape_values_device(ctx.h, 3, p, fe.basis_id, len(bbox), C.c_void_p(dev.put(bbox)), C.c_void_p(dev.put(bptr)),
                                             C.c_void_p(dev.put(X)), X.shape[1], C.c_void_p(d_vals))
        assert rc == 0
        ctx.synchronize()
        assert np.array_equal(dev.get(d_vals, (X.shape[1], n)), want)
    finally:
        ctx.close()
        dev.free()


def test_context_reuse_is_bit_identical_to_fresh_contexts():
    """One context through: 3-D FE_DGQ(3) points (rhs, u_h, shape values); a larger 2-D FE_AggloDGP problem with more points; the first
    problem described Cartesian; the first problem on a row range.  Every result equals a fresh context's bit for bit (the per-context
    caches: the rhs maps of ensure_ap_src, the scratch buffers, the shape-value table)."""
    import polydeal_amd as pa

    ah3, fe3, oah3 = _mirror_problem(4, 2, "dgq", 3)
    var3 = pa.SipVariant.poisson_example(fe3)
    pf = ah3.flatten(var3, True, True)
    cf = ah3.flatten_cartesian(var3, True, True)
    a3 = pf.arrays()
    grid2 = po.hyper_cube_refined(2, 0.0, 1.0, 5).distort(0.1, seed=1)
    fe2 = po.FE_AggloDGP(2, 4)
    oah2 = _oracle(grid2, po.block_agglomerates(grid2, 2), fe2, 5)
    kw2 = flatten(oah2, po.variant_poisson_example(fe2))
    n3 = fe3.n_dofs_per_cell
    half = (ah3.n_agglomerates // 2) * n3

    def work(ctx, view, arr, dim, oah, rows, shape=True):
        r0, r1 = rows or (0, oah.n_dofs)
        ctx.set_problem(view, *(rows or ()))
        vx = _xy(arr["vq_x"], dim)
        out = [ctx.assemble_rhs(fn_f(vx.T), fn_g(_xy(arr["fq_x"], dim).T))]
        u = np.random.default_rng(dim).standard_normal(oah.n_dofs)[r0:r1]
        out += list(ctx.evaluate(u, arr["vq_ptr"], vx, want_grad=True))
        if shape:
            ptr, X = _sub_cell_and_random_points(oah, np.random.default_rng(dim))
            bbox = np.array([np.concatenate(oah.bboxes[P]) for P in range(oah.n_agglomerates)])
            out.append(ctx.shape_values(dim, oah.fe.degree, oah.fe.basis_id, bbox, ptr, X))
        return out

    steps = [(pf, a3, 3, oah3, None, True), (pa.Problem(**kw2), kw2, 2, oah2, None, True), (cf, a3, 3, oah3, None, False),
             (pf, a3, 3, oah3, (half, ah3.n_dofs), False)]
    ctx = pa.Context(0)
    try:
        for k, (view, arr, dim, oah, rows, shape) in enumerate(steps):
            got = work(ctx, view, arr, dim, oah, rows, shape)
            fresh = pa.Context(0)
            try:
                want = work(fresh, view, arr, dim, oah, rows, shape)
            finally:
                fresh.close()
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g, w), k
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# pdh_values_checksum (bench's validity line for the headline matrix)
# ---------------------------------------------------------------------------------------------------------------------------------
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _check_checksum(ctx, vals):
    cs = ctx.checksum()
    fin = np.isfinite(vals)
    a = vals[fin]
    abs_sum = math.fsum(np.abs(a))
    assert cs["non_finite"] == int((~fin).sum())
    assert abs(cs["sum"] - math.fsum(a)) <= 1e-13 * abs_sum, (cs, math.fsum(a))
    assert abs(cs["abs_sum"] - abs_sum) <= 1e-13 * abs_sum
    assert cs["max_abs"] == (float(np.max(np.abs(a))) if a.size else 0.0)
    return cs


def _checksum_problem(dim, lg, b, basis, p, vname, rows_frac=None):
    import polydeal_amd as pa

    fe = _fe(basis, dim, p)
    grid = po.hyper_cube_refined(dim, 0.0, 1.0, lg)
    oah = _oracle(grid, po.block_agglomerates(grid, b), fe, p + 1)
    var = {"poisson": po.variant_poisson_example(fe), "dr": po.variant_diffusion_reaction(fe),
           "p0": po.SipVariant("p0", 10.0, "id", "diameter_in")}[vname]
    kw = flatten(oah, var)
    n = fe.n_dofs_per_cell
    rows = None if rows_frac is None else ((int(oah.n_agglomerates * rows_frac)) * n, oah.n_dofs)
    return oah, var, kw, rows


@pytest.mark.parametrize("dim,lg,b,basis,p,vname,rows_frac", [
    (3, 0, 1, "dgq", 0, "p0", None),          # a single value
    (2, 2, 2, "dgq", 1, "poisson", None),     # 192 values: not a multiple of 256
    (3, 3, 2, "dgq", 3, "poisson", None),     # > 2048 x 256 values: the grid-stride loop wraps
    (3, 3, 2, "dgq", 3, "dr", 0.5),           # rank-local row range: the owned rows only
    (2, 3, 2, "dgq", 2, "dr", None),
    (3, 2, 2, "dgq", 2, "poisson", 0.25),
])
def test_values_checksum(dim, lg, b, basis, p, vname, rows_frac):
    """pdh_values_checksum against the values copied back (sum / abs_sum to 1e-13 of math.fsum(|v|), max_abs exact, no non-finite), and
    for FE_DGQ the closed form bench relies on, per owned polytope P: (A 1) summed over P's rows = sigma |dP n dOmega| + c |P| (the
    basis is a partition of unity; against the oracle matrix too).  Then poisoned values, and NaN / +-Inf / large values written at
    known positions through the device pointer: the count is exact and the sums leave out exactly those entries."""
    import polydeal_amd as pa

    oah, var, kw, rows = _checksum_problem(dim, lg, b, basis, p, vname, rows_frac)
    r0, r1 = rows or (0, oah.n_dofs)
    ctx = pa.Context(0)
    try:
        ctx.set_problem(pa.Problem(**kw), *(rows or ()))
        _kernels(ctx)
        ctx.assemble_device()
        ctx.synchronize()
        vals = ctx.values()
        assert len(vals) == kw["rowptr"][r1] - kw["rowptr"][r0]
        if dim == 3 and lg == 0:
            assert len(vals) == 1
        if (dim, lg, p) == (2, 2, 1):
            assert len(vals) % 256 and len(vals) == 192
        if (dim, lg, p, rows_frac) == (3, 3, 3, None):
            assert len(vals) > 2048 * 256
        cs = _check_checksum(ctx, vals)
        assert cs["non_finite"] == 0
        # closed form: sum over the owned rows of A 1
        sig = np.asarray(kw["face_sigma"]) if kw["n_faces"] else np.zeros(0)
        fo = np.asarray(kw["face_out"]) if kw["n_faces"] else np.zeros(0, dtype=np.int64)
        fi = np.asarray(kw["face_in"]) if kw["n_faces"] else np.zeros(0, dtype=np.int64)
        off = np.asarray(kw["dof_offset"])
        own = (off >= r0) & (off < r1)
        terms = []
        for f in range(len(fo)):
            if fo[f] < 0 and own[fi[f]]:
                terms.append(sig[f] * math.fsum(kw["fq_w"][kw["fq_ptr"][f]:kw["fq_ptr"][f + 1]]))
        vw = np.asarray(kw["vq_w"])
        for a in np.nonzero(own)[0]:
            terms.append(var.reaction_c * math.fsum(vw[kw["vq_ptr"][a]:kw["vq_ptr"][a + 1]]))
        closed = math.fsum(terms)
        rp, ci, ref = po.assemble_csr(oah, var)
        ref_sum = math.fsum(ref[rp[r0]:rp[r1]])
        assert abs(ref_sum - closed) <= 1e-12 * math.fsum(np.abs(ref[rp[r0]:rp[r1]])), (ref_sum, closed)
        assert abs(cs["sum"] - closed) <= 1e-12 * cs["abs_sum"], (cs["sum"], closed)
        # poisoned: every value is a NaN bit pattern
        ctx.poison_values()
        cs = ctx.checksum()
        assert cs == {"sum": 0.0, "abs_sum": 0.0, "max_abs": 0.0, "non_finite": len(vals)}
        # special values at known positions, written the way poison_values writes
        ctx.assemble_device()
        ctx.synchronize()
        ptr, nv = ctx.device_values()
        assert nv == len(vals)
        special = np.array([np.nan, np.inf, -np.inf, 1.0e15, -3.0e14, np.nan])
        pos = np.unique(np.linspace(0, nv - 1, len(special)).astype(np.int64))
        special = special[:len(pos)]
        hip = _hip()
        for k, v in zip(pos, special):
            buf = np.array([v])
            assert hip.hipMemcpy(C.c_void_p(ptr + 8 * int(k)), C.c_void_p(buf.ctypes.data), 8, 1) == 0
        assert hip.hipDeviceSynchronize() == 0
        want = vals.copy()
        want[pos] = special
        assert np.array_equal(ctx.values(), want, equal_nan=True)
        cs = _check_checksum(ctx, want)
        assert cs["non_finite"] == int((~np.isfinite(special)).sum())
    finally:
        ctx.close()
