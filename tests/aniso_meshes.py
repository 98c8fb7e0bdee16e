"""Box meshes whose cells are NOT cubes (test infrastructure): different cell sizes per axis, per-axis grading, origins far
from zero, and box agglomerates that meet neighbours shorter along different axes.  On a cube h_0 = h_1 = h_2 and the 1-D rules
of a cell or sub-face are the same in every direction, so a kernel (or the oracle) that reads the wrong axis passes every cube
test; on these meshes it does not.

`oracle_handler(name, fe, nq)` builds the mesh in the oracle; `mirror_grid(name)` the same mesh in the product mirror (where
the mirror can describe it: rectangles, offsets - not the graded meshes, which only the oracle's vertex arrays can carry).
Cell numbering is lexicographic (x fastest) in both."""
import numpy as np

from oracle import polydeal_oracle as po

# name: (dim, cells per axis, lo, hi, per-axis map of [0, 1] (None: linear), agglomerates)
#   agglomerates: int b = b^dim blocks; "pinwheel" = slabs of 4 x 1 x 1 beside 1 x 4 x 1 (family d)
MESHES = {
    # (a) a different cell size on every axis: h = (1/8, 1/4, 1/2) and the extreme 1 : 1 : 16
    "rect124": (3, (4, 4, 4), (0.0, 0.0, 0.0), (0.5, 1.0, 2.0), None, 2),
    "rect1116": (3, (4, 4, 4), (0.0, 0.0, 0.0), (0.25, 0.25, 4.0), None, 2),
    # (b) per-axis grading, a different map on every axis: x^1.6, y^0.7, z linear (cells stay axis-aligned boxes)
    "graded": (3, (4, 4, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (lambda t: t ** 1.6, lambda t: t ** 0.7, None), 2),
    # (c) origins away from zero: |x| / h <= 64 and |x| / h ~ 4000 (cells of 0.25)
    "offset_mod": (3, (4, 4, 4), (12.0, -14.0, 7.0), (13.0, -13.0, 8.0), None, 2),
    "offset_far": (3, (4, 4, 4), (1000.0, 1000.0, 1000.0), (1001.0, 1001.0, 1001.0), None, 2),
    # (d) anisotropic agglomerates: a pinwheel of 4 x 1 slabs round a 3 x 3 centre in a layer one cell thick, under 1 x 1 x 2
    # columns - every face has a neighbour that is the shorter one along some tangential axis, ratios 4 / 3 / 2 / 1
    "pinwheel": (3, (5, 5, 3), (0.0, 0.0, 0.0), (1.0, 1.25, 0.9), None, "pinwheel"),
    # (a), (b) on 2^3 cells, one polytope each: elements of more than 64 dofs (pdh_tiled.h)
    "rect124_2": (3, (2, 2, 2), (0.0, 0.0, 0.0), (0.25, 0.5, 1.0), None, 1),
    "graded_2": (3, (2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (lambda t: t ** 1.6, lambda t: t ** 0.7, None), 1),
    # 2-D variants of (a) and (c) for the 2-D direct kernels
    "rect2d": (2, (8, 4), (0.0, 0.0), (1.0, 2.0), None, 2),
    "offset2d": (2, (8, 8), (-40.0, 25.0), (-38.0, 27.0), None, 2),
}


def _pinwheel_groups(grid):
    nx, ny, nz = grid.dirs
    c = lambda i, j, k: int(grid.ijk_to_cell[(i, j, k)])
    groups = [
        [c(i, 0, 0) for i in range(4)],          # 4 x 1 x 1
        [c(4, j, 0) for j in range(4)],          # 1 x 4 x 1
        [c(i, 4, 0) for i in range(1, 5)],       # 4 x 1 x 1
        [c(0, j, 0) for j in range(1, 5)],       # 1 x 4 x 1
        [c(i, j, 0) for i in range(1, 4) for j in range(1, 4)],  # 3 x 3 x 1
    ]
    groups += [[c(i, j, 1), c(i, j, 2)] for j in range(ny) for i in range(nx)]  # 1 x 1 x 2 columns
    groups = [sorted(g) for g in groups]
    assert sorted(x for g in groups for x in g) == list(range(grid.n_cells))
    return groups


# |x| / h of the origin of "offset_mod" moved to (off, off, off) (cells of 0.25): where the term kernels stop being taken (1 / 0), and
# whether pdh_rows.h still takes FE_DGQ(3) / FE_AggloDGP(3) (offset_handler, tests/test_anisotropic_cpu.py)
OFFSET_BOUNDARY = [
    (0.0, 1, 1), (16.0, 1, 1), (100.0, 1, 1), (300.0, 1, 1),  # |x| / h <= 1204: term kernels
    (400.0, 0, 1), (1000.0, 0, 1),                            # |x| / h ~ 1600, 4000: rules not tensor to the bound; pdh_rows.h stays
    (4000.0, 0, 0), (1.0e4, 0, 0),                            # |x| / h ~ 1.6e4, 4e4: not even the normals are axis-aligned to the bound
]


def oracle_grid(name, scale=1.0, shift=None, perm=None):
    """The mesh in the oracle.  scale / shift: x -> scale * x + shift (applied to lo / hi, so the mesh is generated there, not
    mapped); perm: axis permutation - axis c of the new mesh is axis perm[c] of the named one."""
    dim, nd, lo, hi, maps, _ = MESHES[name]
    lo, hi, nd = np.array(lo, float), np.array(hi, float), tuple(nd)
    if perm is not None:
        lo, hi, nd = lo[list(perm)], hi[list(perm)], tuple(nd[c] for c in perm)
        maps = None if maps is None else tuple(maps[c] for c in perm)
    lo, hi = lo * scale, hi * scale
    if shift is not None:
        lo, hi = lo + shift, hi + shift
    grid = po.subdivided_hyper_rectangle(dim, nd, lo, hi)
    if maps is not None:
        for c, m in enumerate(maps):
            if m is not None:
                t = (grid.vertices[..., c] - lo[c]) / (hi[c] - lo[c])
                grid.vertices[..., c] = lo[c] + (hi[c] - lo[c]) * m(t)
    return grid


def groups_of(name, grid):
    b = MESHES[name][5]
    return _pinwheel_groups(grid) if b == "pinwheel" else po.block_agglomerates(grid, b)


def oracle_handler(name, fe, nq, groups=None, **grid_kw):
    grid = oracle_grid(name, **grid_kw)
    ah = po.AgglomerationHandler(grid)
    for g in (groups_of(name, grid) if groups is None else groups):
        ah.define_agglomerate(g)
    ah.initialize_fe_values(nq, nq)
    ah.distribute_agglomerated_dofs(fe)
    return ah


def offset_handler(off, fe, nq):
    """"offset_mod" with its lower corner at (off, off, off) (OFFSET_BOUNDARY)."""
    return oracle_handler("offset_mod", fe, nq, shift=np.full(3, off) - np.array(MESHES["offset_mod"][2]))


def kernel_selection(kw):
    """(pdh_check_terms, its pdh_last_error, pdh_check_rows, its pdh_last_error) of a flattened description: which row kernel the
    host selection grants (the library's planner, without the diagnostic switches PDH_TERMS / PDH_TERMS_DGQ3)."""
    import ctypes as C

    import polydeal_amd as pa

    lib = pa.load_library()
    lib.pdh_last_error.restype = C.c_char_p
    prob = pa.Problem(**kw)
    rt = lib.pdh_check_terms(C.byref(prob.c), 0, kw["n_rows"], None)
    wt = (lib.pdh_last_error(None) or b"").decode()
    rr = lib.pdh_check_rows(C.byref(prob.c), 0, kw["n_rows"])
    wr = (lib.pdh_last_error(None) or b"").decode()
    return rt, wt, rr, wr


def mirror_grid(name):
    import polydeal_amd as pa

    dim, nd, lo, hi, maps, _ = MESHES[name]
    assert maps is None, "the product mirror describes uniform rectangles only"
    return pa.BackgroundGrid.subdivided_hyper_rectangle(dim, nd, lo, hi)


def mirror_handler(name, fe, nq):
    """Product mirror on the same mesh and agglomerates (the master cell - the oracle's cells[0], the lowest index - first)."""
    import polydeal_amd as pa

    grid = mirror_grid(name)
    ah = pa.AgglomerationHandler(grid)
    og = oracle_grid(name)
    for g in groups_of(name, og):
        ah.define_agglomerate(g)
    ah.initialize_fe_values(nq, nq)
    ah.distribute_agglomerated_dofs(fe)
    return ah


def permuted_groups(name, perm):
    """The agglomerates of `name` on the mesh permuted by `perm` (oracle_grid(name, perm=perm)), same polytope order."""
    g0, g1 = oracle_grid(name), oracle_grid(name, perm=perm)
    out = []
    for g in groups_of(name, g0):
        cells = []
        for cell in g:
            ijk = g0.cell_ijk[cell]
            cells.append(int(g1.ijk_to_cell[tuple(int(ijk[c]) for c in perm)]))
        out.append(sorted(cells))
    return out


def permutation_map(ah0, ah1, perm):
    """Dof index of ah1 for every dof of ah0, for FE_DGQ on the permuted mesh: polytopes matched by their bounding boxes, dofs by
    rotating the lexicographic digits (dof digit c of ah1 = digit perm[c] of ah0)."""
    fe = ah0.fe
    dim, m = fe.dim, fe.degree + 1
    boxes1 = {tuple(np.round(np.concatenate(ah1.bboxes[Q]), 12)): Q for Q in range(ah1.n_agglomerates)}
    out = np.zeros(ah0.n_dofs, dtype=np.int64)
    for P in range(ah0.n_agglomerates):
        lo, hi = ah0.bboxes[P]
        Q = boxes1[tuple(np.round(np.concatenate([lo[list(perm)], hi[list(perm)]]), 12))]
        for i in range(m ** dim):
            d0 = [(i // m ** c) % m for c in range(dim)]
            j = sum(d0[perm[c]] * m ** c for c in range(dim))
            out[ah0.dof_offset[P] + i] = ah1.dof_offset[Q] + j
    return out


def coefficients(ah, func):
    """Coefficients of a polynomial of degree <= p (func: points [N, dim] -> [N]) in every polytope's basis, from its values at the
    polytope's own quadrature points (least squares; exact for functions the space holds)."""
    u = np.zeros(ah.n_dofs)
    for P in range(ah.n_agglomerates):
        x, _ = ah.agglomerated_quadrature(P)
        val, _ = ah.fe.shape(ah.real_to_unit(P, x))
        u[ah.dof_indices(P)] = np.linalg.lstsq(val, func(x), rcond=None)[0]
    return u


def box_boundary_integrals(lo, hi):
    """|dOmega| and int_dOmega x_c^2 (c = 0 .. d-1) on the box prod [lo_c, hi_c], in closed form: the two faces normal to c carry
    x_c = lo_c, hi_c over an area A_c = prod_{e != c} L_e; a face normal to d != c carries the mean of x_c^2 over [lo_c, hi_c]."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    L = hi - lo
    dim = len(L)
    A = np.array([np.prod(np.delete(L, c)) for c in range(dim)])
    area = 2.0 * A.sum()
    x2 = np.zeros(dim)
    for c in range(dim):
        mean_sq = (hi[c] ** 3 - lo[c] ** 3) / (3.0 * L[c])
        x2[c] = A[c] * (lo[c] ** 2 + hi[c] ** 2) + 2.0 * mean_sq * (A.sum() - A[c])
    return area, x2


def cell_boundary_integrals(ah):
    """Per polytope: (area, int x_c^2 for every c) of its part of the domain boundary, in closed form from the cell vertices of an
    axis-aligned box mesh (graded meshes: sigma differs from polytope to polytope)."""
    g = ah.grid
    dim = g.dim
    area = np.zeros(ah.n_agglomerates)
    x2 = np.zeros((ah.n_agglomerates, dim))
    for P in range(ah.n_agglomerates):
        for cell in ah.get_agglomerate(P):
            clo, chi = g.vertices[cell].min(axis=0), g.vertices[cell].max(axis=0)
            for f in range(2 * dim):
                if g.neighbor(cell, f) != po.INVALID:
                    continue
                ax = f // 2
                a = np.prod(np.delete(chi - clo, ax))
                area[P] += a
                for c in range(dim):
                    if c == ax:
                        x2[P, c] += a * (chi[c] if f % 2 else clo[c]) ** 2
                    else:
                        x2[P, c] += a * (chi[c] ** 3 - clo[c] ** 3) / (3.0 * (chi[c] - clo[c]))
    return area, x2


def domain_box(name, **grid_kw):
    g = oracle_grid(name, **grid_kw)
    V = g.vertices.reshape(-1, g.dim)
    return V.min(axis=0), V.max(axis=0)


def domain_box_of(ah):
    V = ah.grid.vertices.reshape(-1, ah.grid.dim)
    return V.min(axis=0), V.max(axis=0)
