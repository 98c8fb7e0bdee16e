"""The hierarchies of the Galerkin-product tests (test infrastructure): one list for the CPU tests of the host planner and of the NumPy
yardstick (tests/galerkin_ref.py) and for the GPU tests of pdh_galerkin_device (tests/test_gpu_galerkin.py).  Every case asserts its own
shape - dofs per polytope, rows per level, coarse blocks and the largest number of fine blocks one coarse block receives, per level
pair coarse to fine - before anything is computed on it."""
import functools

import numpy as np

import vcycle_cases as vc

# (dim, refinements of the unit cube, cells per direction of a polytope on every level coarse to fine, degree of FE_DGQ)
CASES = [
    (2, 3, (4, 2, 1), 1),     # n = 4
    (2, 3, (8, 4, 2, 1), 2),  # n = 9, four levels, a single coarsest polytope: one block receives everything
    (3, 2, (4, 2, 1), 1),     # n = 8
    (3, 3, (8, 4, 2), 2),     # n = 27
    (3, 2, (4, 2, 1), 3),     # n = 64: the headline element, 32 contributions to a diagonal block
    (2, 2, (2, 1), 7),        # n = 64 with N1D = 8
]
# further cases: ("aniso", mesh of tests/aniso_meshes.py, blocks, degree) - nested block agglomerates on cells that are no cubes;
# ("distorted", dim, refinements, blocks, degree, factor) - BackgroundGrid.distort: bounding boxes that overlap, points-based description
EXTRA = [
    ("aniso", "rect124", (2, 1), 1),
    ("distorted", 2, 3, (4, 2), 2, 0.15),
]
ALL = CASES + EXTRA
# the pair whose polytope numbering and dof offsets are permuted on both levels (tests/test_gpu_galerkin.py)
PERMUTED_BASE = (2, 3, (4, 2), 2)
# all four layout combinations (fine x coarse: deal.II diagonal first | ascending) run on these; the others on deal.II / deal.II
LAYOUT_CASES = [CASES[1], CASES[3], CASES[4]]

# case -> (n, rows per level, coarse blocks per pair, largest number of contributions to one coarse block per pair)
SHAPES = {
    CASES[0]: (4, (16, 64, 256), (12, 64), (12, 12)),
    CASES[1]: (9, (9, 36, 144, 576), (1, 12, 64), (12, 12, 12)),
    CASES[2]: (8, (8, 64, 512), (1, 32), (32, 32)),
    CASES[3]: (27, (27, 216, 1728), (1, 32), (32, 32)),
    CASES[4]: (64, (64, 512, 4096), (1, 32), (32, 32)),
    CASES[5]: (64, (256, 1024), (12,), (12,)),
    EXTRA[0]: (8, (64, 512), (32,), (32,)),
    EXTRA[1]: (9, (36, 144), (12,), (12,)),
    PERMUTED_BASE: (9, (36, 144), (12,), (12,)),
}

# PCG iterations to rel_tol 1e-13 with the V-cycle of vcycle_ref (Chebyshev(3) over block Jacobi, direct coarsest solve) as the
# preconditioner, rhs seed 11, on the oracle's finest matrix as assembled (not symmetrised): (Galerkin hierarchy, re-assembled hierarchy),
# measured by tests/test_galerkin_cpu.py::test_pcg_on_the_galerkin_hierarchy, which pins the first of each pair.
PCG_CASES = [CASES[0], CASES[1], CASES[2], (3, 2, (4, 2, 1), 2), vc.MESH_PAIR[1]]
PCG_COUNTS = dict(zip(PCG_CASES, [(35, 37), (32, 28), (28, 31), (31, 31), (35, 29)]))


def case_id(c):
    if isinstance(c[0], str):
        return "_".join(str(x) if not isinstance(x, tuple) else "-".join(map(str, x)) for x in c)
    return vc.case_id(c)


@functools.lru_cache(maxsize=None)
def handlers(case):
    """([handlers of the host mirror, coarse to fine], [handlers of the oracle on the same vertices]); no GPU"""
    import polydeal_amd as pa
    from oracle import polydeal_oracle as po

    if not isinstance(case[0], str):
        return vc.handlers(*case)
    if case[0] == "aniso":
        import aniso_meshes as am

        _, name, blocks, p = case
        dim = am.MESHES[name][0]
        grid, grid_o = am.mirror_grid(name), am.oracle_grid(name)
    else:
        _, dim, lg, blocks, p, factor = case
        grid_o = po.hyper_cube_refined(dim, 0.0, 1.0, lg)
        grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg)
        grid.distort(factor, seed=3)  # (the two RNG streams differ: distort the product's grid and copy its vertices)
        for cell in range(grid_o.n_cells):
            grid_o.vertices[cell] = grid.cell_vertices(cell)
    mirror, oracles = [], []
    for b in blocks:
        ah = pa.AgglomerationHandler(grid)
        ah.define_block_agglomerates(b)
        ah.initialize_fe_values(p + 1, p + 1)
        ah.distribute_agglomerated_dofs(pa.FE_DGQ(dim, p))
        mirror.append(ah)
        ao = po.AgglomerationHandler(grid_o)
        for g in po.block_agglomerates(grid_o, b):
            ao.define_agglomerate(g)
        ao.initialize_fe_values(p + 1, p + 1)
        ao.distribute_agglomerated_dofs(po.FE_DGQ(dim, p))
        oracles.append(ao)
    return mirror, oracles


def dim_degree(case):
    if case[0] == "aniso":
        import aniso_meshes as am
        return am.MESHES[case[1]][0], case[3]
    return (case[1], case[4]) if case[0] == "distorted" else (case[0], case[3])


@functools.lru_cache(maxsize=None)
def injections(case):
    """[P_l]: the dense injection between level l and l + 1 from the oracle (shared: do not write to them)"""
    from oracle import polydeal_oracle as po

    _, oracles = handlers(case)
    out = []
    for c, f in zip(oracles, oracles[1:]):
        P = po.fill_injection_matrix(c, f)
        P.setflags(write=False)
        out.append(P)
    return out


@functools.lru_cache(maxsize=None)
def oracle_matrices(case):
    """[scipy CSR of every level, coarse to fine] assembled by the oracle (SipVariant.poisson_example), ascending columns"""
    _, oracles = handlers(case)
    return [vc._oracle_matrix(ao) for ao in oracles]


@functools.lru_cache(maxsize=None)
def descriptions(case):
    """[TransferDesc of every level pair, coarse to fine] from the host mirror"""
    from polydeal_amd.handler import transfer_description

    mirror, _ = handlers(case)
    return [transfer_description(c, f) for c, f in zip(mirror, mirror[1:])]


def level_lists(A, desc_off, n, order_key=None):
    """(blk_ptr, blk_dof) of a level from its oracle matrix: the pattern of its rows, blocks in ascending order_key (None: dof_offset)"""
    import galerkin_ref as gr

    off = np.asarray(desc_off, dtype=np.int64)
    poly_of_row = np.empty(A.shape[0], dtype=np.int64)
    for P, o in enumerate(off):
        poly_of_row[o:o + n] = P
    coo = A.tocoo()
    pattern = set(zip(poly_of_row[coo.row].tolist(), poly_of_row[coo.col].tolist()))
    return gr.block_lists(pattern, off, order_key)


def check_shape(case):
    """a case is what SHAPES says: n, rows, and - from the brute-force plan on the oracle's patterns - coarse blocks and the largest number
    of contributions per pair"""
    import galerkin_ref as gr

    n, rows, n_blocks, most = SHAPES[case]
    mirror, _ = handlers(case)
    dim, p = dim_degree(case)
    assert n == (p + 1) ** dim and tuple(ah.n_dofs for ah in mirror) == rows, (case, tuple(ah.n_dofs for ah in mirror))
    mats, descs = oracle_matrices(case), descriptions(case)
    got_blocks, got_most = [], []
    for l, d in enumerate(descs):
        fine = level_lists(mats[l + 1], d.fine_dof_offset, n)
        coarse = level_lists(mats[l], d.coarse_dof_offset, n)
        plan = gr.brute_force_plan(d.parent, fine, d.fine_dof_offset, coarse, d.coarse_dof_offset)
        got_blocks.append(len(plan))
        got_most.append(max(len(e) for e in plan))
    assert (tuple(got_blocks), tuple(got_most)) == (n_blocks, most), (case, got_blocks, got_most)
    return rows


def rhs(N):
    return vc.rhs(N)
