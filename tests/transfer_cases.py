"""The level pairs of the transfer tests (test infrastructure): one list for the CPU tests of the host-only planner and for the GPU tests
of the kernels, each with its description (polydeal_amd._capi.TransferDesc) and the dense injection P it is compared against -
oracle.polydeal_oracle.fill_injection_matrix for the handler pairs, the Kronecker formula in NumPy for the raw descriptions."""
import functools

import numpy as np

# (dim, refinements of the unit cube, coarse block, fine block, degree, distortion): the pairs of test_gpu_parity.py::
# test_injection_matrix_parity that cover every way the kernels cut a wave
PAIRS = [
    (2, 3, 4, 2, 1, 0.0),  # n = 4, many polytopes per wave
    (2, 3, 4, 1, 3, 0.2),  # n = 16, 16 children
    (2, 4, 8, 2, 7, 0.1),  # N1D = 8, n = 64
    (3, 2, 4, 2, 2, 0.1),  # n = 27, does not divide 64
    (3, 2, 2, 1, 3, 0.0),  # n = 64
    (3, 2, 2, 1, 4, 0.1),  # n = 125 > 64
    (3, 1, 2, 1, 1, 0.0),  # one coarse polytope
]
RAW = ["uneven", "permuted", "permuted_2d"]
# one raw description per (dim, N1D) pair the kernels instantiate (csrc/pdh_transfer.hip: launch_dim), see _boxes()
BOX_PAIRS = [(dim, n1d) for dim in (2, 3) for n1d in range(2, 9)]
RAW += ["boxes_%dd_n%d" % pair for pair in BOX_PAIRS]
CASES =[("pair",) + p for p in PAIRS] + [("raw", name) for name in RAW]
PERMUTED_BASE = (3, 2, 4, 2, 2, 0.1)     # (one coarse polytope: only the fine numbering can move)
PERMUTED_2D_BASE = (2, 3, 4, 2, 1, 0.0)  # four coarse polytopes: both numberings move

# two-grid composition: (dim, refinements, coarse block, fine block, degree), undistorted, SipVariant.poisson_example
TWOGRID_PAIRS = [(2, 3, 4, 2, 1), (2, 3, 2, 1, 2), (3, 2, 2, 1, 2)]
TWOGRID_DEGREE = 3  # of the Chebyshev smoother over block Jacobi
# Rounding of the yardstick itself: tests/twogrid_ref.py in float64 against numpy.longdouble (blocks and the coarse matrix inverted in
# long double too) on TWOGRID_PAIRS, three cycles from x = 0 on oracle-assembled matrices, lambda_lo / hi from the float64 estimate.
# Measured by measure_twogrid_spread() below (python tests/transfer_cases.py): the largest |x64 - xld|_inf / |xld|_inf.
TWOGRID_SPREAD = 1.052e-14  # worst: (2, 3, 2, 1, 2)
# The device sums in another order and inverts the blocks by its own Cholesky: 100 x the yardstick's spread as in cheb_cases.py, never below
# 1e-13; relative to |x|_inf.  The test adds what the coarse CG's tolerance leaves: 10 cond_2(A_c) coarse_rel_tol.
TWOGRID_TOL = max(100 * TWOGRID_SPREAD, 1e-13)  # 1.052e-12


def case_id(c):
    return "raw_" + c[1] if c[0] == "raw" else "%dD_lg%d_c%d_f%d_p%d_d%g" % c[1:]


def poly(dim, p):
    """the degree-p polynomial of test_injection_matrix_parity"""
    return lambda x: 1.0 + x[:, 0] ** p - 0.5 * x[:, 1] ** p * x[:, 0] + (x[:, -1] ** p if dim == 3 else 0.0)


def handler_pair(dim, lg, bc, bf, p, dist):
    """((coarse, fine) handlers of the host mirror, (coarse, fine) handlers of the oracle on the same vertices); no GPU"""
    import polydeal_amd as pa
    from oracle import polydeal_oracle as po

    grid_o = po.hyper_cube_refined(dim, 0.0, 1.0, lg)
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg)
    if dist:  # the two RNG streams differ: distort the product's grid and copy its vertices
        grid.distort(dist, seed=3)
        for cell in range(grid_o.n_cells):
            grid_o.vertices[cell] = grid.cell_vertices(cell)
    handlers, oracles = [], []
    for b in (bc, bf):
        ah = pa.AgglomerationHandler(grid)
        ah.define_block_agglomerates(b)
        ah.initialize_fe_values(p + 1, p + 1)
        ah.distribute_agglomerated_dofs(pa.FE_DGQ(dim, p))
        handlers.append(ah)
        ao = po.AgglomerationHandler(grid_o)
        for g in po.block_agglomerates(grid_o, b):
            ao.define_agglomerate(g)
        ao.initialize_fe_values(p + 1, p + 1)
        ao.distribute_agglomerated_dofs(po.FE_DGQ(dim, p))
        oracles.append(ao)
    return handlers, oracles


def multi_index(dim, p):
    """[n][dim] digits of every dof, first axis fastest (pdh::multi_indices)"""
    n1d = p + 1
    i = np.arange(n1d ** dim)
    return np.stack([(i // n1d ** c) % n1d for c in range(dim)], axis=1)


def kron_blocks(B):
    """[n_fine][n][n] from the 1-D factors B [n_fine][dim][n1d][n1d] (B_c[i][j]), first axis fastest"""
    out = B[:, 0]
    for c in range(1, B.shape[1]):
        out = np.einsum("fab,fij->faibj", B[:, c], out).reshape(len(B), B.shape[2] * out.shape[1], -1)
    return out


def dense_from_blocks(desc, blocks):
    P = np.zeros((desc.n_fine_rows, desc.n_coarse_rows))
    n = desc.n
    for F in range(desc.n_fine):
        fo, co = int(desc.fine_dof_offset[F]), int(desc.coarse_dof_offset[desc.parent[F]])
        P[fo:fo + n, co:co + n] = blocks[F]
    return P


def kronecker_ref(desc):
    """dense P of a description by the Kronecker formula in NumPy: B_c[i][j] = l_j((lo_F + node_i h_F - lo_C) / h_C)"""
    from oracle import polydeal_oracle as po

    nodes = po.gauss_lobatto_nodes(desc.degree)
    B = np.zeros((desc.n_fine, desc.dim, desc.degree + 1, desc.degree + 1))
    for F in range(desc.n_fine):
        bf, bc = desc.fine_bbox[F], desc.coarse_bbox[desc.parent[F]]
        for c in range(desc.dim):
            xi = (bf[0, c] + nodes * (bf[1, c] - bf[0, c]) - bc[0, c]) / (bc[1, c] - bc[0, c])
            B[F, c] = po.lagrange_1d(nodes, xi)[0].T
    return dense_from_blocks(desc, kron_blocks(B))


def interpolate(desc, level, f):
    """coefficients of the nodal interpolant of f on the boxes of a level ('fine' | 'coarse') of a description"""
    from oracle import polydeal_oracle as po

    bbox, off, rows = (desc.fine_bbox, desc.fine_dof_offset, desc.n_fine_rows) if level == "fine" else \
        (desc.coarse_bbox, desc.coarse_dof_offset, desc.n_coarse_rows)
    unit = po.gauss_lobatto_nodes(desc.degree)[multi_index(desc.dim, desc.degree)]  # [n][dim]
    u = np.zeros(rows)
    for P in range(len(bbox)):
        u[int(off[P]):int(off[P]) + desc.n] = f(bbox[P, 0] + unit * (bbox[P, 1] - bbox[P, 0]))
    return u


def _uneven():
    """4 x 4 cells on the unit square, p = 2: fine polytopes of 2 x 1 cells, coarse polytopes of 12 and 4 cells (6 and 2 children),
    non-square boxes on both levels"""
    from polydeal_amd._capi import TransferDesc

    fine = [[[0.5 * col, 0.25 * row], [0.5 * (col + 1), 0.25 * (row + 1)]] for row in range(4) for col in range(2)]
    coarse = [[[0.0, 0.0], [1.0, 0.75]], [[0.0, 0.75], [1.0, 1.0]]]
    parent = [0 if row < 3 else 1 for row in range(4) for _ in range(2)]
    return TransferDesc(dim=2, degree=2, fine_bbox=fine, coarse_bbox=coarse, fine_dof_offset=9 * np.arange(8),
                        coarse_dof_offset=9 * np.arange(2), parent=parent)


def _permuted(base=PERMUTED_BASE):
    """a handler pair (the 3-D n = 27 one) with the fine dof offsets in reverse polytope order and the coarse ones shuffled (fixed seed)"""
    from polydeal_amd._capi import TransferDesc

    d = build(("pair",) + base).desc
    coarse_off = d.n * np.random.default_rng(5).permutation(d.n_coarse)
    assert d.n_coarse == 1 or not np.array_equal(coarse_off, d.coarse_dof_offset)
    return TransferDesc(dim=d.dim, degree=d.degree, fine_bbox=d.fine_bbox, coarse_bbox=d.coarse_bbox,
                        fine_dof_offset=d.n * np.arange(d.n_fine)[::-1], coarse_dof_offset=coarse_off, parent=d.parent)


def boxes_group(dim, n1d):
    """G of csrc/pdh_transfer.hip's Cut: polytopes of fewer than 64 dofs that share a wave"""
    return max(1, 64 // n1d ** dim)


def _boxes(dim, n1d):
    """Three coarse boxes inside the unit cube with a different extent on every axis and 1, 2 and G + 3 children: uneven children, and
    fine and coarse counts that are no multiples of G (the kernels' idle groups, pol[g] = -1).  Every child is a proper sub-box of its
    parent - the children need not tile it, the planner only asks that they lie inside - with its own offset and width on EACH axis
    (fixed seed), so that every 1-D matrix of every child is a different full matrix: mixing up two axes or transposing a factor
    changes the answer, which slabs along one axis (identity factors on the others) would not show.  The fine polytopes come in a
    shuffled order (the children of a parent are not contiguous) and the dof offsets of both levels are permuted."""
    from polydeal_amd._capi import TransferDesc

    n, G = n1d ** dim, boxes_group(dim, n1d)
    rng = np.random.default_rng(1000 * dim + n1d)
    coarse = np.array([[[0.00, 0.00, 0.20], [0.30, 0.80, 0.90]],
                       [[0.30, 0.10, 0.00], [0.55, 0.70, 0.50]],
                       [[0.55, 0.25, 0.10], [1.00, 1.00, 1.00]]])[:, :, :dim]
    parent = np.repeat(np.arange(3), [1, 2, G + 3])
    parent = parent[rng.permutation(len(parent))]
    ext = coarse[parent, 1] - coarse[parent, 0]

    def apart(v):  # no two axes of a child alike
        return min(float(np.abs(v[:, a] - v[:, b]).min()) for a in range(dim) for b in range(a)) > 1e-3
    while True:  # (fixed seed: the same draw every time)
        start = rng.uniform(0.05, 0.45, (len(parent), dim))  # as fractions of the parent's extent
        width = rng.uniform(0.20, 0.50, (len(parent), dim))
        if apart(start) and apart(width):
            break
    assert apart(ext)
    lo = coarse[parent, 0] + start * ext
    fine = np.stack([lo, lo + width * ext], axis=1)
    def permutation(m):
        while True:
            p = rng.permutation(m)
            if np.any(p != np.arange(m)):
                return p
    return TransferDesc(dim=dim, degree=n1d - 1, fine_bbox=fine, coarse_bbox=coarse, fine_dof_offset=n * permutation(len(parent)),
                        coarse_dof_offset=n * permutation(3), parent=parent)


class Case:
    def __init__(self, case):
        from polydeal_amd.handler import transfer_description

        self.case = case
        self.handlers = self.oracles = None
        if case[0] == "pair":
            self.handlers, self.oracles = handler_pair(*case[1:])
            self.desc = transfer_description(*self.handlers)
        elif case[1].startswith("boxes_"):
            self.desc = _boxes(int(case[1][6]), int(case[1][10:]))
        else:
            self.desc = {"uneven": _uneven, "permuted": _permuted, "permuted_2d": lambda: _permuted(PERMUTED_2D_BASE)}[case[1]]()
        self._P = None

    @property
    def P(self):
        """transfer_ref: the dense injection, computed once and shared (do not write to it)"""
        if self._P is None:
            if self.oracles is not None:
                from oracle import polydeal_oracle as po
                self._P = po.fill_injection_matrix(*self.oracles)
            else:
                self._P = kronecker_ref(self.desc)
            self._P.setflags(write=False)
        return self._P


@functools.lru_cache(maxsize=None)
def build(case):
    return Case(case)


def transfer_ref(case):
    return build(case).P


def headline_description():
    """the headline pair as a raw description: 64^3 cells of the unit cube, p = 3, blocks of 2 (32^3 fine polytopes) and 4 (16^3 coarse);
    uniform boxes, polytopes in lexicographic order (x fastest), parent and offsets arithmetic"""
    from polydeal_amd._capi import TransferDesc

    def level(m):
        k = np.arange(m ** 3)
        ijk = np.stack([k % m, (k // m) % m, k // (m * m)], axis=1)
        return ijk, np.stack([ijk / m, (ijk + 1) / m], axis=1)
    fi, fb = level(32)
    _, cb = level(16)
    parent = (fi[:, 0] // 2) + 16 * (fi[:, 1] // 2) + 256 * (fi[:, 2] // 2)
    return TransferDesc(dim=3, degree=3, fine_bbox=fb, coarse_bbox=cb, fine_dof_offset=64 * np.arange(32 ** 3),
                        coarse_dof_offset=64 * np.arange(16 ** 3), parent=parent)


# ---- two-grid composition ---------------------------------------------------------------------------------------------------------------
def twogrid_oracle_system(pair):
    """(A_fine, A_coarse as scipy CSR, n, dense P) of a two-grid pair, all from the NumPy oracle"""
    import scipy.sparse as sp
    from oracle import polydeal_oracle as po

    dim, lg, bc, bf, p = pair
    _, oracles = handler_pair(dim, lg, bc, bf, p, 0.0)
    mats = []
    for ao in oracles:
        rp, ci, va = po.assemble_csr(ao, po.variant_poisson_example(ao.fe), diag_first=False)
        mats.append(sp.csr_matrix((va, ci, rp), shape=(ao.n_dofs, ao.n_dofs)))
    return mats[1], mats[0], oracles[0].fe.n_dofs_per_cell, po.fill_injection_matrix(*oracles)


def twogrid_rhs(N):
    return np.random.default_rng(11).standard_normal(N)


def measure_twogrid_spread(verbose=True):
    import cheb_ref as cr
    import twogrid_ref as tg

    LD = np.longdouble
    worst, where = 0.0, ""
    for pair in TWOGRID_PAIRS:
        Af, Ac, n, P = twogrid_oracle_system(pair)
        lo, hi = cr.bounds(cr.estimate(Af, n, "block_jacobi")[0])
        b = twogrid_rhs(Af.shape[0])
        x64, xld = np.zeros(len(b)), np.zeros(len(b), dtype=LD)
        spread = 0.0
        for _ in range(3):
            x64 = tg.cycle(Af, Ac, n, P, lo, hi, TWOGRID_DEGREE, b, x64)
            xld = tg.cycle(Af, Ac, n, P, lo, hi, TWOGRID_DEGREE, b, xld, dtype=LD)
            spread = max(spread, float(np.max(np.abs(x64.astype(LD) - xld)) / np.max(np.abs(xld))))
        if verbose:
            print("%s spread %.3e" % (pair, spread), flush=True)
        if spread > worst:
            worst, where = spread, str(pair)
    return worst, where


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("TWOGRID_SPREAD %.3e (%s)" % measure_twogrid_spread())
