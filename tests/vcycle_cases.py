"""The hierarchies and the direct-solve sizes of the V-cycle tests (test infrastructure): one list for the CPU test of the NumPy
restatement (tests/vcycle_ref.py on oracle-assembled matrices) and for the GPU test of the device path (tests/test_gpu_vcycle.py, on the
matrices read back from the device), with the bounds the device is held to."""
import functools

import numpy as np

# (dim, refinements of the unit cube, cells per direction of a polytope on every level coarse to fine, degree of FE_DGQ)
CASES = [
    (2, 3, (4, 2, 1), 1),     # rows 16 / 64 / 256
    (2, 3, (8, 4, 2, 1), 2),  # 9 / 36 / 144 / 576: four levels, a single coarsest polytope
    (3, 2, (4, 2, 1), 1),     # 8 / 64 / 512
    (3, 3, (8, 4, 2), 2),     # 27 / 216 / 1728: n = 27
    (3, 2, (4, 2, 1), 3),     # 64 / 512 / 4096: n = 64, the headline element
    (3, 1, (2, 1), 4),        # 125 / 1000: n = 125, Chebyshev over point Jacobi, chunks of 64
]
ROWS = [(16, 64, 256), (9, 36, 144, 576), (8, 64, 512), (27, 216, 1728), (64, 512, 4096), (125, 1000)]
CPU_CASES = CASES[:4]            # tests/test_vcycle_cpu.py: symmetry, PCG counts
MESH_PAIR = ((2, 3, (8, 4, 2, 1), 2), (2, 4, (8, 4, 2, 1), 2))  # the same hierarchy one refinement apart: the iteration count stays
DEGREE = 3                       # of the Chebyshev smoother
HIERARCHY_CASE = (3, 2, (4, 2, 1), 2)  # levels.multigrid_hierarchy end to end: 27 / 216 / 1728

# direct solve: (dim, refinements, cells per direction of a polytope, degree) -> rows; one polytope, sizes below, at and across multiples
# of 64, the cap
DIRECT_SIZES = [
    ((2, 3, 8, 2), 9),      # one polytope
    ((3, 2, 4, 3), 64),     # one polytope of 64
    ((3, 1, 2, 4), 125),    # one polytope of 125
    ((2, 3, 1, 2), 576),    # 8 x 8 polytopes of 9
    ((3, 1, 1, 4), 1000),   # 8 polytopes of 125
    ((2, 2, 1, 7), 1024),   # 4 x 4 polytopes of 64: the cap
]
DIRECT_REFUSED = ((2, 3, 1, 4), 1600)  # 8 x 8 polytopes of 25
DIRECT_FEW_COLUMNS = 64    # the 1024-row case reads G through this many fixed columns ...
DIRECT_FULL_UP_TO = 1000   # ... every smaller one through all of them


def case_id(c):
    return "%dD_lg%d_b%s_p%d" % (c[0], c[1], "-".join(str(b) for b in c[2]), c[3])


def size_id(s):
    return "%drows_%dD_lg%d_b%d_p%d" % ((s[1],) + s[0])


def inner_kind(n):
    """what levels.multigrid_hierarchy takes: block Jacobi up to 64 dofs per polytope, point Jacobi above"""
    return "block_jacobi" if n <= 64 else "jacobi"


def handlers(dim, lg, blocks, p):
    """([handlers of the host mirror, coarse to fine], [handlers of the oracle on the same grid]); no GPU"""
    import polydeal_amd as pa
    from oracle import polydeal_oracle as po

    grid_o = po.hyper_cube_refined(dim, 0.0, 1.0, lg)
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg)
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


def check_shape(case, mirror):
    """a case is what its comment says before anything is computed on it"""
    rows = ROWS[CASES.index(case)] if case in CASES else None
    got = tuple(ah.n_dofs for ah in mirror)
    assert rows is None or got == rows, (case, got, rows)
    assert all(a < b for a, b in zip(got, got[1:])), got
    return got


@functools.lru_cache(maxsize=None)
def injections(case):
    """[P_l]: the dense injection between level l and l + 1 from the oracle (shared: do not write to them)"""
    from oracle import polydeal_oracle as po

    _, oracles = handlers(*case)
    out = []
    for c, f in zip(oracles, oracles[1:]):
        P = po.fill_injection_matrix(c, f)
        P.setflags(write=False)
        out.append(P)
    return out


def _oracle_matrix(ao):
    import scipy.sparse as sp
    from oracle import polydeal_oracle as po

    rp, ci, va = po.assemble_csr(ao, po.variant_poisson_example(ao.fe), diag_first=False)
    return sp.csr_matrix((va, ci, rp), shape=(ao.n_dofs, ao.n_dofs))


@functools.lru_cache(maxsize=None)
def oracle_hierarchy(case, degree=DEGREE, coarse="direct"):
    """vcycle_ref.Hierarchy of a case from the NumPy oracle alone (SipVariant.poisson_example), smoother bounds from cheb_ref's estimate"""
    import vcycle_ref as vr

    mirror, oracles = handlers(*case)
    check_shape(case, mirror)
    mats = [_oracle_matrix(ao) for ao in oracles]
    n = oracles[0].fe.n_dofs_per_cell
    kind = inner_kind(n)
    return vr.Hierarchy(mats, n, injections(case), vr.smoother_bounds(mats, n, kind), degree, kind, coarse)


def direct_handler(size):
    """(handler of the host mirror, FE) of a direct-solve size, its row count asserted"""
    import polydeal_amd as pa

    (dim, lg, block, p), rows = size
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(block)
    fe = pa.FE_DGQ(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    assert ah.n_dofs == rows, (size, ah.n_dofs)
    return ah, fe


def direct_oracle_matrix(size):
    (dim, lg, block, p), rows = size
    _, oracles = handlers(dim, lg, (block,), p)
    A = _oracle_matrix(oracles[0])
    assert A.shape == (rows, rows)
    return A


def direct_columns(rows):
    """the columns of G a test reads: all of them, or DIRECT_FEW_COLUMNS fixed ones spread over the polytopes (first and last included)"""
    if rows <= DIRECT_FULL_UP_TO:
        return np.arange(rows)
    return np.unique(np.linspace(0, rows - 1, DIRECT_FEW_COLUMNS).round().astype(np.int64))


def rhs(N):
    return np.random.default_rng(11).standard_normal(N)


# Rounding of the yardsticks themselves, measured on the CPU by python tests/vcycle_cases.py (measure_spreads below) on oracle-assembled
# matrices:
#   CYCLE_SPREAD    tests/vcycle_ref.py in float64 against numpy.longdouble (blocks and the coarsest matrix inverted in long double too) on
#                   CASES, three V-cycles from x = 0 at smoother degree DEGREE, lambda_lo / hi from the float64 estimate: the largest
#                   |x64 - xld|_inf / |xld|_inf
#   INVERSE_SPREAD  numpy.linalg.inv against vcycle_ref.inverse_longdouble per size of DIRECT_SIZES: max|G64 - Gld| / max|Gld| (it follows
#                   the condition number, 8.6 at 9 rows and 1.1e4 at 1024: one bound per size, not the worst for all)
CYCLE_SPREAD = 6.360e-15  # worst: 2D_lg3_b8-4-2-1_p2
INVERSE_SPREAD = {9: 1.969e-16, 64: 4.965e-16, 125: 7.324e-16, 576: 1.890e-14, 1000: 3.012e-15, 1024: 8.284e-14}
# The device sums in another order (wave butterfly, fused multiply-add) and inverts by its own Cholesky: 100 x the yardstick's spread as in
# cheb_cases.py and transfer_cases.py, never below 1e-13; relative to |x|_inf for a cycle and to max|G| for the inverse.  The V-cycle
# test adds what the coarsest level's conditioning does to a double inverse: 10 cond_2(A_0) 2.2e-16.
CYCLE_TOL = max(100 * CYCLE_SPREAD, 1e-13)  # 6.360e-13
INVERSE_TOL = {rows: max(100 * s, 1e-13) for rows, s in INVERSE_SPREAD.items()}  # 1e-13 up to 125 rows ... 8.284e-12 at 1024


def measure_spreads(verbose=True):
    import vcycle_ref as vr

    LD = np.longdouble
    wc, wi = 0.0, {}
    for case in CASES:
        H = oracle_hierarchy(case)
        b = rhs(H.mats[-1].shape[0])
        x64, xld, spread = None, None, 0.0
        for _ in range(3):
            x64 = vr.cycle(H, b, x64)
            xld = vr.cycle(H, b, xld, dtype=LD)
            spread = max(spread, float(np.max(np.abs(x64.astype(LD) - xld)) / np.max(np.abs(xld))))
        if verbose:
            print("%-24s cycle spread %.3e" % (case_id(case), spread), flush=True)
        wc = max(wc, spread)
    for size in DIRECT_SIZES:
        D = np.asarray(direct_oracle_matrix(size).todense())
        Gld = vr.inverse_longdouble(D)
        spread = float(np.max(np.abs(np.linalg.inv(D).astype(LD) - Gld)) / np.max(np.abs(Gld)))
        if verbose:
            print("%-28s inverse spread %.3e (cond %.3e)" % (size_id(size), spread, np.linalg.cond(D)), flush=True)
        wi[size[1]] = float("%.3e" % spread)
    return wc, wi


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("CYCLE_SPREAD %.3e INVERSE_SPREAD %s" % measure_spreads())
