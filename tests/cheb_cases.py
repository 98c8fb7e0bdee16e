"""The problems of the Chebyshev tests (test infrastructure): one list for the CPU test of the NumPy restatement (tests/cheb_ref.py on
oracle-assembled matrices) and for the GPU test of the device path, so that the device is only compared on cases whose reference
passed its own conditions."""
import numpy as np
import scipy.sparse as sp

# (dim, cells per axis, polytope block, basis, degree of the element, agglomerates, inner kinds)
CASES = [
    (2, 8, 2, "dgq", 2, "block", ("jacobi", "block_jacobi")),   # n = 9
    (3, 4, 2, "dgp", 3, "block", ("jacobi", "block_jacobi")),   # n = 20
    (3, 4, 2, "dgq", 3, "block", ("jacobi", "block_jacobi")),   # n = 64
    (3, 2, 1, "dgq", 4, "block", ("jacobi",)),                  # n = 125 > 64: point Jacobi only
    (2, 16, 2, "dgp", 2, "grown", ("jacobi", "block_jacobi")),  # agglomerates grown over the cell graph
    (3, 2, 2, "dgq", 3, "block", ("jacobi", "block_jacobi")),   # ONE polytope
]
DEGREES = (1, 2, 5)


def case_id(c):
    return "%dD_c%d_b%d_%s%d_%s" % c[:6]


def grown_agglomerates(dim, cells, per):
    """the cell lists of polydeal_amd's define_grown_agglomerates (host mirror, no GPU), as the GPU tests build them, master first"""
    import polydeal_amd as pa

    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, cells.bit_length() - 1)
    ah = pa.AgglomerationHandler(grid)
    ah.define_grown_agglomerates(per ** dim, seed=cells)
    groups = [list(ah.get_agglomerate(P)) for P in range(ah.n_agglomerates)]
    return [g[-1:] + g[:-1] for g in groups]  # the host mirror keeps the master cell last, the oracle takes the first as master


def oracle_system(case, diag_first):
    """(A as scipy CSR, n) of a case, assembled by the NumPy oracle"""
    from oracle import polydeal_oracle as po

    dim, cells, per, basis, p, kind = case[:6]
    grid = po.hyper_cube_refined(dim, 0.0, 1.0, cells.bit_length() - 1)
    ah = po.AgglomerationHandler(grid)
    for g in (po.block_agglomerates(grid, per) if kind == "block" else grown_agglomerates(dim, cells, per)):
        ah.define_agglomerate(g)
    fe = (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    rp, ci, va = po.assemble_csr(ah, po.variant_poisson_example(fe), diag_first=diag_first)
    return sp.csr_matrix((va, ci, rp), shape=(ah.n_dofs, ah.n_dofs)), fe.n_dofs_per_cell


def vectors(N):
    """(b, x0) of the application tests"""
    rng = np.random.default_rng(11)
    return rng.standard_normal(N), rng.standard_normal(N)


# Rounding of the yardstick itself: tests/cheb_ref.py in float64 against numpy.longdouble (x87 80-bit, blocks inverted in long double
# too) on CASES x both layouts x inner kinds x DEGREES x (zero, non-zero start), lambda_lo/hi from the float64 estimate.  Measured by
# measure_spreads() below (python tests/cheb_cases.py): the largest |z64 - zld|_inf / |zld|_inf and |est64 - estld| / estld.
Z_SPREAD = 1.596e-14    # worst: 2D_c16_b2_dgp2_grown, block Jacobi
EST_SPREAD = 2.662e-15  # worst: the single polytope with block Jacobi (P^-1 A = I: CG runs on rounding noise after its first step)
# The device sums in another order (wave butterfly, fused multiply-add) and inverts the blocks by its own Cholesky: 100 x the
# yardstick's spread, the factor between the project's 1e-13 vmult bound and its observed 2e-15; never below 1e-13.
Z_TOL = max(100 * Z_SPREAD, 1e-13)      # 1.596e-12, relative to |z|_inf
EST_TOL = max(100 * EST_SPREAD, 1e-13)  # 2.662e-13, relative to est


def measure_spreads(verbose=True):
    import cheb_ref as cr

    LD = np.longdouble
    wz = we = 0.0
    for case in CASES:
        for df in (True, False):
            A, n = oracle_system(case, df)
            b, x0 = vectors(A.shape[0])
            for kind in case[6]:
                e64, _ = cr.estimate(A, n, kind)
                eld, _ = cr.estimate(A, n, kind, dtype=LD)
                de = float(abs(LD(e64) - eld) / eld)
                lo, hi = cr.bounds(e64)
                dz = 0.0
                for m in DEGREES:
                    for start in (None, x0):
                        z64 = cr.apply(A, n, kind, lo, hi, m, b, start)
                        zld = cr.apply(A, n, kind, lo, hi, m, b, start, dtype=LD)
                        dz = max(dz, float(np.max(np.abs(z64.astype(LD) - zld)) / np.max(np.abs(zld))))
                wz, we = max(wz, dz), max(we, de)
                if verbose:
                    print("%-24s diag_first=%d %-12s est %.6g  spread of est %.3e  of z %.3e" % (case_id(case), df, kind, e64, de, dz), flush=True)
    return wz, we


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("Z_SPREAD %.3e EST_SPREAD %.3e" % measure_spreads())
