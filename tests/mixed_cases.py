"""The shapes and bounds of the single-precision-smoother tests (test infrastructure, no GPU): one list for tests/test_mixed_cpu.py (the
NumPy restatement tests/mixed_ref.py on oracle-assembled matrices) and for tests/test_gpu_smoother_f32.py (the device, on the matrices
read back).  The shapes are those of cheb_cases.py / solve_shape_cases.py / vcycle_cases.py, imported, not restated; every shape names
the property it is listed for and both tests assert it (check_shape_property) before anything is computed."""
import numpy as np

import cheb_cases as cc
import solve_shape_cases as sc
import vcycle_cases as vc

# Exact-entry shapes.  ("block", dim, cells per axis, cells per polytope and axis, basis, degree) as test_gpu_solve._handler /
# cheb_cases.oracle_system take it, or ("shape", id of solve_shape_cases.CASES); then n, polytopes, shortest and longest row, and why.
ENTRY_SHAPES = {
    "dgq1_2d": (("block", 2, 8, 2, "dgq", 1), 4, 16, 12, 20, "rows shorter than one piece of 128 entries"),
    "dgq2_2d": (("block", 2, 8, 2, "dgq", 2), 9, 16, 27, 45, "odd row lengths 27 and 45 (and 36): the rows of corner and interior polytopes end in a pad entry"),
    "dgq2_3d": (("block", 3, 4, 2, "dgq", 2), 27, 8, 108, 108, "n = 27, odd n: the last row of a slot goes alone"),
    # 4^3 cells: in polytopes of 2^3 every row has 4 blocks (256 entries, two whole pieces); one cell per polytope gives the interior
    # rows of 7 blocks (448 entries: three pieces and a half) - both are kept
    "dgq3_3d_b2": (("block", 3, 4, 2, "dgq", 3), 64, 8, 256, 256, "n = 64, rows of exactly two pieces"),
    "dgq3_3d_b1": (("block", 3, 4, 1, "dgq", 3), 64, 64, 256, 448, "n = 64, rows of 256 .. 448: a partial last piece"),
    "single": (("block", 3, 2, 2, "dgq", 3), 64, 1, 64, 64, "ONE polytope, no neighbours"),
    "dgq3_grown": (("shape", "dgq3_grown"), 64, 27, 384, 1024, "the row length varies per slot, up to 1024 = 8 whole pieces"),
}
# Chebyshev applications: the exact-entry shapes plus n = 125, where point Jacobi (double) runs over the shadow matrix
CHEB_SHAPES = dict(ENTRY_SHAPES)
CHEB_SHAPES["dgq4_3x3x3"] = (("shape", "dgq4_3x3x3"), 125, 27, 500, 875, "n > 64: point Jacobi over the shadow rows, row groups of 64")
# the product on long rows and large n, against NumPy within 1e-13 sum_j |a~_ij x_j| per row
PRODUCT_IDS = ["dgq4_3x3x3", "dgq6", "dgq7", "dgp6", "lds_cap_in"]
DEGREES = (1, 2, 5)
LAYOUTS = (True, False)


def kinds_of(sid):
    return ("jacobi",) + (("block_jacobi",) if CHEB_SHAPES[sid][1] <= 64 else ())


def mirror_flat(sid, diag_first):
    """(handler, element, flattened problem) of the product's host mirror"""
    import polydeal_amd as pa

    spec = CHEB_SHAPES[sid][0]
    if spec[0] == "shape":
        return sc.mirror_flat(spec[1], diag_first)
    _, dim, cells, per, basis, p = spec
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, cells.bit_length() - 1)
    ah = pa.AgglomerationHandler(grid)
    ah.define_block_agglomerates(per)
    fe = (pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah, fe, ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)


def check_shape_property(sid, n, n_agg, rowptr):
    """the property a shape is listed for, from the row pointer of whatever holds it (flattened arrays or a scipy matrix)"""
    _, want_n, want_agg, row_min, row_max, _ = CHEB_SHAPES[sid]
    rows = np.diff(np.asarray(rowptr, dtype=np.int64))
    assert (n, n_agg, len(rows)) == (want_n, want_agg, want_n * want_agg), (sid, n, n_agg, len(rows))
    assert (int(rows.min()), int(rows.max())) == (row_min, row_max), (sid, int(rows.min()), int(rows.max()))
    if sid == "dgq2_2d":
        assert {27, 36, 45} == set(rows.tolist())  # corner, edge and interior polytopes: two of the three lengths are odd
    if sid == "dgq3_3d_b1":
        assert row_max % 128 != 0 and row_max > 128
    return rows


def oracle_system(sid, diag_first=False):
    """(A as scipy CSR, n) of a shape from the NumPy oracle, its property asserted"""
    spec = CHEB_SHAPES[sid][0]
    A, n = sc.oracle_system(spec[1], diag_first) if spec[0] == "shape" else cc.oracle_system(spec[1:] + ("block",), diag_first)
    check_shape_property(sid, n, A.shape[0] // n, A.indptr)
    return A, n


def vectors(N):
    """(b, x0) of the applications (cheb_cases.vectors)"""
    return cc.vectors(N)


# Rounding of the yardstick itself: tests/mixed_ref.py in float64 against numpy.longdouble (x87 80-bit) on oracle-assembled matrices,
# measured on the CPU by `python tests/mixed_cases.py` (measure_spreads below).  Both runs round the SAME doubles to float32 (the matrix
# and numpy.linalg.inv of the blocks), so the spread is that of the double recurrences alone.
#   MIXED_Z_SPREAD      mixed_ref.apply per (shape of CHEB_SHAPES, inner kind), the larger of the two layouts, over DEGREES x (zero, non-zero
#                       start), lambda_lo / hi from cheb_ref's float64 estimate on the unrounded matrix: the largest
#                       |z64 - zld|_inf / |zld|_inf.  One figure per pair, not the worst for all (the convention of
#                       vcycle_cases.INVERSE_SPREAD): the pairs differ in conditioning by orders of magnitude, see below
#   MIXED_CYCLE_SPREAD  mixed_ref.cycle on vcycle_cases.CASES, every level above the coarsest F32, three V-cycles from x = 0 at smoother
#                       degree vcycle_cases.DEGREE: the largest |x64 - xld|_inf / |xld|_inf
MIXED_Z_SPREAD = {
    ("dgq1_2d", "jacobi"): 2.112e-15, ("dgq1_2d", "block_jacobi"): 3.296e-15,
    ("dgq2_2d", "jacobi"): 4.360e-15, ("dgq2_2d", "block_jacobi"): 2.957e-15,
    ("dgq2_3d", "jacobi"): 3.466e-15, ("dgq2_3d", "block_jacobi"): 5.388e-15,
    ("dgq3_3d_b2", "jacobi"): 3.374e-15, ("dgq3_3d_b2", "block_jacobi"): 4.561e-15,
    ("dgq3_3d_b1", "jacobi"): 1.941e-15, ("dgq3_3d_b1", "block_jacobi"): 2.367e-15,
    ("single", "jacobi"): 4.988e-15, ("single", "block_jacobi"): 1.658e-14,  # the worst well-conditioned pair
    ("dgq3_grown", "jacobi"): 7.260e-16, ("dgq3_grown", "block_jacobi"): 5.171e-10,  # (diag_first; 7.620e-11 ascending)
    ("dgq4_3x3x3", "jacobi"): 3.880e-15,
}
MIXED_CYCLE_SPREAD = 5.206e-15  # worst: 2D_lg3_b8-4-2-1_p2
# One pair stands apart: dgq3_grown with block Jacobi.  Its diagonal blocks (FE_DGQ(3) on the bounding box of an irregular agglomerate) have
# cond_2 up to 6e9 (test_gpu_solve_shapes.py), more than 2^24: an inverse rounded to float32 is no small perturbation of the inverse,
# lambda_hi no longer bounds P~^-1 A~ and the polynomial amplifies the rounding of the double recurrence itself.  What the pair can show
# is that conversion and kernels do what the restatement does - not that the result is useful (include/polydeal_hip.h says so).
ILL_CONDITIONED = {("dgq3_grown", "block_jacobi")}
# The device sums in another order (wave butterfly, fused multiply-add): 100 x the yardstick's spread, never below 1e-13 - the convention
# of cheb_cases.py and vcycle_cases.py; relative to |z|_inf.  The V-cycle test adds vcycle_cases' 10 cond_2(A_0) 2.2e-16 for the coarsest
# level's double inverse.
MIXED_Z_TOL = {k: max(100 * v, 1e-13) for k, v in MIXED_Z_SPREAD.items()}  # 1.941e-13 .. 1.658e-12; 5.171e-08 for the pair above
MIXED_CYCLE_TOL = max(100 * MIXED_CYCLE_SPREAD, 1e-13)  # 5.206e-13
# A device that ignored the switch would compute the double application: the two must lie this many bounds apart wherever a shadow entry
# enters the result.  It does not in ONE case - degree 1 from zero over point Jacobi is c2 D^-1 b, no product and a double inverse: there
# the two are the same bits - and the ill-conditioned pair above has no room for it (its bound is the size of the rounding to float32).
SEPARATION = 1000.0


def z_tol(sid, kind):
    return MIXED_Z_TOL[(sid, kind)]


def shadow_enters(kind, degree, zero_start):
    return not (kind == "jacobi" and degree == 1 and zero_start)


def measure_spreads(verbose=True):
    """({(shape, kind): spread of z}, spread of the cycle, its worst case)"""
    import cheb_ref as cr
    import mixed_ref as mr

    LD = np.longdouble
    wz, wc, nc = {}, 0.0, None
    for sid in CHEB_SHAPES:
        for df in LAYOUTS:
            A, n = oracle_system(sid, df)
            b, x0 = vectors(A.shape[0])
            for kind in kinds_of(sid):
                lo, hi = cr.bounds(cr.estimate(A, n, kind)[0])
                S64, Sld = mr.Smoother(A, n, kind), mr.Smoother(A, n, kind, LD)
                dz = 0.0
                for m in DEGREES:
                    for start in (None, x0):
                        z64, zld = S64.apply(lo, hi, m, b, start), Sld.apply(lo, hi, m, b, start)
                        dz = max(dz, float(np.max(np.abs(z64.astype(LD) - zld)) / np.max(np.abs(zld))))
                if verbose:
                    print("apply  %-12s diag_first=%d %-12s spread of z %.3e" % (sid, df, kind, dz), flush=True)
                wz[(sid, kind)] = max(wz.get((sid, kind), 0.0), float("%.3e" % dz))
    for case in vc.CASES:
        H = mr.Hierarchy(vc.oracle_hierarchy(case))
        b = vc.rhs(H.mats[-1].shape[0])
        x64, xld, spread = None, None, 0.0
        for _ in range(3):
            x64 = mr.cycle(H, b, x64)
            xld = mr.cycle(H, b, xld, dtype=LD)
            spread = max(spread, float(np.max(np.abs(x64.astype(LD) - xld)) / np.max(np.abs(xld))))
        if verbose:
            print("cycle  %-24s spread %.3e" % (vc.case_id(case), spread), flush=True)
        if spread > wc:
            wc, nc = spread, vc.case_id(case)
    return wz, wc, nc


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("MIXED_Z_SPREAD %s MIXED_CYCLE_SPREAD %.3e (worst: %s)" % measure_spreads())
