"""The problems of the matrix-free operator tests (test infrastructure): one table for the CPU test of the NumPy restatement
(tests/matfree_ref.py against the oracle's matrix) and for the GPU test of csrc/pdh_matfree.h, so that the device is only compared on
cases whose reference passed its own conditions.  Every case is an ORACLE handler of Cartesian cells and a SIP variant."""
import functools

import numpy as np
import scipy.sparse as sp

import cheb_cases as cc
import solve_shape_cases as ssc

# id: (mesh, agglomerates, basis, degree, variant) and what the case reaches in the kernel
#   mesh: ("refined", cells) hyper_cube_refined (Morton) | ("cube", cells) subdivided_hyper_cube (lexicographic) | ("aniso", name)
#   agglomerates: ("block", b) | ("grown", b) cheb_cases.grown_agglomerates | ("big", lo, r) solve_shape_cases.big_among_singles | None
CASES = {}
for _b, _p in (("dgq", 1), ("dgq", 2), ("dgq", 3), ("dgp", 1), ("dgp", 2), ("dgp", 3)):
    # every polytope has a boundary run; merged cells and sub-faces; 4- and 8-slot records
    CASES["c4_b2_%s%d" % (_b, _p)] = (("refined", 4), ("block", 2), _b, _p, "poisson")
for _b in ("dgq", "dgp"):
    # the centre polytope has no boundary run (first_int = 0) and its own block in the middle of the row
    CASES["c6_b2_%s3" % _b] = (("cube", 6), ("block", 2), _b, 3, "poisson")
# several planes per neighbour, terms that do not merge, uneven run lengths
CASES["grown_dgq2"] = (("refined", 4), ("grown", 2), "dgq", 2, "poisson")
CASES["grown_dgp3"] = (("refined", 4), ("grown", 2), "dgp", 3, "poisson")
# a wrong axis, a wrong frame, neighbours shorter along one tangential axis
for _m in ("rect124", "graded", "offset_mod", "pinwheel"):
    CASES["%s_dgq3" % _m] = (("aniso", _m), None, "dgq", 3, "poisson")
CASES["one_polytope_dgq3"] = (("refined", 2), ("block", 2), "dgq", 3, "poisson")  # no interior run
# one polytope of 4^3 cells among single cells: X tables across boxes of ratio 4, 48 interior runs (FE_DGQ(1): the tables of a larger element
# exceed the term kernels' LDS budget on this polytope and the planner takes another kernel)
CASES["big4_dgq1"] = (("cube", 5), ("big", 0, 4), "dgq", 1, "poisson")
CASES["reaction_dgq2"] = (("refined", 4), ("block", 2), "dgq", 2, "reaction")  # K0' = K0 + c M0
CASES["reaction_dgp3"] = (("refined", 4), ("block", 2), "dgp", 3, "reaction")

# the smallest case of every kind (<= 512 columns): the whole operator is read column by column on the device
WHOLE_OPERATOR_IDS = ["c4_b2_dgq1", "c4_b2_dgq2", "c4_b2_dgq3", "c4_b2_dgp1", "c4_b2_dgp2", "c4_b2_dgp3"]
# the Chebyshev applications with the matrix-free operator
CHEB_IDS = ["c4_b2_dgq3", "c4_b2_dgp3", "grown_dgq2", "c6_b2_dgq3"]


def _fe(po, basis, p):
    return (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(3, p)


def variant(po, name, fe):
    return po.variant_poisson_example(fe) if name == "poisson" else po.variant_diffusion_reaction(fe)


@functools.lru_cache(maxsize=None)
def oracle_handler(cid):
    """(oracle handler, SipVariant) of a case (do not write to it)"""
    from oracle import polydeal_oracle as po

    mesh, agg, basis, p, vname = CASES[cid]
    fe = _fe(po, basis, p)
    if mesh[0] == "aniso":
        import aniso_meshes as am

        ah = am.oracle_handler(mesh[1], fe, p + 1)
        return ah, variant(po, vname, fe)
    cells = mesh[1]
    grid = po.hyper_cube_refined(3, 0.0, 1.0, cells.bit_length() - 1) if mesh[0] == "refined" else po.subdivided_hyper_cube(3, cells, 0.0, 1.0)
    if agg[0] == "block":
        groups = po.block_agglomerates(grid, agg[1])
    elif agg[0] == "grown":
        groups = cc.grown_agglomerates(3, cells, agg[1])
    else:
        groups = ssc.big_among_singles(3, cells, agg[1], agg[2])
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah, variant(po, vname, fe)


@functools.lru_cache(maxsize=None)
def oracle_matrix(cid):
    """the oracle's matrix of a case as scipy CSR in the ascending layout (do not write to it)"""
    from oracle import polydeal_oracle as po

    ah, var = oracle_handler(cid)
    rp, ci, va = po.assemble_csr(ah, var, diag_first=False)
    return sp.csr_matrix((va, ci, rp), shape=(ah.n_dofs, ah.n_dofs))


@functools.lru_cache(maxsize=None)
def term_form(cid):
    import matfree_ref as mr

    return mr.TermForm(*oracle_handler(cid))


def check_property(cid, ah):
    """the property a case is listed for, from the oracle handler"""
    mesh, agg, basis, p, _ = CASES[cid]
    nb = [sum(1 for f in range(ah.n_faces[P]) if ah.at_boundary(P, f)) for P in range(ah.n_agglomerates)]
    if cid.startswith("c4_b2") or cid.startswith("reaction"):
        assert ah.n_agglomerates == 8 and all(nb)
    if cid.startswith("c6_b2"):
        assert ah.n_agglomerates == 27 and nb.count(0) == 1
        P = nb.index(0)
        lower = sum(1 for Q in ah.sparsity_blocks()[P] if ah.dof_offset[Q] < ah.dof_offset[P])
        assert 0 < lower < len(ah.sparsity_blocks()[P]) - 1  # own block in the middle of the row
    if cid.startswith("grown"):
        sizes = sorted({len(ah.interface[(P, ah.neighbor(P, f))]) for P in range(ah.n_agglomerates) for f in range(ah.n_faces[P])
                        if not ah.at_boundary(P, f)})
        assert len(sizes) > 1, sizes  # uneven run lengths
    if cid == "one_polytope_dgq3":
        assert ah.n_agglomerates == 1 and ah.n_faces[0] == 1
    if cid == "big4_dgq1":
        ext = [ah.bboxes[P][1] - ah.bboxes[P][0] for P in range(ah.n_agglomerates)]
        assert ext[0].min() >= 4.0 * (1.0 - 1e-12) * ext[1].max() and ah.fe.n_dofs_per_cell <= 64
    if cid.startswith("reaction"):
        assert oracle_handler(cid)[1].reaction_c != 0.0
    assert ah.fe.n_dofs_per_cell <= 64 and ah.fe.degree == p


# Rounding of the yardstick itself: matfree_ref.TermForm.apply in float64 against numpy.longdouble (x87 80-bit) on CASES with the two
# vectors of cheb_cases.vectors, per row relative to sum_j |A_ij| |x_j| of the oracle's matrix.  Measured by measure_spreads() below
# (python tests/matfree_cases.py): the worst row of the worst case.
PRODUCT_SPREAD = 8.761e-16  # worst: graded_dgq3 (3.2e-16 .. 7.1e-16 on the others)
PRODUCT_SPREAD_CASE = "graded_dgq3"
# The device sums in another order (merged terms, fused multiply-add): 100 x the yardstick's spread, the project's factor between a
# yardstick's own spread and what the device is allowed; never below 1e-13.
PRODUCT_TOL = max(100 * PRODUCT_SPREAD, 1e-13)  # 1e-13


def product_spread(cid):
    tf, A = term_form(cid), oracle_matrix(cid)
    worst = 0.0
    for x in cc.vectors(A.shape[0]):
        y64, yld = tf.apply(x), tf.apply(x, np.longdouble)
        scale = np.asarray(abs(A) @ np.abs(x)).reshape(-1)
        worst = max(worst, float(np.max(np.abs(y64.astype(np.longdouble) - yld) / scale)))
    return worst


def measure_spreads(verbose=True):
    worst, where = 0.0, None
    for cid in CASES:
        s = product_spread(cid)
        if verbose:
            print("%-20s spread of the product %.3e" % (cid, s), flush=True)
        if s > worst:
            worst, where = s, cid
    return worst, where


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("PRODUCT_SPREAD %.3e (worst: %s)" % measure_spreads())
