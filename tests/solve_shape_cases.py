"""The problems of the solver's shape tests (test infrastructure, no GPU): one list for tests/test_solve_shape_cases_cpu.py (the host
mirror's flattening and the NumPy restatements on oracle-assembled matrices) and for tests/test_gpu_solve_shapes.py (the device), in the
style of cheb_cases.py and transfer_cases.py.  Every case names the property of the flattened arrays it exists for - the branch of
csrc/pdh_solve.hip it reaches - and both tests assert that property (check_property) before anything else, so that a case cannot
silently stop reaching its branch.  All on the unit cube / square with SipVariant.poisson_example."""
import functools

import numpy as np
import scipy.sparse as sp

CHEB_DEGREES = (1, 2, 5)


# ---- agglomerates ---------------------------------------------------------------------------------------------------------------------
def _lex(cells, ijk):
    """cell index of a lexicographic grid (x fastest), as subdivided_hyper_cube numbers it in the mirror and in the oracle"""
    return int(sum(int(ijk[c]) * cells ** c for c in range(len(ijk))))


def big_among_singles(dim, cells, lo, r):
    """one polytope of the r^dim cells [lo, lo + r)^dim (index 0) among single-cell polytopes in cell order, on a lexicographic grid"""
    box = [tuple((k // r ** c) % r + lo for c in range(dim)) for k in range(r ** dim)]
    big = sorted(_lex(cells, ijk) for ijk in box)
    inside = set(big)
    return [big] + [[c] for c in range(cells ** dim) if c not in inside]


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# id: dim, cells per axis (lexicographic subdivided_hyper_cube), agglomerates, basis, degree, and the property the case exists for:
#   n, n_agg, row_min / row_max: shortest and longest row (entries) of the flattened pattern.
# agglomerates: ("block", b) | ("grown", cells per polytope, seed) | ("big", lo, r)
def _case(dim, cells, agg, basis, p, n, n_agg, row_min, row_max, why):
    return dict(dim=dim, cells=cells, agg=agg, basis=basis, p=p, n=n, n_agg=n_agg, row_min=row_min, row_max=row_max, why=why)


CASES = {
    "dgq4_3x3x3": _case(3, 3, ("block", 1), "dgq", 4, 125, 27, 500, 875,
                        "n = 125 with an interior polytope: row_dot's case 8 (500 entries) and its default loop (625 .. 875) in one matrix"),
    "dgq3_big_among_singles": _case(3, 4, ("big", 0, 2), "dgq", 3, 64, 57, 256, 832,
                                    "n = 64: the corner polytope has 12 neighbours, 13 blocks = 832 entries; 4 .. 7 blocks elsewhere"),
    # define_grown_agglomerates(8, seed=6) on 6^3 cells, the call of test_gpu_solve.py's _handler(3, 6, 2, "dgq", 3, "grown"): 27
    # polytopes; with this seed the rows have 6 .. 16 blocks (asserted), so no other seed or mesh was needed
    "dgq3_grown": _case(3, 6, ("grown", 8, 6), "dgq", 3, 64, 27, 384, 1024, "irregular agglomerates with 9 or more blocks in a row"),
    "dgp6": _case(3, 2, ("block", 1), "dgp", 6, 84, 8, 336, 336, "even n > 64: two row groups, the last of 20; two passes per slot"),
    "dgp7": _case(3, 2, ("block", 1), "dgp", 7, 120, 8, 480, 480, "even n > 64: last row group of 56"),
    "dgq5": _case(3, 2, ("block", 1), "dgq", 5, 216, 8, 864, 864, "n = 216: last row group of 24, 4 passes per slot, 2 trips of the default loop"),
    "dgq6": _case(3, 2, ("block", 1), "dgq", 6, 343, 8, 1372, 1372, "odd n = 343: 6 passes per slot, 3 trips"),
    "dgq7": _case(3, 2, ("block", 1), "dgq", 7, 512, 8, 2048, 2048, "n = 512 = 8 x 64: only the full-group trigger stores, 8 full passes, 4 full trips"),
    "slots_289": _case(2, 34, ("block", 2), "dgq", 1, 4, 289, 12, 20, "289 = 256 + 33 slots: k_cg_finalise's second stride is partial"),
    "slots_1024": _case(2, 64, ("block", 2), "dgq", 1, 4, 1024, 12, 20, "1024 slots: 4 partials per thread of k_cg_finalise"),
    "lds_cap_in": _case(2, 33, ("big", 1, 31), "dgq", 7, 64, 129, 192, 8000,
                        "125 blocks x 64 = 8000 entries: 64 000 B of dynamic LDS, 16 trips of the default loop (the last one short)"),
    "lds_cap_out": _case(2, 34, ("big", 1, 32), "dgq", 7, 64, 133, 192, 8256, "129 blocks = 8256 entries > 8192: refused"),
}
LDS_CAP_ENTRIES = 8192

VMULT_IDS = [k for k in CASES if k != "lds_cap_out"]                                      # A
CG3_IDS = [k for k in CASES if CASES[k]["n"] > 64] + ["dgq3_big_among_singles", "dgq3_grown"]  # B
SLOT_IDS = ["slots_289", "slots_1024"]                                                    # C
CHEB_IDS = ["dgq4_3x3x3", "dgq3_big_among_singles", "dgq7", "dgp6"]                       # D
# F: the stored block inverse.  ("mirror", id of CASES) | ("block", dim, cells, per, basis, p) | ("aniso", mesh of aniso_meshes.py, p)
INVERSE_CASES = {
    "dgq3_4x4x4_b2": ("block", 3, 4, 2, "dgq", 3),
    "rect1116": ("aniso", "rect1116", 3),   # cells 1 : 1 : 16, FE_DGQ(3)
    "graded": ("aniso", "graded", 3),       # x^1.6, y^0.7 grading, FE_DGQ(3)
    "dgq3_big_among_singles": ("mirror", "dgq3_big_among_singles"),
}
ANISO_CG_IDS = ["rect1116", "graded"]


def kinds_of(cid):
    """preconditioners of the three-step CG test: block Jacobi where the library offers it (n <= 64)"""
    return ("none", "jacobi") + (("block_jacobi",) if CASES[cid]["n"] <= 64 else ())


def groups_of(cid):
    """explicit cell lists of a case ('big'), or None where the mirror and the oracle define the agglomerates themselves"""
    c = CASES[cid]
    return big_among_singles(c["dim"], c["cells"], c["agg"][1], c["agg"][2]) if c["agg"][0] == "big" else None


def mirror_handler(cid):
    """(handler, element) of the product's host mirror"""
    import polydeal_amd as pa

    c = CASES[cid]
    ah = pa.AgglomerationHandler(pa.BackgroundGrid.subdivided_hyper_cube(c["dim"], c["cells"], 0.0, 1.0))
    if c["agg"][0] == "block":
        ah.define_block_agglomerates(c["agg"][1])
    elif c["agg"][0] == "grown":
        ah.define_grown_agglomerates(c["agg"][1], seed=c["agg"][2])
    else:
        for g in groups_of(cid):
            ah.define_agglomerate(g)
    fe = (pa.FE_DGQ if c["basis"] == "dgq" else pa.FE_AggloDGP)(c["dim"], c["p"])
    ah.initialize_fe_values(c["p"] + 1, c["p"] + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah, fe


def mirror_flat(cid, diag_first):
    import polydeal_amd as pa

    ah, fe = mirror_handler(cid)
    return ah, fe, ah.flatten(pa.SipVariant.poisson_example(fe), diag_first, True)


def check_property(cid, ah, fe, arr):
    """the property the case is listed for, from the handler and the flattened arrays"""
    c = CASES[cid]
    rows = np.diff(np.asarray(arr["rowptr"], dtype=np.int64))
    assert fe.n_dofs_per_cell == c["n"], (cid, fe.n_dofs_per_cell)
    assert ah.n_agglomerates == c["n_agg"] and len(rows) == c["n"] * c["n_agg"], (cid, ah.n_agglomerates, len(rows))
    assert int(rows.max()) == c["row_max"], (cid, int(rows.max()))
    if c["row_min"] is not None:
        assert int(rows.min()) == c["row_min"], (cid, int(rows.min()))
    assert np.all(rows % c["n"] == 0)
    if cid == "lds_cap_out":
        assert rows.max() > LDS_CAP_ENTRIES
    else:
        assert rows.max() <= LDS_CAP_ENTRIES
    if cid in ("dgq4_3x3x3", "dgq3_big_among_singles", "dgq3_grown"):
        assert rows.max() > 512  # row_dot's default loop
    if cid == "dgq4_3x3x3":
        assert rows.min() == 512 - 12  # and its case 8 in the same matrix
    return rows


def _oracle_handler_of(dim, cells, groups, basis, p):
    from oracle import polydeal_oracle as po

    grid = po.subdivided_hyper_cube(dim, cells, 0.0, 1.0)
    ah = po.AgglomerationHandler(grid)
    for g in groups:
        ah.define_agglomerate(g)
    fe = (po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p)
    ah.initialize_fe_values(p + 1, p + 1)
    ah.distribute_agglomerated_dofs(fe)
    return ah


def _csr(ah, diag_first):
    from oracle import polydeal_oracle as po

    rp, ci, va = po.assemble_csr(ah, po.variant_poisson_example(ah.fe), diag_first=diag_first)
    return sp.csr_matrix((va, ci, rp), shape=(ah.n_dofs, ah.n_dofs))


@functools.lru_cache(maxsize=None)
def oracle_system(cid, diag_first=False):
    """(A as scipy CSR, n) of a case of CASES, assembled by the NumPy oracle on the mirror's agglomerates (do not write to it)"""
    from oracle import polydeal_oracle as po

    c = CASES[cid]
    if c["agg"][0] == "block":
        groups = po.block_agglomerates(po.subdivided_hyper_cube(c["dim"], c["cells"], 0.0, 1.0), c["agg"][1])
    elif c["agg"][0] == "grown":
        ah, _ = mirror_handler(cid)  # the mirror keeps the master cell last, the oracle takes the first as master
        groups = [list(ah.get_agglomerate(P)) for P in range(ah.n_agglomerates)]
        groups = [g[-1:] + g[:-1] for g in groups]
    else:
        groups = groups_of(cid)
    return _csr(_oracle_handler_of(c["dim"], c["cells"], groups, c["basis"], c["p"]), diag_first), c["n"]


def inverse_oracle_handler(iid):
    """the oracle's handler of a case of INVERSE_CASES"""
    import aniso_meshes as am
    from oracle import polydeal_oracle as po

    spec = INVERSE_CASES[iid]
    if spec[0] == "aniso":
        return am.oracle_handler(spec[1], po.FE_DGQ(3, spec[2]), spec[2] + 1)
    if spec[0] == "block":
        _, dim, cells, per, basis, p = spec
        return _oracle_handler_of(dim, cells, po.block_agglomerates(po.subdivided_hyper_cube(dim, cells, 0.0, 1.0), per), basis, p)
    c = CASES[spec[1]]
    return _oracle_handler_of(c["dim"], c["cells"], groups_of(spec[1]), c["basis"], c["p"])


@functools.lru_cache(maxsize=None)
def inverse_oracle_system(iid, diag_first=False):
    if INVERSE_CASES[iid][0] == "mirror":
        return oracle_system(INVERSE_CASES[iid][1], diag_first)
    ah = inverse_oracle_handler(iid)
    return _csr(ah, diag_first), ah.fe.n_dofs_per_cell


def rhs(N):
    """b of the CG tests (the seed of test_cg_against_spsolve_and_the_host_loop)"""
    return np.random.default_rng(8).standard_normal(N)


def vectors(N):
    """(b, x0) of the Chebyshev applications (cheb_cases.vectors)"""
    rng = np.random.default_rng(11)
    return rng.standard_normal(N), rng.standard_normal(N)


# ---- measured constants -----------------------------------------------------------------------------------------------------------------
# Rounding of the yardsticks themselves, float64 against numpy.longdouble (x87 80-bit) on oracle-assembled matrices, measured on the CPU
# by `python tests/solve_shape_cases.py` (measure_spreads() below; the printed figures rounded up in their last digit).  The device sums in another order (wave butterfly, fused multiply-add)
# and inverts the blocks by its own Cholesky: it may differ from the float64 yardstick by 100 x the yardstick's spread, the factor
# between the project's 1e-13 vmult bound and its observed 2e-15 (cheb_cases.py); never below 1e-13.
#
# C: cheb_ref.estimate (20 CG steps) on SLOT_IDS, both inner kinds: |est64 - estld| / estld
SLOT_EST_SPREAD = 4.457e-16  # worst: slots_289, point Jacobi
# D: cheb_ref.apply on CHEB_IDS, point Jacobi and (n <= 64) block Jacobi, CHEB_DEGREES, zero and non-zero start: |z64 - zld|_inf / |zld|_inf
SHAPE_Z_SPREAD = 2.919e-15   # worst: dgp6, point Jacobi
# F: numpy.linalg.inv in float64 against cheb_ref.batched_inverse in long double on the diagonal blocks of INVERSE_CASES, per block
# relative to the block's max |D^-1| (the worst block of each case)
INVERSE_SPREAD = {
    "dgq3_4x4x4_b2": 4.179e-16,           # block 5
    "rect1116": 2.772e-16,                # block 0
    "graded": 4.755e-16,                  # block 2
    "dgq3_big_among_singles": 6.001e-16,  # block 37
}
SLOT_EST_TOL = max(100 * SLOT_EST_SPREAD, 1e-13)
SHAPE_Z_TOL = max(100 * SHAPE_Z_SPREAD, 1e-13)
INVERSE_TOL = {k: max(100 * v, 1e-13) for k, v in INVERSE_SPREAD.items()}


def inverse_spread(iid):
    """(largest spread over the blocks of a case of INVERSE_CASES, its block)"""
    import cheb_ref as cr
    from pcg_ref import diag_blocks

    A, n = inverse_oracle_system(iid)
    blocks = diag_blocks(A, n)
    i64 = np.linalg.inv(blocks)
    ild = cr.batched_inverse(blocks, np.longdouble)
    per = np.max(np.abs(i64.astype(np.longdouble) - ild), axis=(1, 2)) / np.max(np.abs(ild), axis=(1, 2))
    return float(per.max()), int(per.argmax())


def estimate_spread(cid, kind):
    import cheb_ref as cr

    A, n = oracle_system(cid)
    e64, eld = cr.estimate(A, n, kind)[0], cr.estimate(A, n, kind, dtype=np.longdouble)[0]
    return float(abs(np.longdouble(e64) - eld) / eld)


def cheb_kinds(cid):
    return ("jacobi",) + (("block_jacobi",) if CASES[cid]["n"] <= 64 else ())


def z_spread(cid, kind, degrees=CHEB_DEGREES):
    import cheb_ref as cr

    LD = np.longdouble
    A, n = oracle_system(cid)
    b, x0 = vectors(A.shape[0])
    lo, hi = cr.bounds(cr.estimate(A, n, kind)[0])
    worst = 0.0
    for m in degrees:
        for start in (None, x0):
            z64 = cr.apply(A, n, kind, lo, hi, m, b, start)
            zld = cr.apply(A, n, kind, lo, hi, m, b, start, dtype=LD)
            worst = max(worst, float(np.max(np.abs(z64.astype(LD) - zld)) / np.max(np.abs(zld))))
    return worst


def measure_spreads():
    we = wz = 0.0
    for cid in SLOT_IDS:
        for kind in ("jacobi", "block_jacobi"):
            s = estimate_spread(cid, kind)
            print("estimate  %-24s %-12s %.3e" % (cid, kind, s), flush=True)
            we = max(we, s)
    for cid in CHEB_IDS:
        for kind in cheb_kinds(cid):
            s = z_spread(cid, kind)
            print("apply     %-24s %-12s %.3e" % (cid, kind, s), flush=True)
            wz = max(wz, s)
    print("SLOT_EST_SPREAD %.3e SHAPE_Z_SPREAD %.3e" % (we, wz))
    for iid in INVERSE_CASES:
        s, blk = inverse_spread(iid)
        print("inverse   %-24s %.3e (block %d)" % (iid, s, blk), flush=True)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure_spreads()
