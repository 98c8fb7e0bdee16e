"""The p-pairs, raw descriptions and hierarchies of the p-multigrid tests (test infrastructure): one list for the CPU tests of the host-only
planner and the NumPy restatement (tests/pmg_ref.py on oracle-assembled matrices) and for the GPU tests of the kernels and the V-cycle
(on the matrices read back from the device), with the bounds the device is held to and the figures `python tests/ptransfer_cases.py`
measured on the CPU."""
import functools

import numpy as np

ALL_PAIRS = [(q, p) for p in range(2, 8) for q in range(1, p)]  # (coarse degree, fine degree): 21
EXACT_PAIRS = [(1, 2), (2, 3), (1, 3), (3, 4), (6, 7)]

# raw descriptions of the GPU transfer tests: (dim, basis, q, p)
RAW_PAIRS = [(2, "dgq", q, p) for q, p in [(1, 2), (2, 3), (1, 3), (6, 7), (1, 7)]] + \
            [(3, "dgq", q, p) for q, p in [(1, 2), (2, 3), (1, 3), (3, 4), (2, 5), (6, 7)]] + \
            [(2, "dgp", q, p) for q, p in [(1, 2), (2, 3), (1, 3)]] + \
            [(3, "dgp", q, p) for q, p in [(1, 2), (2, 3), (3, 5), (6, 7)]]
RAW_COUNTS = [1, 7, 33]  # polytopes: below, and no multiples of, every number of polytopes a wave takes (64 // n_f = 1 .. 7)
N_F = {(3, "dgq", 4): 125, (3, "dgq", 5): 216, (3, "dgq", 7): 512, (3, "dgp", 5): 56, (3, "dgp", 7): 120}  # what the list is there for


def raw_id(c):
    return "%dD_%s_%dto%d" % c


def n_dofs(dim, basis, degree):
    import math
    return (degree + 1) ** dim if basis == "dgq" else math.comb(degree + dim, dim)


def raw_desc(dim, basis, q, p, count):
    """_capi.PTransferDesc of `count` polytopes in a permuted order, with gaps between the dof ranges and before the first, on both levels"""
    import polydeal_amd as pa
    from polydeal_amd._capi import PTransferDesc

    n_f, n_c = n_dofs(dim, basis, p), n_dofs(dim, basis, q)
    assert N_F.get((dim, basis, p), n_f) == n_f
    rng = np.random.default_rng(100 * p + 10 * q + count)
    fine_off = 5 + rng.permutation(count) * (n_f + 3)
    coarse_off = 2 + rng.permutation(count) * (n_c + 1)
    return PTransferDesc(dim=dim, fine_degree=p, coarse_degree=q, basis=pa.PDH_BASIS_DGQ if basis == "dgq" else pa.PDH_BASIS_AGGLODGP,
                         fine_dof_offset=fine_off, coarse_dof_offset=coarse_off, n_fine_rows=5 + count * (n_f + 3) + 4,
                         n_coarse_rows=2 + count * (n_c + 1) + 3)


def raw_dense(dim, basis, q, p, desc):
    import pmg_ref

    return pmg_ref.dense(dim, basis, q, p, desc.fine_dof_offset, desc.coarse_dof_offset, desc.n_fine_rows, desc.n_coarse_rows)


# Hierarchies: (dim, refinements of the unit cube, [(cells per direction of a polytope, basis, degree)] coarse to fine)
HIERARCHIES = {
    "A": (2, 3, [(1, "dgq", 1), (1, "dgq", 2), (1, "dgq", 3)]),
    "B": (3, 1, [(1, "dgq", 1), (1, "dgq", 2), (1, "dgq", 3)]),
    "C": (3, 1, [(1, "dgq", 3), (1, "dgq", 4)]),                                  # fine n = 125: point Jacobi
    "D": (2, 3, [(4, "dgq", 1), (2, "dgq", 1), (2, "dgq", 2), (2, "dgq", 3)]),    # mixed: an h-pair, then two p-pairs
    "E": (3, 2, [(2, "dgq", 1), (1, "dgq", 1), (1, "dgq", 2)]),
    "F": (2, 4, [(2, "dgp", 1), (2, "dgp", 2), (2, "dgp", 3)]),
    "G": (3, 2, [(2, "dgp", 1), (2, "dgp", 2), (2, "dgp", 3)]),
}
ROWS = {"A": (256, 576, 1024), "B": (64, 216, 512), "C": (512, 1000), "D": (16, 64, 144, 256), "E": (64, 512, 1728),
        "F": (192, 384, 640), "G": (32, 80, 160)}
CPU_HIERARCHIES = ["A", "B", "D", "F", "G"]
DEGREE = 3  # of the Chebyshev smoother
# PCG iterations to rel_tol 1e-13, b = default_rng(11).standard_normal, variant_poisson_example, by tests/pcg_ref.py on oracle-assembled
# matrices: (with the p-V-cycle of pmg_ref, exact coarsest solve; with Chebyshev(3) alone on the finest level - None: not compared).
# F with one Chebyshev application as the coarsest "solve": F_CHEBYSHEV_COUNT.
PCG_COUNTS = {"A": (23, 141), "B": (24, 45), "C": (29, 65), "D": (25, None), "E": (33, None), "F": (32, 159), "G": (18, 30)}
F_CHEBYSHEV_COUNT = 56


def inner_kind(n):
    return "block_jacobi" if n <= 64 else "jacobi"


@functools.lru_cache(maxsize=None)
def handlers(name):
    """([handlers of the host mirror, coarse to fine], [handlers of the oracle on the same grid]); no GPU"""
    import polydeal_amd as pa
    from oracle import polydeal_oracle as po

    dim, lg, levels = HIERARCHIES[name]
    grid_o = po.hyper_cube_refined(dim, 0.0, 1.0, lg)
    grid = pa.BackgroundGrid.hyper_cube_refined(dim, 0.0, 1.0, lg)
    mirror, oracles = [], []
    for b, basis, p in levels:
        ah = pa.AgglomerationHandler(grid)
        ah.define_block_agglomerates(b)
        ah.initialize_fe_values(p + 1, p + 1)
        ah.distribute_agglomerated_dofs((pa.FE_DGQ if basis == "dgq" else pa.FE_AggloDGP)(dim, p))
        mirror.append(ah)
        ao = po.AgglomerationHandler(grid_o)
        for g in po.block_agglomerates(grid_o, b):
            ao.define_agglomerate(g)
        ao.initialize_fe_values(p + 1, p + 1)
        ao.distribute_agglomerated_dofs((po.FE_DGQ if basis == "dgq" else po.FE_AggloDGP)(dim, p))
        oracles.append(ao)
    assert tuple(ah.n_dofs for ah in mirror) == ROWS[name], (name, [ah.n_dofs for ah in mirror])
    return mirror, oracles


@functools.lru_cache(maxsize=None)
def injections(name):
    """[P_l]: the dense injection between level l and l + 1 from the oracle alone (shared: do not write to them): pmg_ref.dense for a
    p-pair, the oracle's fill_injection_matrix for an h-pair"""
    import pmg_ref
    from oracle import polydeal_oracle as po

    dim, _, levels = HIERARCHIES[name]
    _, oracles = handlers(name)
    out = []
    for (bc, basis, q), (bf, _, p), c, f in zip(levels, levels[1:], oracles, oracles[1:]):
        if q == p:
            P = po.fill_injection_matrix(c, f)
        else:
            assert bc == bf and c.n_agglomerates == f.n_agglomerates
            P = pmg_ref.dense(dim, basis, q, p, [f.dof_indices(a)[0] for a in range(f.n_agglomerates)],
                              [c.dof_indices(a)[0] for a in range(c.n_agglomerates)], f.n_dofs, c.n_dofs)
        P.setflags(write=False)
        out.append(P)
    return out


def level_ns(name):
    dim, _, levels = HIERARCHIES[name]
    return [n_dofs(dim, basis, p) for _, basis, p in levels]


def _oracle_matrix(ao):
    import scipy.sparse as sp
    from oracle import polydeal_oracle as po

    rp, ci, va = po.assemble_csr(ao, po.variant_poisson_example(ao.fe), diag_first=False)
    return sp.csr_matrix((va, ci, rp), shape=(ao.n_dofs, ao.n_dofs))


@functools.lru_cache(maxsize=None)
def oracle_hierarchy(name, coarse="direct"):
    """pmg_ref.Hierarchy of a case from the NumPy oracle alone (variant_poisson_example per level), smoother bounds from cheb_ref's estimate"""
    import pmg_ref

    _, oracles = handlers(name)
    mats = [_oracle_matrix(ao) for ao in oracles]
    ns = level_ns(name)
    kinds = [inner_kind(n) for n in ns]
    return pmg_ref.Hierarchy(mats, ns, injections(name), pmg_ref.smoother_bounds(mats, ns, kinds), DEGREE, kinds, coarse)


def rhs(N):
    return np.random.default_rng(11).standard_normal(N)


# Rounding of the yardsticks themselves, measured on the CPU by python tests/ptransfer_cases.py (measure below):
#   MATRIX_1D_SPREAD  the oracle's product form of the 1-D matrix (pmg_ref.matrix_1d) against the same product in numpy.longdouble on
#                     long-double Gauss-Lobatto nodes (Newton-polished in long double), the largest |B64 - Bld| over the pairs with p = 7
#   CYCLE_SPREAD      pmg_ref.cycle in float64 against numpy.longdouble on hierarchies A - G (F with both coarsest kinds), three V-cycles
#                     from x = 0: the largest |x64 - xld|_inf / |xld|_inf
MATRIX_1D_SPREAD = 7.842e-16  # (q = 6: the product form loses its digits in the differences of neighbouring nodes)
CYCLE_SPREAD = 1.918e-14      # worst: F with the direct coarsest solve
# pdh_ptransfer_matrix_1d is held to 1e-14 (the bound of the h-transfer factors), or to 100 x the spread of the oracle's own form where
# that is further than 1e-16 from the long-double evaluation
MATRIX_1D_TOL = 1e-14 if MATRIX_1D_SPREAD <= 1e-16 else 100 * MATRIX_1D_SPREAD
# the construction of vcycle_cases.CYCLE_TOL: the device sums in another order; the V-cycle test adds 10 cond_2(A_0) 2.2e-16
CYCLE_TOL = max(100 * CYCLE_SPREAD, 1e-13)


def _nodes_longdouble(p):
    from oracle import polydeal_oracle as po

    LD = np.longdouble
    x = 2 * po.gauss_lobatto_nodes(p).astype(LD) - 1
    if p >= 2:
        inner = x[1:-1]
        for _ in range(3):  # Newton on P_p' with the recurrences in long double
            p0, p1 = np.ones_like(inner), inner.copy()
            for k in range(1, p):
                p0, p1 = p1, ((2 * k + 1) * inner * p1 - k * p0) / (k + 1)
            dP = p * (p0 - inner * p1) / (1 - inner * inner)
            d2P = (2 * inner * dP - p * (p + 1) * p1) / (1 - inner * inner)
            inner = inner - dP / d2P
        x[1:-1] = inner
    return (x + 1) / 2


def matrix_1d_longdouble(q, p):
    LD = np.longdouble
    nq, npp = _nodes_longdouble(q), _nodes_longdouble(p)
    B = np.ones((p + 1, q + 1), dtype=LD)
    for j in range(q + 1):
        for m in range(q + 1):
            if m != j:
                B[:, j] *= (npp - nq[m]) / (nq[j] - nq[m])
    return B


def measure(verbose=True):
    import pmg_ref

    LD = np.longdouble
    wm = 0.0
    for q in range(1, 7):
        wm = max(wm, float(np.max(np.abs(pmg_ref.matrix_1d(q, 7).astype(LD) - matrix_1d_longdouble(q, 7)))))
    if verbose:
        print("MATRIX_1D_SPREAD %.3e" % wm, flush=True)
    wc = 0.0
    for name, coarse in [(n, "direct") for n in HIERARCHIES] + [("F", "chebyshev")]:
        H = oracle_hierarchy(name, coarse)
        b = rhs(H.mats[-1].shape[0])
        x64, xld, spread = None, None, 0.0
        for _ in range(3):
            x64 = pmg_ref.cycle(H, b, x64)
            xld = pmg_ref.cycle(H, b, xld, dtype=LD)
            spread = max(spread, float(np.max(np.abs(x64.astype(LD) - xld)) / np.max(np.abs(xld))))
        if verbose:
            print("%s (%s): cycle spread %.3e" % (name, coarse, spread), flush=True)
        wc = max(wc, spread)
    return wm, wc


def measure_counts():
    import cheb_ref as cr
    import pcg_ref
    import pmg_ref

    for name in HIERARCHIES:
        H = oracle_hierarchy(name)
        A = H.mats[-1]
        b = rhs(A.shape[0])
        its = pcg_ref.pcg(A, b, pmg_ref.preconditioner(H), rel_tol=1e-13)[1]
        lo, hi = H.bounds[-1]
        cheb = pcg_ref.pcg(A, b, cr.chebyshev_preconditioner(A, H.ns[-1], H.kinds[-1], lo, hi, DEGREE), rel_tol=1e-13)[1]
        print("%s: p-V-cycle %d, Chebyshev(%d) alone %d" % (name, its, DEGREE, cheb), flush=True)
    H = oracle_hierarchy("F", "chebyshev")
    print("F, Chebyshev coarsest: %d" % pcg_ref.pcg(H.mats[-1], rhs(H.mats[-1].shape[0]), pmg_ref.preconditioner(H), rel_tol=1e-13)[1], flush=True)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure_counts()
    print("MATRIX_1D_SPREAD %.3e CYCLE_SPREAD %.3e" % measure())
