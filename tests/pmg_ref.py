"""NumPy restatement of p-multigrid (test infrastructure): the dense injection of a p-pair - the same polytopes at two degrees q < p -
built from the oracle alone, and the V-cycle of tests/vcycle_ref.py with a per-level element (vcycle_ref.Hierarchy has one n and one inner
preconditioner for all levels)."""
import numpy as np

import cheb_ref as cr


def index_map(dim, q, p):
    """FE_AggloDGP: the fine dof with the multi-index of every coarse dof, from the oracle's lists"""
    from oracle import polydeal_oracle as po

    fine = [tuple(m) for m in po.FE_AggloDGP(dim, p).multi_index]
    return np.array([fine.index(tuple(m)) for m in po.FE_AggloDGP(dim, q).multi_index], dtype=np.int32)


def matrix_1d(q, p):
    """FE_DGQ: [p+1][q+1], the degree-q Lagrange basis on its Gauss-Lobatto nodes at the degree-p Gauss-Lobatto nodes (oracle's product form)"""
    from oracle import polydeal_oracle as po

    return po.lagrange_1d(po.gauss_lobatto_nodes(q), po.gauss_lobatto_nodes(p))[0].T


def block(dim, basis, q, p):
    """[n_f][n_c]: the injection block every polytope has; basis 'dgq' (Kronecker power, first axis fastest) | 'dgp' (index map)"""
    if basis == "dgq":
        B = matrix_1d(q, p)
        out = B
        for _ in range(1, dim):
            out = np.kron(B, out)  # the new axis is the slower one
        return out
    m = index_map(dim, q, p)
    from oracle import polydeal_oracle as po

    out = np.zeros((po.FE_AggloDGP(dim, p).n_dofs_per_cell, len(m)))
    out[m, np.arange(len(m))] = 1.0
    return out


def dense(dim, basis, q, p, fine_off, coarse_off, n_fine_rows, n_coarse_rows):
    """dense P [n_fine_rows][n_coarse_rows]: block diagonal over the polytopes, rows outside every polytope zero"""
    blk = block(dim, basis, q, p)
    P = np.zeros((n_fine_rows, n_coarse_rows))
    for fo, co in zip(fine_off, coarse_off):
        P[int(fo):int(fo) + blk.shape[0], int(co):int(co) + blk.shape[1]] = blk
    return P


class Hierarchy:
    """vcycle_ref.Hierarchy with ns[l] dofs per polytope and kinds[l] = the inner preconditioner of the smoother per level"""

    def __init__(self, mats, ns, Ps, bounds, degree, kinds, coarse="direct"):
        assert len(Ps) == len(mats) - 1 and len(bounds) == len(mats) == len(ns) == len(kinds)
        self.mats, self.ns, self.Ps, self.bounds, self.degree, self.kinds, self.coarse = mats, ns, Ps, bounds, degree, kinds, coarse
        self._inv = {}

    def coarse_solve(self, b, dtype):
        A = self.mats[0]
        if self.coarse == "chebyshev":
            lo, hi = self.bounds[0]
            return cr.apply(A, self.ns[0], self.kinds[0], lo, hi, self.degree, b, None, dtype=dtype)
        if dtype not in self._inv:
            D = np.asarray(A.todense())
            self._inv[dtype] = np.linalg.inv(D) if dtype == np.float64 else cr.batched_inverse(D[None], dtype)[0]
        return self._inv[dtype] @ b


def cycle(H, b, x=None, dtype=np.float64, level=None):
    """vcycle_ref.cycle: one V-cycle on x (None: from zero) for the right-hand side b on `level` (None: the finest)"""
    l = len(H.mats) - 1 if level is None else level
    b = np.asarray(b, dtype=dtype)
    if l == 0:
        return H.coarse_solve(b, dtype)
    A, (lo, hi), n, kind = H.mats[l], H.bounds[l], H.ns[l], H.kinds[l]
    x = cr.apply(A, n, kind, lo, hi, H.degree, b, None if x is None else np.asarray(x, dtype=dtype), dtype=dtype)
    r = b - cr.operator(A, dtype)(x)
    Pd = np.asarray(H.Ps[l - 1], dtype=dtype)
    x = x + Pd @ cycle(H, Pd.T @ r, None, dtype, l - 1)
    return cr.apply(A, n, kind, lo, hi, H.degree, b, x, dtype=dtype)


def preconditioner(H):
    """r -> z = one V-cycle from zero, for pcg_ref.pcg"""
    return lambda r: cycle(H, r)


def smoother_bounds(mats, ns, kinds):
    return [cr.bounds(cr.estimate(A, n, kind)[0]) for A, n, kind in zip(mats, ns, kinds)]
