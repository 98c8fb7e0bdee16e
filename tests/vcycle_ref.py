"""NumPy restatement of the multigrid V-cycle of include/polydeal_hip.h (pdh_mg_create, pdh_mg_vcycle_device; test infrastructure):
recursive over tests/cheb_ref.py's Chebyshev application as the smoother, the dense injection per level pair as the transfer, and a
dense solve on the coarsest level.  Every routine takes a dtype like cheb_ref and twogrid_ref: numpy.float64 is the yardstick,
numpy.longdouble measures the yardstick's own rounding (blocks and the coarsest matrix inverted in long double too)."""
import numpy as np

import cheb_ref as cr


class Hierarchy:
    """mats: the level matrices as scipy CSR, coarse to fine; n: dofs per polytope; Ps[l]: dense injection from level l to l + 1
    ([rows of l + 1][rows of l]); bounds[l] = (lambda_lo, lambda_hi) of the smoother of level l >= 1 (bounds[0] is not read, unless
    coarse = 'chebyshev': then the coarsest level is one application from zero with bounds[0]); degree of the smoother; kind: its
    inner preconditioner."""

    def __init__(self, mats, n, Ps, bounds, degree, kind="block_jacobi", coarse="direct"):
        assert len(Ps) == len(mats) - 1 and len(bounds) == len(mats)
        self.mats, self.n, self.Ps, self.bounds, self.degree, self.kind, self.coarse = mats, n, Ps, bounds, degree, kind, coarse
        self._inv = {}

    def coarse_solve(self, b, dtype):
        A = self.mats[0]
        if self.coarse == "chebyshev":
            lo, hi = self.bounds[0]
            return cr.apply(A, self.n, self.kind, lo, hi, self.degree, b, None, dtype=dtype)
        if dtype not in self._inv:  # (long double: cheb_ref's Gauss-Jordan, numpy.linalg has none)
            D = np.asarray(A.todense())
            self._inv[dtype] = np.linalg.inv(D) if dtype == np.float64 else cr.batched_inverse(D[None], dtype)[0]
        return self._inv[dtype] @ b


def cycle(H, b, x=None, dtype=np.float64, level=None):
    """one V-cycle on x (None: from zero) for the right-hand side b on `level` (None: the finest)"""
    l = len(H.mats) - 1 if level is None else level
    b = np.asarray(b, dtype=dtype)
    if l == 0:
        return H.coarse_solve(b, dtype)
    A, (lo, hi) = H.mats[l], H.bounds[l]
    x = cr.apply(A, H.n, H.kind, lo, hi, H.degree, b, None if x is None else np.asarray(x, dtype=dtype), dtype=dtype)
    r = b - cr.operator(A, dtype)(x)
    Pd = np.asarray(H.Ps[l - 1], dtype=dtype)
    x = x + Pd @ cycle(H, Pd.T @ r, None, dtype, l - 1)
    return cr.apply(A, H.n, H.kind, lo, hi, H.degree, b, x, dtype=dtype)


def preconditioner(H):
    """r -> z = one V-cycle from zero, for pcg_ref.pcg"""
    return lambda r: cycle(H, r)


def smoother_bounds(mats, n, kind="block_jacobi"):
    """bounds of a Hierarchy from cheb_ref's own estimate on every level"""
    return [cr.bounds(cr.estimate(A, n, kind)[0]) for A in mats]


def product_longdouble(A, B, bits=21, slices=3):
    """A @ B of two float64 matrices, accurate to long double, at the speed of float64 BLAS: every row of A and every column of B is cut
    into `slices` pieces of `bits` bits below the power of two above its largest entry (integers times a power of two - the cuts are
    exact, and 3 x 21 bits hold a whole double next to the largest entry); a product of two pieces sums K products of integers below
    2^bits, exact in float64 while 2 bits + log2(K) <= 53; the slices x slices partial products are added in long double, smallest first.
    What is dropped lies 2^-63 below the largest entry of a row or column."""
    LD = np.longdouble
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert 2 * bits + int(np.ceil(np.log2(max(A.shape[1], 2)))) <= 53

    def cut(M, axis):
        top = np.max(np.abs(M), axis=axis, keepdims=True)
        e = np.where(top > 0, np.floor(np.log2(np.where(top > 0, top, 1.0))) + 1, 0.0)  # |M| < 2^e along the axis
        rem, out = M.copy(), []
        for k in range(slices):
            piece = np.ldexp(np.round(np.ldexp(rem, (bits * (k + 1) - e).astype(np.int64))), (e - bits * (k + 1)).astype(np.int64))
            rem = rem - piece
            out.append(piece)
        return out
    As, Bs = cut(A, 1), cut(B, 0)
    total = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for order in range(2 * slices - 2, -1, -1):  # smallest partial products first
        for k in range(slices):
            l = order - k
            if 0 <= l < slices:
                total += (As[k] @ Bs[l]).astype(LD)
    return total


def inverse_longdouble(D, cols=None):
    """columns `cols` (None: all) of the inverse of the dense SPD matrix D in long double: numpy.linalg.inv's answer X plus ONE step of
    iterative refinement with the residual E - D X formed to long double accuracy (product_longdouble) - the error of X is ~ cond(D) 1e-16
    of it, that of the refined answer the square of that, below the 5e-20 of the format for every matrix of these tests (cond <= 1e7).
    A Gauss-Jordan sweep in long double (cheb_ref.batched_inverse) takes minutes at 1024 rows."""
    LD = np.longdouble
    D = np.asarray(D, dtype=np.float64)
    N = D.shape[0]
    cols = np.arange(N) if cols is None else np.asarray(cols)
    X = np.linalg.inv(D)
    E = np.zeros((N, len(cols)), dtype=LD)
    E[cols, np.arange(len(cols))] = 1
    R = E - product_longdouble(D, X[:, cols])
    return X[:, cols].astype(LD) + (X @ R.astype(np.float64)).astype(LD)  # (the correction is ~1e-10 of X: its own rounding is far below)
