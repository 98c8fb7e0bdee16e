"""NumPy restatement of the single-precision smoother matrices of include/polydeal_hip.h (pdh_set_smoother_precision; test
infrastructure): the recurrences of tests/cheb_ref.py (apply) and tests/vcycle_ref.py (cycle) with the matrix of a level and its block
inverses ROUNDED to float32 and used as doubles - A~ = A.astype(float32).astype(float64) on the CSR data.  Everything else is as there:
vectors, products and sums in `dtype` (numpy.float64 is the yardstick, numpy.longdouble measures the yardstick's own rounding), the
point-Jacobi inverse and the coarsest level from the UNROUNDED matrix.

The block inverses are computed in double from the unrounded blocks (numpy.linalg.inv) and then rounded, for every dtype: what is rounded
is a double.  A double that lies within its own error of the middle between two floats rounds either way, and one float ulp is 6e-8 of
the entry - so a test of the DEVICE passes `inv64`, the double inverses the device itself stores (read back bit for bit as in
test_gpu_solve_shapes.py, and held to the long-double inverse there), and both sides round the same doubles."""
import numpy as np
import scipy.sparse as sp

import cheb_ref as cr
import vcycle_ref as vr
from pcg_ref import diag_blocks


def round32(a):
    """float64 -> float32 -> float64, element-wise (round to nearest even, as the device's conversion)"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def rounded_matrix(A):
    """A~ of a scipy sparse matrix: the same pattern, the data rounded"""
    A = A.tocsr()
    return sp.csr_matrix((round32(A.data), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def inner_preconditioner(A, n, kind, dtype=np.float64, inv64=None):
    """r -> P~^-1 r: 'jacobi' as cheb_ref (the inverse of the unrounded diagonal, a vector: it stays double), 'block_jacobi' with the
    double inverses of the unrounded blocks (inv64 [B][n][n], None: numpy.linalg.inv) rounded to float32"""
    if kind == "jacobi":
        return cr.inner_preconditioner(A, n, kind, dtype)
    assert kind == "block_jacobi", kind
    inv = round32(np.linalg.inv(diag_blocks(A, n)) if inv64 is None else inv64).astype(dtype)
    return lambda r: np.einsum("bij,bj->bi", inv, r.reshape(-1, n)).ravel()


def chebyshev(mv, prec, lo, hi, degree, b, x0=None, dtype=np.float64):
    """the recurrence of cheb_ref.apply for a given product and inner preconditioner"""
    c1, c2 = cr.coefficients(dtype(lo), dtype(hi), degree)
    b = np.asarray(b, dtype=dtype)
    if x0 is None:
        r = b.copy()
        x = np.zeros(len(b), dtype=dtype)
    else:
        x = np.array(x0, dtype=dtype)
        r = b - mv(x)
    d = c2[0] * prec(r)
    x = x + d
    for k in range(1, degree):
        r = r - mv(d)
        d = c1[k] * d + c2[k] * prec(r)
        x = x + d
    return x


class Smoother:
    """the F32 smoother of one level: product with A~ and the rounded inner inverse, built once per dtype"""

    def __init__(self, A, n, kind, dtype=np.float64, inv64=None):
        self.mv = cr.operator(rounded_matrix(A), dtype)
        self.prec = inner_preconditioner(A, n, kind, dtype, inv64)
        self.dtype = dtype

    def apply(self, lo, hi, degree, b, x0=None):
        return chebyshev(self.mv, self.prec, lo, hi, degree, b, x0, self.dtype)


def apply(A, n, kind, lo, hi, degree, b, x0=None, dtype=np.float64, inv64=None):
    """cheb_ref.apply with the rounded matrix and the rounded block inverses"""
    return Smoother(A, n, kind, dtype, inv64).apply(lo, hi, degree, b, x0)


class Hierarchy(vr.Hierarchy):
    """vcycle_ref.Hierarchy plus f32[l]: level l smooths and forms its residual with the rounded matrices (f32[0], the coarsest level, is
    not read: its solver stays double on the unrounded matrix); inv64[l]: the double block inverses of level l to round (None: NumPy's)"""

    def __init__(self, H, f32=None, inv64=None):
        super().__init__(H.mats, H.n, H.Ps, H.bounds, H.degree, H.kind, H.coarse)
        L = len(H.mats)
        self.f32 = [False] + [True] * (L - 1) if f32 is None else list(f32)
        self.inv64 = [None] * L if inv64 is None else list(inv64)
        assert len(self.f32) == L and len(self.inv64) == L
        self._sm = {}

    def smoother(self, l, dtype):
        if (l, dtype) not in self._sm:
            self._sm[(l, dtype)] = Smoother(self.mats[l], self.n, self.kind, dtype, self.inv64[l])
        return self._sm[(l, dtype)]


def cycle(H, b, x=None, dtype=np.float64, level=None):
    """vcycle_ref.cycle on a mixed_ref.Hierarchy"""
    l = len(H.mats) - 1 if level is None else level
    b = np.asarray(b, dtype=dtype)
    if l == 0:
        return H.coarse_solve(b, dtype)
    (lo, hi) = H.bounds[l]
    if H.f32[l]:
        S = H.smoother(l, dtype)
        smooth, mv = (lambda rhs, x0: S.apply(lo, hi, H.degree, rhs, x0)), S.mv
    else:
        A = H.mats[l]
        smooth, mv = (lambda rhs, x0: cr.apply(A, H.n, H.kind, lo, hi, H.degree, rhs, x0, dtype=dtype)), cr.operator(A, dtype)
    x = smooth(b, None if x is None else np.asarray(x, dtype=dtype))
    r = b - mv(x)
    Pd = np.asarray(H.Ps[l - 1], dtype=dtype)
    x = x + Pd @ cycle(H, Pd.T @ r, None, dtype, l - 1)
    return smooth(b, x)


def preconditioner(H):
    """r -> z = one mixed V-cycle from zero, for pcg_ref.pcg"""
    return lambda r: cycle(H, r)
