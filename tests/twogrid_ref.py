"""NumPy restatement of polydeal_amd.levels.two_grid_cycle_device (test infrastructure): pre-smoothing by tests/cheb_ref.py's Chebyshev
application over block Jacobi, residual, restriction by the dense injection, a dense coarse solve, prolongation, post-smoothing.  Every
routine takes a dtype like cheb_ref: numpy.float64 is the yardstick, numpy.longdouble measures the yardstick's own rounding."""
import numpy as np

import cheb_ref as cr


def coarse_solver(Ac, dtype=np.float64):
    """rc -> A_c^-1 rc with the dense coarse matrix (long double: inverted by cheb_ref's Gauss-Jordan, numpy.linalg has none)"""
    D = np.asarray(Ac.todense())
    if dtype == np.float64:
        return lambda rc: np.linalg.solve(D, rc)
    inv = cr.batched_inverse(D[None], dtype)[0]
    return lambda rc: inv @ rc


def cycle(Af, Ac, n, P, lo, hi, degree, b, x, dtype=np.float64, kind="block_jacobi"):
    """one two-grid cycle on x; lo / hi: the smoother's eigenvalue bounds on the fine level"""
    mv, solve = cr.operator(Af, dtype), coarse_solver(Ac, dtype)
    Pd = np.asarray(P, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    x = cr.apply(Af, n, kind, lo, hi, degree, b, np.asarray(x, dtype=dtype), dtype=dtype)
    r = b - mv(x)
    x = x + Pd @ solve(Pd.T @ r)
    return cr.apply(Af, n, kind, lo, hi, degree, b, x, dtype=dtype)


def residual_norm(Af, b, x):
    return float(np.linalg.norm(b - Af @ x))
