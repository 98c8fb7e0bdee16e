"""NumPy restatement of examples/host_solver.h's preconditioned conjugate gradients (test infrastructure): the yardstick the device
solver (pdh_solve_cg) is compared with.  Same loop - stop test before every iteration, x += alpha p, r -= alpha q, z = P^-1 r,
p = z + beta p - with an initial guess and the stop rule ||r|| <= max(abs_tol, rel_tol ||b||) of include/polydeal_hip.h."""
import numpy as np


def diag_blocks(A, n):
    """The n x n diagonal blocks of a scipy.sparse matrix whose rows come in whole polytopes of n dofs: [N / n][n][n]."""
    N = A.shape[0]
    A = A.tocsr()
    out = np.zeros((N // n, n, n))
    for B in range(N // n):
        out[B] = A[B * n:(B + 1) * n, B * n:(B + 1) * n].toarray()
    return out


def preconditioner(A, n, kind):
    """z = P^-1 r of 'none', 'jacobi' (inverse of the diagonal) or 'block_jacobi' (inverses of the n x n diagonal blocks)."""
    if kind == "none":
        return lambda r: r.copy()
    if kind == "jacobi":
        d = A.diagonal()
        return lambda r: r / d
    inv = np.linalg.inv(diag_blocks(A, n))
    return lambda r: np.einsum("bij,bj->bi", inv, r.reshape(-1, n)).ravel()


def pcg(A, b, prec, x0=None, rel_tol=1e-13, abs_tol=0.0, max_iter=20000):
    """(x, iterations, ||r||) of examples/host_solver.h's loop."""
    x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x
    z = prec(r)
    p = z.copy()
    rz = r @ z
    stop = max(abs_tol, rel_tol * np.sqrt(b @ b))
    it = 0
    while it < max_iter and np.sqrt(r @ r) > stop:
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = prec(r)
        rz1 = r @ z
        p = z + (rz1 / rz) * p
        rz = rz1
        it += 1
    return x, it, float(np.sqrt(r @ r))
