"""NumPy restatement of the Chebyshev smoother / preconditioner of include/polydeal_hip.h (pdh_setup_chebyshev; test infrastructure),
built on pcg_ref.preconditioner: the eigenvalue estimate (Lanczos tridiagonal of P-preconditioned CG on the fixed vector b0) and one
application of the degree-m polynomial.  Every routine takes a dtype: numpy.float64 is the yardstick, numpy.longdouble measures the
yardstick's own rounding (the matrix is then used as a dense array, scipy has no long double product)."""
import numpy as np

from pcg_ref import diag_blocks


def b0(N, dtype=np.float64):
    """b0[i] = ((2654435761 i) mod 2^32) / 2^32 - 1/2, exact in double"""
    i = np.arange(N, dtype=np.uint64)
    return (((np.uint64(2654435761) * i) % np.uint64(1 << 32)).astype(np.float64) / 4294967296.0 - 0.5).astype(dtype)


def operator(A, dtype=np.float64):
    """x -> A x in dtype"""
    if dtype == np.float64:
        return lambda x: A @ x
    D = np.asarray(A.todense()).astype(dtype)
    return lambda x: D @ x


def batched_inverse(blocks, dtype):
    """inverses of SPD blocks [B][n][n] in dtype by Gauss-Jordan elimination without pivoting (numpy.linalg has no long double)"""
    M = np.array(blocks, dtype=dtype)
    B, n, _ = M.shape
    M = np.concatenate([M, np.broadcast_to(np.eye(n, dtype=dtype), (B, n, n))], axis=2)
    for k in range(n):
        M[:, k, :] = M[:, k, :] / M[:, k, k:k + 1]
        f = M[:, :, k].copy()
        f[:, k] = 0
        M -= f[:, :, None] * M[:, k:k + 1, :]
    return M[:, :, n:]


def inner_preconditioner(A, n, kind, dtype=np.float64):
    """pcg_ref.preconditioner for 'jacobi' | 'block_jacobi' in dtype; the long double run inverts the blocks in long double too, so
    the spread between the two runs includes what the conditioning of the blocks does to a double inverse"""
    if kind == "jacobi":
        d = A.diagonal().astype(dtype)
        return lambda r: r / d
    assert kind == "block_jacobi", kind
    inv = np.linalg.inv(diag_blocks(A, n)) if dtype == np.float64 else batched_inverse(diag_blocks(A, n), dtype)
    return lambda r: np.einsum("bij,bj->bi", inv, r.reshape(-1, n)).ravel()


def lanczos_tridiagonal(alpha, beta):
    """T_jj = 1 / alpha_j + beta_(j-1) / alpha_(j-1), T_(j,j+1) = sqrt(beta_j) / alpha_j"""
    k = len(alpha)
    diag = np.array([1 / alpha[j] + (beta[j - 1] / alpha[j - 1] if j else 0) for j in range(k)], dtype=np.asarray(alpha).dtype)
    off = np.array([np.sqrt(beta[j]) / alpha[j] for j in range(k - 1)], dtype=np.asarray(alpha).dtype)
    return diag, off


def cg_coefficients(mv, prec, b, k):
    """alpha_j, beta_j of k steps of preconditioned CG on A x = b from x = 0 (the loop of pcg_ref.pcg); fewer if r reaches zero"""
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    alpha, beta = [], []
    for _ in range(k):
        if not r @ r > 0:
            break
        q = mv(p)
        a = rz / (p @ q)
        r = r - a * q
        z = prec(r)
        rz1 = r @ z
        alpha.append(a)
        beta.append(rz1 / rz)
        p = z + beta[-1] * p
        rz = rz1
    return np.array(alpha, dtype=b.dtype), np.array(beta, dtype=b.dtype)


def estimate(A, n, kind, k=20, dtype=np.float64):
    """(est, steps): largest eigenvalue of the Lanczos tridiagonal"""
    alpha, beta = cg_coefficients(operator(A, dtype), inner_preconditioner(A, n, kind, dtype), b0(A.shape[0], dtype), k)
    diag, off = lanczos_tridiagonal(alpha, beta)
    T = np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)
    if dtype == np.float64:
        return float(np.linalg.eigvalsh(T)[-1]), len(alpha)
    return eig_max_longdouble(diag, off), len(alpha)


def eig_max_longdouble(diag, off):
    """largest eigenvalue of a tridiagonal in long double: bisection on the Sturm count from eigvalsh's double answer"""
    diag, off = np.asarray(diag, dtype=np.longdouble), np.asarray(off, dtype=np.longdouble)
    k = len(diag)
    if k == 1:
        return diag[0]
    T = (np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)).astype(np.float64)
    lam = np.longdouble(np.linalg.eigvalsh(T)[-1])
    w = np.longdouble(1e-10) * abs(lam)

    def below(x):
        c, q = 0, diag[0] - x
        c += q < 0
        for i in range(1, k):
            q = diag[i] - x - off[i - 1] * off[i - 1] / (q if q != 0 else np.longdouble(1e-4000))
            c += q < 0
        return c
    a, b = lam - w, lam + w
    assert below(a) <= k - 1 < below(b)
    for _ in range(200):
        m = a + (b - a) / 2
        if not a < m < b:
            break
        if below(m) <= k - 1:
            a = m
        else:
            b = m
    return a + (b - a) / 2


def bounds(est, smoothing_range=20.0):
    """(lambda_lo, lambda_hi) of an estimate"""
    hi = 1.2 * est
    return hi / smoothing_range, hi


def coefficients(lo, hi, degree):
    """(c1[k], c2[k]): d_k = c1[k] d_(k-1) + c2[k] P^-1 r_k; c2[0] = 1 / theta, c1[0] unused.  The expressions of pdh_setup_chebyshev."""
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    sigma = theta / delta
    c1, c2 = [0 * theta], [1 / theta]
    rho_old = 1 / sigma
    for _ in range(1, degree):
        rho = 1 / (2 * sigma - rho_old)
        c1.append(rho * rho_old)
        c2.append(2 * rho / delta)
        rho_old = rho
    return c1, c2


def apply(A, n, kind, lo, hi, degree, b, x0=None, dtype=np.float64):
    """one application of degree m to b from x0 (None: zero, no product with A for r_0)"""
    mv, prec = operator(A, dtype), inner_preconditioner(A, n, kind, dtype)
    c1, c2 = coefficients(dtype(lo), dtype(hi), degree)
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


def chebyshev_preconditioner(A, n, kind, lo, hi, degree):
    """r -> z for pcg_ref.pcg"""
    return lambda r: apply(A, n, kind, lo, hi, degree, r)
