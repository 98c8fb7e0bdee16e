"""Parity assertions shared by the GPU tests (BASELINE.json north_star: "matrix entries matching to 1e-12", fp64).

Two bounds, both against the oracle on identical inputs:
  * global:     max|A_gpu - A_ref| <= tol * max|A_ref|
  * per block:  for every n x n block (P, Q) of the pattern
                max|block_gpu - block_ref| <= tol * max(max|block_ref|, floor * max|A_ref|)
    - a coupling block is 10..1000 times smaller than the diagonal blocks, so the global bound alone would let it lose
    digits unnoticed; `floor` keeps blocks that vanish identically (to rounding) from asking for relative accuracy of zero.
The unit of the relative bound is the block, not the entry: an entry is a sum of terms of the size of its block's largest
entries, and that is what rounding is relative to.
"""
import numpy as np

TOL = 1e-12
FLOOR = 1e-6


def block_keys(rowptr, colind, n):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colind = np.asarray(colind, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    nbc = int(colind.max()) // n + 1 if len(colind) else 1
    return (rows // n) * nbc + colind // n


def assert_parity(got, ref, rowptr, colind, n, tol=TOL, floor=FLOOR, what=""):
    got = np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), what
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    err = np.abs(got - ref)
    gmax = float(err.max()) if err.size else 0.0
    assert gmax <= tol * scale, "%s global: max err %.3e = %.3e * max|A|" % (what, gmax, gmax / max(scale, 1e-300))
    keys = block_keys(rowptr, colind, n)
    assert keys.shape == ref.shape
    _, inv = np.unique(keys, return_inverse=True)
    nb = int(inv.max()) + 1 if inv.size else 0
    bmax = np.zeros(nb)
    berr = np.zeros(nb)
    np.maximum.at(bmax, inv, np.abs(ref))
    np.maximum.at(berr, inv, err)
    bound = tol * np.maximum(bmax, floor * scale)
    bad = np.nonzero(berr > bound)[0]
    assert bad.size == 0, "%s per block: %d of %d blocks off, worst err/bound %.3e (block max %.3e, global max %.3e)" % (
        what, bad.size, nb, float((berr / bound).max()), float(bmax[np.argmax(berr / bound)]), scale)
    return gmax / max(scale, 1e-300)


def assert_parity_ah(got, ref, ah, diag_first=True, rows=None, **kw):
    """Same, with the pattern taken from an oracle handler; rows = (r0, r1): `got` / `ref` hold the values of that row
    range only (rank-local assemblies)."""
    cache = ah.__dict__.setdefault("_sp_cache", {})
    if diag_first not in cache:
        cache[diag_first] = ah.sparsity_pattern(diag_first)
    rp, ci = cache[diag_first]
    n = ah.fe.n_dofs_per_cell
    if rows is not None:
        r0, r1 = rows
        ci = ci[rp[r0]:rp[r1]]
        rp = rp[r0:r1 + 1] - rp[r0]
    return assert_parity(got, ref, rp, ci, n, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# Vectors (right-hand side, u_h and grad u_h at points, basis values on boxes): the unit is the polytope, as the block is for
# matrices.  A polytope's entries are sums of terms of the size of ITS volume, boundary area, coefficients and box - next to a
# polytope of 8^3 cells, on a graded mesh, or for the Nitsche gradient term against the penalty term, hundreds of times below
# max|ref| - so the global bound alone would let them lose digits unnoticed.  S_P is a per-polytope scale that cancellation cannot
# shrink: the largest sum of ABSOLUTE terms of an entry of P (oracle: assemble_rhs(absolute=True), abs_eval_scales).
# ---------------------------------------------------------------------------------------------------------------------
def assert_vector_parity(got, ref, seg, scale, tol=TOL, floor=FLOOR, what=""):
    """got / ref / scale: [N] or [N, m]; seg [N]: polytope (or box) of every row.  Per column c:
      global:        max|got - ref| <= tol * max|ref|
      per polytope:  max_{i in P} |got_i - ref_i| <= tol * max(S_P, floor * max|ref|),  S_P = max_{i in P} scale_i."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.asarray(scale, dtype=np.float64)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    assert np.all(np.isfinite(got)), "%s: non-finite entries" % what
    if got.ndim == 1:
        got, ref, scale = got[:, None], ref[:, None], scale[:, None]
    seg = np.asarray(seg, dtype=np.int64)
    assert seg.shape == (got.shape[0],)
    if not seg.size:
        return 0.0
    # the scale dominates the reference entry by construction (a sum of |terms| >= |sum of terms|)
    assert np.all(scale >= (1.0 - 1e-12) * np.abs(ref)), "%s: scale below |ref|" % what
    err = np.abs(got - ref)
    nseg = int(seg.max()) + 1
    worst = 0.0
    for c in range(got.shape[1]):
        gmax = float(np.max(np.abs(ref[:, c])))
        e = float(err[:, c].max())
        assert e <= tol * gmax, "%s[%d] global: max err %.3e = %.3e * max|ref|" % (what, c, e, e / max(gmax, 1e-300))
        smax = np.zeros(nseg)
        serr = np.zeros(nseg)
        np.maximum.at(smax, seg, scale[:, c])
        np.maximum.at(serr, seg, err[:, c])
        bound = tol * np.maximum(smax, floor * gmax)
        ratio = np.where(bound > 0, serr / np.where(bound > 0, bound, 1.0), np.where(serr > 0, np.inf, 0.0))
        bad = np.nonzero(ratio > 1.0)[0]
        assert bad.size == 0, "%s[%d] per polytope: %d of %d off, worst err/bound %.3e (polytope %d: S_P %.3e, global max %.3e)" % (
            what, c, bad.size, nseg, float(ratio.max()), int(np.argmax(ratio)), float(smax[np.argmax(ratio)]), gmax)
        worst = max(worst, float(ratio.max()))
    return worst


def dof_segments(n_rows, n):
    """Polytope of every row of a vector with n contiguous dofs per polytope."""
    return np.arange(n_rows, dtype=np.int64) // n


def point_segments(pt_ptr):
    """Polytope of every point of a per-polytope CSR point list."""
    ptr = np.asarray(pt_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


def oracle_evaluate(ah, u, P, x):
    """(u_h [q], grad u_h [q, dim], scale of u_h [q], scale of grad u_h [q, dim]) of oracle polytope P at real points x:
    the scales are sum_i |c_i phi_i| and sum_i |c_i d_c phi_i| (from the oracle's shape values)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    lo, hi = ah.bboxes[P]
    val, ugrad = ah.fe.shape(ah.real_to_unit(P, x))
    grad = ugrad * (1.0 / (hi - lo))
    coef = np.asarray(u)[ah.dof_indices(P)]
    ac = np.abs(coef)
    return val @ coef, np.einsum("qic,i->qc", grad, coef), np.abs(val) @ ac, np.einsum("qic,i->qc", np.abs(grad), ac)


def shape_value_scale(fe, unit_pts):
    """[q, n]: for phi_j = prod_c B_(k_c)(x_c) at every unit point, prod_c max_k |B_k(x_c)| - the size of the 1-D functions the factors
    of phi_j are evaluated among (their rounding is relative to that, pdh_basis.h evaluates them all at once).  |phi_j| alone cannot be
    the scale: where a factor has a root (a Lagrange function at another node - the sub-cell vertices on the box faces are such
    points) it is 0 while the rounding of the factor is not.  At least 1 / (p + 1)^dim for FE_DGQ (partition of unity), 1 for
    FE_AggloDGP (B_0 = 1)."""
    unit_pts = np.atleast_2d(np.asarray(unit_pts, dtype=np.float64))
    m = np.ones(len(unit_pts))
    for c in range(unit_pts.shape[1]):
        m *= np.max(np.abs(fe.eval_1d(unit_pts[:, c])[0]), axis=0)
    return np.repeat(m[:, None], fe.n_dofs_per_cell, axis=1)
