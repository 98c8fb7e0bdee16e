"""NumPy yardstick of the Galerkin product of include/polydeal_hip.h (pdh_galerkin_device; test infrastructure): P^T A P from the dense
injection and a given fine matrix, in float64 and to long double accuracy, the sum of absolute products the device is held to, and the
brute-force plan the host planner is compared against."""
import numpy as np

LD = np.longdouble
TOL = 1e-13  # of (|P|^T |A| |P|)_ij: the project's bound of a sum against the sum of its absolute products (k_vmult, the transfers)


def dense(A):
    return np.asarray(A.todense()) if hasattr(A, "todense") else np.asarray(A)


def product(P, A):
    """P^T A P in float64 (BLAS order)"""
    P, A = np.asarray(P, dtype=np.float64), dense(A).astype(np.float64)
    return P.T @ (A @ P)


def abs_product(P, A):
    """(|P|^T |A| |P|)_ij: what every entry's rounding is measured against"""
    P, A = np.abs(np.asarray(P, dtype=np.float64)), np.abs(dense(A).astype(np.float64))
    return P.T @ (A @ P)


def product_longdouble(P, A, desc):
    """P^T A P in long double, every entry to the accuracy of ITS OWN sum of absolute products (a split float64 product is accurate to
    the largest entry of a row only, and the injection has entries of 1e-17 where a Lagrange polynomial vanishes at a node).  Block by
    block like the device, which keeps it affordable: P of a description (_capi.TransferDesc) has one n x n block per fine polytope, in
    its parent's columns - asserted - so P^T A P = sum over the fine blocks (F, F') of B_F^T A[F, F'] B_F'."""
    import scipy.sparse as sp

    n = desc.n
    f_off, c_off, parent = (np.asarray(a, dtype=np.int64) for a in (desc.fine_dof_offset, desc.coarse_dof_offset, desc.parent))
    P = np.asarray(P, dtype=np.float64)
    blocks = [P[f_off[F]:f_off[F] + n, c_off[parent[F]]:c_off[parent[F]] + n].astype(LD) for F in range(len(f_off))]
    rest = P.copy()
    for F in range(len(f_off)):
        rest[f_off[F]:f_off[F] + n, c_off[parent[F]]:c_off[parent[F]] + n] = 0.0
    assert not rest.any(), "the injection has entries outside the blocks (fine polytope, parent)"
    A = sp.csr_matrix(A)
    poly_of_row = np.full(A.shape[0], -1, dtype=np.int64)
    for F, o in enumerate(f_off):
        poly_of_row[o:o + n] = F
    G = np.zeros((P.shape[1], P.shape[1]), dtype=LD)
    for F in range(len(f_off)):
        rows = A[f_off[F]:f_off[F] + n]
        dense_rows = None
        for F2 in np.unique(poly_of_row[rows.indices]):
            assert F2 >= 0
            if dense_rows is None:
                dense_rows = rows.toarray()
            T = dense_rows[:, f_off[F2]:f_off[F2] + n].astype(LD)
            C, C2 = parent[F], parent[F2]
            G[c_off[C]:c_off[C] + n, c_off[C2]:c_off[C2] + n] += blocks[F].T @ (T @ blocks[F2])
    return G


def chain(Ps, A_fine, descs=None):
    """[A_0, .., A_L = A_fine] with A_l = P_l^T A_(l+1) P_l, float64 matrices between the levels; descs (one per pair): every product in
    long double (product_longdouble) and rounded once, else in float64"""
    mats = [dense(A_fine).astype(np.float64)]
    for l in range(len(Ps) - 1, -1, -1):
        G = product(Ps[l], mats[0]) if descs is None else product_longdouble(Ps[l], mats[0], descs[l])
        mats.insert(0, np.asarray(G, dtype=np.float64))
    return mats


def block_pattern(M, n, threshold):
    """{(I, J)}: the n x n blocks of the dense matrix M with an entry above `threshold` in absolute value"""
    nb = M.shape[0] // n
    big = np.abs(M).reshape(nb, n, M.shape[1] // n, n).max(axis=(1, 3)) > threshold
    return {(int(i), int(j)) for i, j in zip(*np.nonzero(big))}


def block_lists(pattern, dof_offset, order_key=None):
    """(blk_ptr, blk_dof) of a level from its block pattern {(polytope, polytope)}: the blocks of a polytope's rows in ascending
    order_key (None: dof_offset - the other ordering of pdh_problem is col_offset), blk_dof = the first dof of each"""
    off = np.asarray(dof_offset, dtype=np.int64)
    key = off if order_key is None else np.asarray(order_key, dtype=np.int64)
    ptr, dof = [0], []
    for I in range(len(off)):
        cols = sorted((J for (i, J) in pattern if i == I), key=lambda J: key[J])
        dof += [int(off[J]) for J in cols]
        ptr.append(len(dof))
    return np.array(ptr, dtype=np.int64), np.array(dof, dtype=np.int32)


def brute_force_plan(parent, fine_lists, fine_off, coarse_lists, coarse_off):
    """[[(fine slot, block position)] per coarse block in value order]: every fine block under the coarse block of its parents, fine
    blocks visited in ascending (slot, position)"""
    f_ptr, f_dof = fine_lists
    c_ptr, c_dof = coarse_lists
    f_at = {int(o): F for F, o in enumerate(fine_off)}
    out = [[] for _ in range(int(c_ptr[-1]))]
    for F in range(len(fine_off)):
        C = int(parent[F])
        for t in range(int(f_ptr[F + 1] - f_ptr[F])):
            C2 = int(parent[f_at[int(f_dof[f_ptr[F] + t])]])
            row = [int(d) for d in c_dof[c_ptr[C]:c_ptr[C + 1]]]
            out[int(c_ptr[C]) + row.index(int(coarse_off[C2]))].append((F, t))
    return out
