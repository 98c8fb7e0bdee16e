"""The term form of the SIP operator restated in NumPy from an ORACLE handler of Cartesian cells (test infrastructure): what the
matrix-free product of csrc/pdh_matfree.h rests on.  Per polytope P with box [lo, lo + h] and 1-D bases B_k on it (from the oracle's
fe.eval_1d), every block is a sum of Kronecker products of three 1-D matrices (csrc/pdh_terms.h, header comment):

  A[P,P] = sum over cells        K0' (x) M1 (x) M2 + M0 (x) K1 (x) M2 + M0 (x) M1 (x) K2       M_d = sum_a w_a B_k B_l,
                                                                                              K_d = sum_a w_a B'_k B'_l / h_d^2
         + sum over sub-faces    D0 (x) D1 (x) D2                                              (K0' = K0 + c M0)
  A[P,Q] = sum over the sub-faces shared with Q    X0 (x) X1 (x) X2

No merging: one term per cell and per cell face, the rules are the oracle's Gauss rules on the cell.  dense() is the matrix,
apply(x, dtype) the product by sum factorisation of every term in float64 or numpy.longdouble (the tables themselves are float64
data in both: the spread between the two is the rounding of the product alone).  FE_AggloDGP (k0 + k1 + k2 <= p) is embedded in the
full tensor with zeros; apply_truncated() is the direct sum over the index set instead."""
import numpy as np

from oracle import polydeal_oracle as po


def _cell_box(grid, cell):
    V = grid.vertices[cell]
    lo, hi = V.min(axis=0), V.max(axis=0)
    corners = np.array([[(hi if (v >> c) & 1 else lo)[c] for c in range(grid.dim)] for v in range(2 ** grid.dim)])
    assert sorted(map(tuple, np.round(V, 14))) == sorted(map(tuple, np.round(corners, 14))), "cell %d is not an axis-aligned box" % cell
    return lo, hi


class TermForm:
    def __init__(self, ah, var):
        assert ah.grid.dim == 3
        self.ah, self.var = ah, var
        fe = ah.fe
        self.N = fe.n1d
        self.n = fe.n_dofs_per_cell
        mi = np.asarray(fe.multi_index, dtype=np.int64)
        self.full_index = mi[:, 0] + self.N * mi[:, 1] + self.N * self.N * mi[:, 2]  # place of every function in the N^3 tensor
        self.own = []       # per polytope: list of (T0, T1, T2) applied to x_P
        self.coupling = []  # per polytope: list of (Q, T0, T1, T2) applied to x_Q
        for P in range(ah.n_agglomerates):
            own, cpl = self._terms(P)
            self.own.append(own)
            self.coupling.append(cpl)

    # ---- 1-D pieces -------------------------------------------------------------------------------------------------------------
    def _basis(self, P, axis, x):
        """B [N, q], dB/dx [N, q] of polytope P's 1-D basis along `axis` at real coordinates x"""
        lo, hi = self.ah.bboxes[P]
        h = hi[axis] - lo[axis]
        v, d = self.ah.fe.eval_1d((np.atleast_1d(x) - lo[axis]) / h)
        return v, d / h

    @staticmethod
    def _rule(a, b, nq):
        x1, w1 = po.qgauss_1d(nq)
        return a + (b - a) * x1, (b - a) * w1

    def _terms(self, P):
        ah, var, g = self.ah, self.var, self.ah.grid
        own, cpl = [], []
        for cell in ah.get_agglomerate(P):
            clo, chi = _cell_box(g, cell)
            M, K = [], []
            for d in range(3):
                x, w = self._rule(clo[d], chi[d], ah.nq)
                B, dB = self._basis(P, d, x)
                M.append((B * w) @ B.T)
                K.append((dB * w) @ dB.T)
            own.append((K[0] + var.reaction_c * M[0], M[1], M[2]))
            own.append((M[0], K[1], M[2]))
            own.append((M[0], M[1], K[2]))
        for f in range(ah.n_faces[P]):
            if ah.at_boundary(P, f):
                if var.boundary == "zero":
                    continue
                sig = po.face_sigma(ah, var, P)
                for cell, lf in ah.interface[(P, P)]:
                    own.append(self._face_tables(P, None, cell, lf, 2.0, 0.5 * sig)[0])
            else:
                Q = ah.neighbor(P, f)
                sig = po.face_sigma(ah, var, P, Q) if po._owns(ah, var, P, Q) else po.face_sigma(ah, var, Q, P)
                for cell, lf in ah.interface[(P, Q)]:
                    D, X = self._face_tables(P, Q, cell, lf, 1.0, sig)
                    own.append(D)
                    cpl.append((Q,) + X)
        return own, cpl

    def _face_tables(self, P, Q, cell, lf, wscale, sig):
        """(D0, D1, D2), (X0, X1, X2) of the cell face (cell, lf) of P; Q None: boundary (weights 2 JxW, sigma / 2: the same sums)"""
        ah = self.ah
        clo, chi = _cell_box(ah.grid, cell)
        c, side = lf // 2, lf % 2
        s = 1.0 if side else -1.0
        z = chi[c] if side else clo[c]
        D, X = [None] * 3, [None] * 3
        first = True
        for d in range(3):
            if d == c:
                B, dB = self._basis(P, c, z)
                B, dB = B[:, 0], dB[:, 0]
                D[c] = sig * np.outer(B, B) - 0.5 * s * (np.outer(dB, B) + np.outer(B, dB))
                if Q is not None:
                    Bq, dBq = self._basis(Q, c, z)
                    Bq, dBq = Bq[:, 0], dBq[:, 0]
                    X[c] = np.outer(0.5 * s * dB - sig * B, Bq) - 0.5 * s * np.outer(B, dBq)
            else:
                x, w = self._rule(clo[d], chi[d], ah.nqf)
                if first:  # (the factor of the boundary weights rides on one tangential direction)
                    w = w * wscale
                    first = False
                B, _ = self._basis(P, d, x)
                D[d] = (B * w) @ B.T
                if Q is not None:
                    Bq, _ = self._basis(Q, d, x)
                    X[d] = (B * w) @ Bq.T
        return tuple(D), (tuple(X) if Q is not None else None)

    # ---- the matrix -------------------------------------------------------------------------------------------------------------
    def _kron(self, T):
        idx = self.full_index
        return np.kron(T[2], np.kron(T[1], T[0]))[np.ix_(idx, idx)]

    def blocks(self):
        out = {}
        for P in range(self.ah.n_agglomerates):
            out[(P, P)] = sum(self._kron(T) for T in self.own[P])
            for Q, *T in self.coupling[P]:
                out[(P, Q)] = out.get((P, Q), 0.0) + self._kron(T)
        return out

    def dense(self):
        ah = self.ah
        A = np.zeros((ah.n_dofs, ah.n_dofs))
        for (P, Q), M in self.blocks().items():
            A[np.ix_(ah.dof_indices(P), ah.dof_indices(Q))] += M
        return A

    def csr_values(self, diag_first=True):
        """the values in the oracle's CSR layout (ah.sparsity_pattern)"""
        rp, ci = self.ah.sparsity_pattern(diag_first)
        A = self.dense()
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        return A[rows, ci]

    # ---- the product ------------------------------------------------------------------------------------------------------------
    def _factorised(self, T, xf, dtype):
        N = self.N
        X = xf.reshape(N, N, N)  # [k2][k1][k0]
        T0, T1, T2 = (np.asarray(t, dtype=dtype) for t in T)
        a = np.einsum("cz,zyx->cyx", T2, X)
        b = np.einsum("by,cyx->cbx", T1, a)
        return np.einsum("ax,cbx->cba", T0, b).reshape(-1)

    def apply(self, x, dtype=np.float64):
        """A x: every term by three passes in the full tensor, accumulated in `dtype`"""
        ah, idx = self.ah, self.full_index
        x = np.asarray(x, dtype=dtype)
        y = np.zeros(ah.n_dofs, dtype=dtype)

        def embed(P):
            xf = np.zeros(self.N ** 3, dtype=dtype)
            xf[idx] = x[ah.dof_indices(P)]
            return xf

        for P in range(ah.n_agglomerates):
            acc = np.zeros(self.N ** 3, dtype=dtype)
            xp = embed(P)
            for T in self.own[P]:
                acc += self._factorised(T, xp, dtype)
            for Q, *T in self.coupling[P]:
                acc += self._factorised(T, embed(Q), dtype)
            y[ah.dof_indices(P)] = acc[idx]
        return y

    def apply_truncated(self, x):
        """A x as the direct sum over the element's own index set (no embedding), float64"""
        ah = self.ah
        x = np.asarray(x, dtype=np.float64)
        y = np.zeros(ah.n_dofs)
        for P in range(ah.n_agglomerates):
            acc = np.zeros(self.n)
            for T in self.own[P]:
                acc += self._kron(T) @ x[ah.dof_indices(P)]
            for Q, *T in self.coupling[P]:
                acc += self._kron(T) @ x[ah.dof_indices(Q)]
            y[ah.dof_indices(P)] = acc
        return y


def row_scale(A, x):
    """sum_j |A_ij| |x_j| per row (A dense or scipy sparse)"""
    return np.asarray(abs(A) @ np.abs(x)).reshape(-1)
