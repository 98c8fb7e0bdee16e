// pdh_dense.h — the dense direct solve on the resident matrix (pdh_dense.hip; C ABI: pdh_setup_direct, PDH_PREC_DIRECT): the coarse
// solver of a multigrid hierarchy, the reference's MGCoarseDirect.  Shared by the kernels and the driver (pdh_capi_solve.cpp).
//
// A context that owns all N <= PDH_DENSE_MAX_ROWS rows keeps the explicit inverse G = A^-1 as a dense array of leading dimension
// ld = N rounded up to a multiple of PDH_DENSE_TILE, so that every row is a whole number of 512-byte pieces; rows and columns N .. ld - 1
// are those of the identity, whatever is read there multiplies a zero.  The set-up runs on the device, queued on one stream:
//   gather      D = A, dense, from the resident rows (one wave per polytope; pdh_solve.h's layout, the diagonal-first shift undone)
//   cholesky    A = L L^T in place in the upper triangle (U = L^T, U[k][c] = L[c][k]); the diagonal of L goes to dg, U[k][k] keeps the
//               pivot (the diagonal entry at its elimination step, L_kk^2)
//   tri_inverse W = L^-1, column by column
//   gram        G = W^T W, entry (i, j) = sum_{k >= max(i, j)} W[k][i] W[k][j] in ascending k, computed once for i >= j and stored
//               at (i, j) and (j, i): G is exactly symmetric
// Every sum has a fixed order and there are no atomics: the same values give the same G.
#pragma once
#include <stdint.h>

#define PDH_DENSE_MAX_ROWS 1024 // one workgroup factors the matrix, a thread per column
#define PDH_DENSE_TILE 64       // doubles per row piece (one wave's load)

static inline int pdh_dense_ld(int64_t n_rows) { return (int)((n_rows + PDH_DENSE_TILE - 1) / PDH_DENSE_TILE * PDH_DENSE_TILE); }
