// pdh_shadow.h — the single-precision SHADOW of a level's matrix and of its block-Jacobi inverses (pdh_shadow.hip; C ABI:
// pdh_set_smoother_precision, pdh_smoother_vmult_device).  The Chebyshev smoother and the V-cycle residual of a level read the shadow;
// vectors, products and sums stay double, so the smoother is exactly that of the rounded matrices.
//
// Layout: slot s holds its n rows at values[base[s] + i * stride(row_len[s])], every row in ASCENDING column order whatever the layout
// of the double matrix (the conversion undoes the diagonal-first shift), padded with zeros to an even number of entries: every row
// starts on 8 bytes, the per-lane load of the product kernel.  base[s] is even too.  The block inverses are rounded entry by entry
// (they stay exactly symmetric) in the layout of the double ones, [n_owned][n][n].
#pragma once
#include "pdh_solve.h"

#include <hip/hip_runtime.h>

struct PdhShadowArgs
{
  const float *values;  // [base[n_owned - 1] + n * stride(row_len[n_owned - 1])]
  const int64_t *base;  // [n_owned] first entry of the slot's rows, computed once per problem
};

__host__ __device__ static inline int pdh_shadow_stride(int row_len) { return (row_len + 1) & ~1; }

extern "C" {
// the shadow rows of every owned slot from A->values as they stand (vector stores in address order, no read-back)
hipError_t pdh_launch_shadow_rows(const PdhSolveArgs *A, const int64_t *base, float *out, hipStream_t stream);
// out[k] = (float)in[k], k < count (the block inverses)
hipError_t pdh_launch_shadow_round(const double *in, float *out, int64_t count, hipStream_t stream);
// y[own rows] = A~ x: the structure of pdh_launch_vmult over the shadow rows, products and sums in double
hipError_t pdh_launch_vmult_f32(const PdhSolveArgs *A, const PdhShadowArgs *S, const double *x, double *y, hipStream_t stream);
// pdh_launch_cheb_update with kind = PDH_PREC_BLOCK_JACOBI reading the float inverses (n <= 64)
hipError_t pdh_launch_cheb_update_f32(const PdhSolveArgs *A, int first, const float *dinv, const double *b, const double *q, double *d,
                                      double *r, double *x, double c1, double c2, int zero_start, const double *rcg, double *part,
                                      hipStream_t stream);
}
