// pdh_solve.h — operator apply, preconditioners and the vector kernels of conjugate gradients on the RESIDENT matrix values
// (pdh_solve.hip).  Shared by the kernels and the C ABI (pdh_capi.cpp); the host passes this struct by value.
//
// Layout walked (pdh_plan.h: Packed): owned slot s holds the n rows of one polytope, row i at values[row_base[s] + i * row_len[s]],
// all of length row_len[s] = (number of coupled blocks) * n.  The blocks of a row are the polytope and its neighbours in ascending
// column number (col_offset or dof_offset); blk_dof[blk_ptr[s] + t] is the first GLOBAL dof of the t-th of them, so the entry at
// ascending position a = t * n + j multiplies x[blk_dof[blk_ptr[s] + t] + j] - whichever numbering orders the blocks.  diag_L[s] is
// the ascending position of the own block.  In the deal.II layout (diag_first) row i stores its diagonal entry first and the entries
// at ascending positions 0 .. diag_L + i - 1 one place later; the others stay where they are.
#pragma once
#include <stdint.h>

struct PdhSolveArgs
{
  const double *values;    // owned rows' values (pdh_device_values)
  const int64_t *row_base; // [n_owned]
  const int32_t *row_len;  // [n_owned]
  const int32_t *diag_L;   // [n_owned]
  const int32_t *own_row;  // [n_owned] first row of the slot relative to the owned row range
  const int64_t *blk_ptr;  // [n_owned + 1]
  const int32_t *blk_dof;  // [blk_ptr[n_owned]] first global dof of every block, in value order
  int32_t n, diag_first, n_owned, max_row_len;
};

// scalars of one CG run in device memory (pdh_launch_cg_finalise writes them, the vector kernels read alpha / beta)
enum PdhCgScalar
{
  PDH_CG_RZ = 0,    // r^T z of the current residual
  PDH_CG_PQ = 1,    // p^T A p
  PDH_CG_ALPHA = 2, // rz / pq
  PDH_CG_BETA = 3,  // rz_new / rz_old
  PDH_CG_RR = 4,    // r^T r   (the stop test; read back by the host)
  PDH_CG_BB = 5,    // b^T b   (first stage only)
  PDH_CG_NSCALARS = 8
};
// per-slot partial sums: [PDH_CG_NPART][n_owned]
enum PdhCgPartial
{
  PDH_PART_PQ = 0,
  PDH_PART_RZ = 1,
  PDH_PART_RR = 2,
  PDH_PART_BB = 3,
  PDH_CG_NPART = 4
};
// (the Chebyshev chain - pdh_launch_cheb_update - takes its coefficients as kernel arguments and writes only PDH_PART_RZ, on its last
// step inside CG; it reads no scalar)
// modes of the fused vector kernel pdh_launch_cg_update
enum PdhCgMode
{
  PDH_UPD_APPLY = 0, // z = P^-1 r
  PDH_UPD_INIT = 1,  // r = b - q, z = P^-1 r; partials of r^T z, r^T r, b^T b
  PDH_UPD_STEP = 2   // x += alpha p, r -= alpha q, z = P^-1 r; partials of r^T z, r^T r
};
