// pdh_galerkin.h — the coarse level matrix as the Galerkin product A_c = P^T A_f P of two resident level matrices (pdh_galerkin.hip;
// C ABI: pdh_galerkin_device, pdh_galerkin_plan).  Shared by the kernel, the host-only planner (pdh_galerkin_plan.cpp) and the driver;
// the host passes the argument struct by value.
//
// With par() the parent map of the transfer and B_X the Kronecker injection block of fine polytope X (pdh_transfer.h),
//   A_c[C, C'] = sum over the fine blocks (F, F') with par(F) = C, par(F') = C' of  B_F^T A_f[F, F'] B_F'.
// Every fine block contributes to exactly one coarse block, and on nested face-neighbour patterns that block exists in the coarse
// level's resident rows: the product is written into the layout the coarse context already has (pdh_solve.h).  The PLAN is a CSR over
// the coarse blocks in value order (block b = blk_ptr[slot] + position): its entries are the fine blocks in ascending (fine slot, block
// position) - the summation order.  Both sides are applied by sum factorisation with the transfer's 1-D matrices.
#pragma once
#include <stdint.h>

struct PdhGalerkinArgs
{
  const double *fine_values; // the fine context's values (read) ...
  double *coarse_values;     // ... and the coarse context's (every entry written once)
  // rows of both levels (pdh_solve.h): per slot
  const int64_t *f_row_base, *c_row_base;
  const int32_t *f_row_len, *c_row_len;
  const int32_t *f_diag_L, *c_diag_L;
  const double *tab;       // [n_fine][dim][n1d][n1d] of the transfer, exact where a fine support point is a coarse one (pdh_galerkin_tables)
  const int64_t *plan_ptr; // [n_blocks + 1]
  const int32_t *plan_slot, *plan_pos; // fine slot F and block position t of every entry ...
  const int32_t *plan_col;             // ... and the fine polytope F' of the block's columns
  const int32_t *blk_slot, *blk_pos;   // [n_blocks] coarse slot and block position of every coarse block
  int32_t n_blocks, f_diag_first, c_diag_first;
};

#include <string>
#include <vector>

struct pdh_transfer_desc;
struct pdh_galerkin_level;
// What pdh_galerkin_device uploads, built on the host (pdh_galerkin_plan.cpp) after the refusals of pdh_galerkin_plan.  A failure
// returns its PDH_E* code and leaves the message in `err`.
struct PdhGalerkinPlan
{
  std::vector<int64_t> ptr;
  std::vector<int32_t> slot, pos, col, blk_slot, blk_pos;
};
// the part of a pdh_transfer_desc the planner reads (a transfer keeps host copies of these)
struct PdhGalerkinPair
{
  int dim, degree;
  int32_t n_fine, n_coarse;
  int64_t n_fine_rows, n_coarse_rows;
  const int32_t *parent, *fine_off, *coarse_off;
};
int pdh_plan_galerkin(std::string &err, const PdhGalerkinPair &T, const pdh_galerkin_level *fine, const pdh_galerkin_level *coarse,
                      PdhGalerkinPlan &plan);
// The 1-D matrices the product applies: those of the transfer (n_matrices = n_fine * dim of them, [n1d][n1d] each) with every row that
// is a unit vector to rounding made that unit vector - the structural zeros of P^T A P stay zeros.  out may be tab.
void pdh_galerkin_tables(int n1d, size_t n_matrices, const double *tab, double *out);
