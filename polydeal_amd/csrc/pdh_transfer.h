// pdh_transfer.h — level transfer between two nested polytopal FE_DGQ spaces (pdh_transfer.hip; C ABI: pdh_transfer_create,
// pdh_prolongate*, pdh_restrict*).  Shared by the kernels, the host-only planner (pdh_transfer_plan.cpp) and the driver; the host passes
// the argument struct by value.
//
// FE_DGQ lives on the bounding box and the support points of a fine polytope F are a tensor grid in ITS box, so the injection block
// (F, parent C) is the Kronecker product of `dim` one-dimensional n1d x n1d matrices
//   B_c[i][j] = l_j((lo_F[c] + node_i h_F[c] - lo_C[c]) / h_C[c]),      l_j the Lagrange polynomials on the Gauss-Lobatto nodes,
// first axis fastest in the multi-index (pdh::multi_indices).  tab holds them as [n_fine][dim][n1d][n1d]: dim n1d^2 doubles per fine
// polytope instead of the n^2 of the block; the kernels apply them axis by axis (sum factorisation).
#pragma once
#include <stdint.h>

struct PdhTransferArgs
{
  const double *tab;         // [n_fine][dim][n1d][n1d]  B_c[i][j], row i = fine node, column j = coarse function
  const int32_t *parent;     // [n_fine] coarse polytope of every fine one
  const int32_t *child_ptr;  // [n_coarse + 1] children CSR ...
  const int32_t *child_idx;  // [n_fine] ... in ascending fine index per parent: the summation order of the restriction
  const int32_t *fine_off;   // [n_fine] first dof of every fine polytope in the fine vector
  const int32_t *coarse_off; // [n_coarse] first dof of every coarse polytope in the coarse vector
  int32_t n_fine, n_coarse;
};

#include <string>
#include <vector>

struct pdh_transfer_desc;
// What pdh_transfer_create uploads, built on the host (pdh_transfer_plan.cpp) after pdh_check_transfer's refusals.  A failure returns its
// PDH_E* code and leaves the message in `err`.
struct PdhTransferPlan
{
  std::vector<double> tab;
  std::vector<int32_t> child_ptr, child_idx;
};
int pdh_plan_transfer(std::string &err, const pdh_transfer_desc *d, PdhTransferPlan &plan);
