// pdh_ptransfer.h — transfer between two polynomial degrees q < p on the SAME polytopes (pdh_ptransfer.hip; C ABI: pdh_ptransfer_create,
// served by pdh_prolongate*, pdh_restrict*).  Shared by the kernels, the host-only planner (pdh_transfer_plan.cpp) and the driver; the host
// passes the argument struct by value.
//
// Both bases live in the unit coordinates of the polytope's box, so every polytope has the same injection block:
//   FE_DGQ       the Kronecker power (first axis fastest) of ONE (p+1) x (q+1) matrix B[i][j] = l^q_j(node^p_i); it travels in the
//                kernel arguments (at most 8 x 7 doubles), the kernels apply it axis by axis (rectangular sum factorisation);
//   FE_AggloDGP  a coarse basis function IS a fine one: an index map between the two multi-index lists.
#pragma once
#include <stdint.h>

constexpr int PDH_PTRANSFER_B_MAX = 8 * 7; // (p+1) (q+1), q < p <= 7

struct PdhPTransferArgs
{
  double B[PDH_PTRANSFER_B_MAX]; // FE_DGQ: [nf1d][nc1d], row i = fine node, column j = coarse function
  const int32_t *fine_off;       // [n_polytopes] first dof of every polytope in the fine vector
  const int32_t *coarse_off;     // [n_polytopes] ... in the coarse vector
  const int32_t *map;            // FE_AggloDGP: [n_c] fine dof of every coarse dof
  const int32_t *inv;            // FE_AggloDGP: [n_f] coarse dof of every fine dof, -1: outside the image
  int32_t n_polytopes;
  int32_t nf1d, nc1d;            // FE_DGQ: p + 1, q + 1
  int32_t n_f, n_c;              // dofs per polytope on the two levels
};

#include <string>
#include <vector>

struct pdh_ptransfer_desc;
// What pdh_ptransfer_create takes to the device, built on the host (pdh_transfer_plan.cpp) after pdh_check_ptransfer's refusals.  A failure
// returns its PDH_E* code and leaves the message in `err`.
struct PdhPTransferPlan
{
  int n_f = 0, n_c = 0;
  std::vector<double> B;         // FE_DGQ, else empty
  std::vector<int32_t> map, inv; // FE_AggloDGP, else empty
};
int pdh_plan_ptransfer(std::string &err, const pdh_ptransfer_desc *d, PdhPTransferPlan &plan);
