// pdh_dist.h — solving over several ranks: the halo of a rank's local vector (include/polydeal_hip.h: pdh_halo_*, pdh_vmult_local_device,
// pdh_dcg_*).  The plan is host-only (pdh_halo_plan.cpp, plain C++: pdh_check_halo runs it on machines without a GPU); the kernels that
// follow it are pdh_dist.hip, the driver pdh_capi_dist.cpp.
//
// A rank owns the rows [row_begin, row_end).  Its LOCAL VECTOR holds the owned rows in order, then one block of n doubles per distinct
// ghost polytope, ascending by first global dof - grouped by owning rank in rank order, because ranks own contiguous ranges.  The plan
// turns the block lists of the owned slots (pdh_solve.h: blk_ptr, blk_dof) into
//   blk_loc    the same lists with LOCAL positions: dof - row_begin for an owned block, n_owned_rows + n * (rank in the tail) for a ghost
//   pack_src   per block of the send buffer (peer by peer, ascending dof inside a peer) its first entry in the owned part
//   slots      the owned slots, all / interior (every block owned) / boundary, each ascending
#pragma once
#include "../../include/polydeal_hip.h"

#include <cstdint>
#include <string>
#include <vector>

struct PdhHaloPlan
{
  int n_ranks = 0, rank = -1; // rank: the range of row_splits that is [row_begin, row_end)
  int64_t n_owned_rows = 0, n_ghost_rows = 0;
  std::vector<int64_t> send_count, recv_count; // [n_ranks] doubles
  std::vector<int64_t> pack_src;               // [sum send_count / n]
  std::vector<int32_t> blk_loc;                // [blk_ptr[n_slots]]
  std::vector<int32_t> slots_all, slots_interior, slots_boundary;
};

// slot_dof [n_slots]: first global dof of every owned slot's polytope.  PDH_EINVAL with the message in `err`: see pdh_check_halo.
int pdh_plan_halo(std::string &err, int n, int32_t row_begin, int32_t row_end, int n_slots, const int64_t *blk_ptr, const int32_t *blk_dof,
                  const int32_t *slot_dof, int n_ranks, const int32_t *row_splits, PdhHaloPlan &plan);
