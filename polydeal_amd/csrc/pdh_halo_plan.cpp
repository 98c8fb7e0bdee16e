// pdh_halo_plan.cpp — the host-only planner of a rank's vector halo (pdh_dist.h) and pdh_check_halo.  Plain C++ like pdh_galerkin_plan.cpp:
// no HIP header, no HIP call.  Every index the kernels of pdh_dist.hip follow is checked here, before anything is uploaded.
#include "pdh_dist.h"

#include "pdh_basis.h"
#include "pdh_plan_internal.h"

#include <algorithm>

int pdh_plan_halo(std::string &err, int n, int32_t row_begin, int32_t row_end, int n_slots, const int64_t *blk_ptr, const int32_t *blk_dof,
                  const int32_t *slot_dof, int n_ranks, const int32_t *row_splits, PdhHaloPlan &plan)
{
  plan = PdhHaloPlan{};
  if (n_ranks < 1 || !row_splits)
    return fail(err, PDH_EINVAL, "halo: n_ranks must be at least 1 and row_splits [n_ranks + 1] is required");
  for (int r = 0; r < n_ranks; ++r)
    if (row_splits[r] > row_splits[r + 1])
      return fail(err, PDH_EINVAL, "halo: row_splits are not ascending at rank " + std::to_string(r) + " (" + std::to_string(row_splits[r]) +
                                     " > " + std::to_string(row_splits[r + 1]) + ")");
  int me = -1;
  for (int r = 0; r < n_ranks && me < 0; ++r)
    if (row_splits[r] == row_begin && row_splits[r + 1] == row_end)
      me = r;
  if (me < 0)
    return fail(err, PDH_EINVAL, "halo: no range of row_splits is the owned range [" + std::to_string(row_begin) + ", " +
                                   std::to_string(row_end) + ")");
  // rank of a polytope from its first dof: the last range that starts at or before it (empty ranges own nothing)
  auto owner_of = [&](int32_t dof, int &rank) {
    if (dof < row_splits[0] || dof >= row_splits[n_ranks])
      return fail(err, PDH_EINVAL, "halo: the block at dof " + std::to_string(dof) + " lies in no range of row_splits [" +
                                     std::to_string(row_splits[0]) + ", " + std::to_string(row_splits[n_ranks]) + ")");
    rank = (int)(std::upper_bound(row_splits, row_splits + n_ranks + 1, dof) - row_splits) - 1;
    if ((int64_t)dof + n > row_splits[rank + 1])
      return fail(err, PDH_EINVAL, "halo: row_splits cut the polytope at dofs [" + std::to_string(dof) + ", " + std::to_string(dof + n) +
                                     "): rank " + std::to_string(rank) + " ends at " + std::to_string(row_splits[rank + 1]));
    return PDH_OK;
  };
  plan.n_ranks = n_ranks;
  plan.rank = me;
  plan.n_owned_rows = (int64_t)row_end - row_begin;
  plan.send_count.assign((size_t)n_ranks, 0);
  plan.recv_count.assign((size_t)n_ranks, 0);

  // distinct ghost polytopes, ascending by dof (= by rank, then dof); (peer, owned dof) pairs of the send buffer
  std::vector<int32_t> ghosts;
  std::vector<std::pair<int32_t, int32_t>> sends;
  const int64_t n_blocks = n_slots > 0 ? blk_ptr[n_slots] : 0;
  std::vector<int32_t> blk_rank((size_t)n_blocks);
  for (int s = 0; s < n_slots; ++s)
    {
      int own = -1;
      PDH_TRY(owner_of(slot_dof[s], own));
      if (own != me)
        return fail(err, PDH_EINVAL, "halo: the owned polytope at dof " + std::to_string(slot_dof[s]) + " lies outside the owned range");
      bool interior = true;
      for (int64_t b = blk_ptr[s]; b < blk_ptr[s + 1]; ++b)
        {
          int r = -1;
          PDH_TRY(owner_of(blk_dof[b], r));
          blk_rank[(size_t)b] = r;
          if (r != me)
            {
              interior = false;
              ghosts.push_back(blk_dof[b]);
              sends.emplace_back(r, slot_dof[s]);
            }
        }
      plan.slots_all.push_back(s);
      (interior ? plan.slots_interior : plan.slots_boundary).push_back(s);
    }
  std::sort(ghosts.begin(), ghosts.end());
  ghosts.erase(std::unique(ghosts.begin(), ghosts.end()), ghosts.end());
  std::sort(sends.begin(), sends.end());
  sends.erase(std::unique(sends.begin(), sends.end()), sends.end());
  plan.n_ghost_rows = (int64_t)ghosts.size() * n;
  if (plan.n_owned_rows + plan.n_ghost_rows > 0x7fffffff)
    return fail(err, PDH_EUNSUPPORTED, "halo: the local vector has more than 2^31 - 1 entries");

  plan.blk_loc.resize((size_t)n_blocks);
  for (int64_t b = 0; b < n_blocks; ++b)
    {
      if (blk_rank[(size_t)b] == me)
        plan.blk_loc[(size_t)b] = blk_dof[b] - row_begin;
      else
        { // (the tail position of a ghost does not depend on the block that names it)
          const int64_t at = std::lower_bound(ghosts.begin(), ghosts.end(), blk_dof[b]) - ghosts.begin();
          plan.blk_loc[(size_t)b] = (int32_t)(plan.n_owned_rows + at * n);
        }
    }
  for (int32_t g : ghosts)
    {
      int r = -1;
      PDH_TRY(owner_of(g, r));
      plan.recv_count[(size_t)r] += n;
    }
  plan.pack_src.reserve(sends.size());
  for (const auto &sd : sends)
    {
      plan.send_count[(size_t)sd.first] += n;
      plan.pack_src.push_back((int64_t)sd.second - row_begin);
    }
  return PDH_OK;
}

// Host-only: what pdh_halo_setup would report for this description and row range.  The halo follows from the block pattern alone, so
// only the sizes, dof_offset and the face list are read (and checked): a description without its point arrays - the view
// pdh_set_problem_cartesian takes - is served like any other.
extern "C" int pdh_check_halo(const pdh_problem *p, int32_t row_begin, int32_t row_end, int n_ranks, const int32_t *row_splits,
                              int64_t *send_count, int64_t *recv_count, pdh_halo_info *info)
{
  std::string &err = pdh_noctx_error();
  err.clear();
  if (!p)
    return fail(err, PDH_EINVAL, "problem is NULL");
  if (!send_count || !recv_count || !info)
    return fail(err, PDH_EINVAL, "pdh_check_halo: send_count, recv_count and info are required");
  if (p->dim != 2 && p->dim != 3)
    return fail(err, PDH_EINVAL, "dim must be 2 or 3");
  if (p->basis != PDH_BASIS_DGQ && p->basis != PDH_BASIS_AGGLODGP)
    return fail(err, PDH_EINVAL, "unknown basis");
  if (p->degree < 0 || p->degree > 7)
    return fail(err, PDH_EUNSUPPORTED, "degree must be in [0,7]");
  if (p->n_agg <= 0 || p->n_faces < 0)
    return fail(err, PDH_EINVAL, "n_agg must be positive and n_faces non-negative");
  if (!p->dof_offset || (p->n_faces > 0 && (!p->face_in || !p->face_out)))
    return fail(err, PDH_EINVAL, "a required array is NULL");
  const int n = pdh::n_dofs_per_cell(p->dim, p->degree, p->basis), nA = p->n_agg;
  if (p->n_rows <= 0 || p->n_rows % n)
    return fail(err, PDH_EINVAL, "n_rows must be a positive multiple of dofs_per_cell");
  if (row_begin < 0 || row_end > p->n_rows || row_begin > row_end || row_begin % n || row_end % n)
    return fail(err, PDH_EINVAL, "owned row range must be aligned to whole polytopes");
  for (int a = 0; a < nA; ++a)
    if (p->dof_offset[a] < 0 || p->dof_offset[a] % n || p->dof_offset[a] + n > p->n_rows)
      return fail(err, PDH_EINVAL, "dof_offset must be a multiple of dofs_per_cell inside [0,n_rows)");
  // the blocks of every owned polytope: itself and its face neighbours, ascending by dof (the order inside a row does not enter the sizes)
  std::vector<std::vector<int32_t>> nbr((size_t)nA);
  auto owned = [&](int a) { return p->dof_offset[a] >= row_begin && p->dof_offset[a] < row_end; };
  for (int f = 0; f < p->n_faces; ++f)
    {
      const int in = p->face_in[f], out = p->face_out[f];
      if (in < 0 || in >= nA || out < -1 || out >= nA || out == in)
        return fail(err, PDH_EINVAL, "face_in/face_out out of range");
      if (out < 0)
        continue;
      if (owned(in))
        nbr[(size_t)in].push_back(p->dof_offset[out]);
      if (owned(out))
        nbr[(size_t)out].push_back(p->dof_offset[in]);
    }
  std::vector<int64_t> blk_ptr{0};
  std::vector<int32_t> blk_dof, slot_dof;
  for (int a = 0; a < nA; ++a)
    if (owned(a))
      {
        std::vector<int32_t> &b = nbr[(size_t)a];
        b.push_back(p->dof_offset[a]);
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        blk_dof.insert(blk_dof.end(), b.begin(), b.end());
        blk_ptr.push_back((int64_t)blk_dof.size());
        slot_dof.push_back(p->dof_offset[a]);
      }
  if ((int64_t)slot_dof.size() * n != (int64_t)row_end - row_begin)
    return fail(err, PDH_EINVAL, "the description does not hold every polytope of the owned row range");
  PdhHaloPlan plan;
  PDH_TRY(pdh_plan_halo(err, n, row_begin, row_end, (int)slot_dof.size(), blk_ptr.data(), blk_dof.data(), slot_dof.data(), n_ranks, row_splits,
                        plan));
  for (int r = 0; r < n_ranks; ++r)
    {
      send_count[r] = plan.send_count[(size_t)r];
      recv_count[r] = plan.recv_count[(size_t)r];
    }
  info->n_owned_rows = plan.n_owned_rows;
  info->n_ghost_rows = plan.n_ghost_rows;
  info->n_interior = (int32_t)plan.slots_interior.size();
  info->n_boundary = (int32_t)plan.slots_boundary.size();
  return PDH_OK;
}
