// pdh_galerkin_plan.cpp — the host-only planner of the Galerkin product (pdh_galerkin.h): the refusals of pdh_galerkin_plan and the CSR
// over the coarse blocks that fixes which fine blocks a coarse block receives and in which order.  Plain C++ like pdh_transfer_plan.cpp:
// no HIP header, no HIP call.  Every index the kernel follows is checked here, before anything is uploaded.
#include "pdh_galerkin.h"

#include "pdh_plan_internal.h"

#include <algorithm>
#include <unordered_map>

namespace
{
// what one level contributes to the checks: `who` is "fine" or "coarse"
int check_level(std::string &err, const char *who, const pdh_galerkin_level *L, int32_t n_polytopes, int64_t n_rows, const int32_t *off)
{
  const std::string lvl = std::string("the ") + who + " level";
  if (!L || !L->blk_ptr || !L->blk_dof || !L->dof_offset)
    return fail(err, PDH_EINVAL, lvl + ": blk_ptr, blk_dof and dof_offset are required");
  if (L->exchange_mode == PDH_EXCHANGE_GHOST)
    return fail(err, PDH_EUNSUPPORTED, lvl + " was set in PDH_EXCHANGE_GHOST mode; the Galerkin product needs contexts that own all rows with "
                                             "PDH_EXCHANGE_NONE");
  if (L->n_rows_owned != L->n_rows)
    return fail(err, PDH_EUNSUPPORTED, lvl + " owns rows " + std::to_string(L->n_rows_owned) + " of " + std::to_string(L->n_rows) +
                                         "; the Galerkin product needs all rows in one context");
  if (L->n_slots != n_polytopes)
    return fail(err, PDH_EINVAL, lvl + " has " + std::to_string(L->n_slots) + " polytopes, the transfer " + std::to_string(n_polytopes));
  if (L->n_rows != n_rows)
    return fail(err, PDH_EINVAL, lvl + " has " + std::to_string(L->n_rows) + " rows, the transfer " + std::to_string(n_rows));
  for (int32_t s = 0; s < n_polytopes; ++s)
    if (L->dof_offset[s] != off[s])
      return fail(err, PDH_EINVAL, "the dof offset of " + std::string(who) + " polytope " + std::to_string(s) + " is " +
                                     std::to_string(L->dof_offset[s]) + ", the transfer's " + std::to_string(off[s]));
  if (L->blk_ptr[0] != 0)
    return fail(err, PDH_EINVAL, lvl + ": blk_ptr must start at 0");
  for (int32_t s = 0; s < n_polytopes; ++s)
    if (L->blk_ptr[s + 1] <= L->blk_ptr[s])
      return fail(err, PDH_EINVAL, lvl + ": polytope " + std::to_string(s) + " has no block");
  return PDH_OK;
}
} // namespace

int pdh_plan_galerkin(std::string &err, const PdhGalerkinPair &T, const pdh_galerkin_level *fine, const pdh_galerkin_level *coarse,
                      PdhGalerkinPlan &plan)
{
  int n = 1;
  for (int c = 0; c < T.dim; ++c)
    n *= T.degree + 1;
  if (n > 64)
    return fail(err, PDH_EUNSUPPORTED, "the Galerkin product needs at most 64 dofs per polytope, FE_DGQ(" + std::to_string(T.degree) + ") in " +
                                         std::to_string(T.dim) + "-D has " + std::to_string(n) +
                                         " (the transfers accept 3-D FE_DGQ(4..7), the product does not)");
  PDH_TRY(check_level(err, "fine", fine, T.n_fine, T.n_fine_rows, T.fine_off));
  PDH_TRY(check_level(err, "coarse", coarse, T.n_coarse, T.n_coarse_rows, T.coarse_off));
  if (fine->device != coarse->device)
    return fail(err, PDH_EUNSUPPORTED, "the fine level lives on device " + std::to_string(fine->device) + ", the coarse one on device " +
                                         std::to_string(coarse->device) + "; the Galerkin product needs both on one device");
  std::unordered_map<int32_t, int32_t> fine_at, coarse_at; // first dof -> polytope
  fine_at.reserve((size_t)T.n_fine * 2);
  for (int32_t F = 0; F < T.n_fine; ++F)
    fine_at[T.fine_off[F]] = F;
  for (int32_t C = 0; C < T.n_coarse; ++C)
    coarse_at[T.coarse_off[C]] = C;
  // the coarse blocks: (slot, position) of every block, and per slot its block dofs checked
  const int64_t n_cblk = coarse->blk_ptr[T.n_coarse], n_fblk = fine->blk_ptr[T.n_fine];
  plan.blk_slot.resize((size_t)n_cblk);
  plan.blk_pos.resize((size_t)n_cblk);
  for (int32_t C = 0; C < T.n_coarse; ++C)
    for (int64_t b = coarse->blk_ptr[C]; b < coarse->blk_ptr[C + 1]; ++b)
      {
        if (!coarse_at.count(coarse->blk_dof[b]))
          return fail(err, PDH_EINVAL, "block " + std::to_string(b - coarse->blk_ptr[C]) + " of coarse polytope " + std::to_string(C) +
                                         " starts at dof " + std::to_string(coarse->blk_dof[b]) + ", which is not the first dof of a polytope");
        plan.blk_slot[(size_t)b] = C;
        plan.blk_pos[(size_t)b] = (int32_t)(b - coarse->blk_ptr[C]);
      }
  // the coarse block of every fine block, fine blocks in ascending (slot, position)
  std::vector<int64_t> target((size_t)n_fblk);
  std::vector<int32_t> col((size_t)n_fblk);
  plan.ptr.assign((size_t)n_cblk + 1, 0);
  for (int32_t F = 0; F < T.n_fine; ++F)
    {
      const int32_t C = T.parent[F];
      if (C < 0 || C >= T.n_coarse)
        return fail(err, PDH_EINVAL, "the parent of fine polytope " + std::to_string(F) + " is out of range");
      for (int64_t b = fine->blk_ptr[F]; b < fine->blk_ptr[F + 1]; ++b)
        {
          const auto it = fine_at.find(fine->blk_dof[b]);
          if (it == fine_at.end())
            return fail(err, PDH_EINVAL, "block " + std::to_string(b - fine->blk_ptr[F]) + " of fine polytope " + std::to_string(F) +
                                           " starts at dof " + std::to_string(fine->blk_dof[b]) + ", which is not the first dof of a polytope");
          const int32_t F2 = it->second, C2 = T.parent[F2];
          if (C2 < 0 || C2 >= T.n_coarse)
            return fail(err, PDH_EINVAL, "the parent of fine polytope " + std::to_string(F2) + " is out of range");
          const int32_t want = T.coarse_off[C2];
          const int32_t *lo = coarse->blk_dof + coarse->blk_ptr[C], *hi = coarse->blk_dof + coarse->blk_ptr[C + 1];
          const int32_t *at = std::find(lo, hi, want);
          if (at == hi)
            return fail(err, PDH_EINVAL, "fine polytopes " + std::to_string(F) + " and " + std::to_string(F2) + " are coupled, their parents " +
                                           std::to_string(C) + " and " + std::to_string(C2) +
                                           " are not: the levels are not nested, or the patterns are not face-neighbour patterns");
          target[(size_t)b] = coarse->blk_ptr[C] + (at - lo);
          col[(size_t)b] = F2;
          ++plan.ptr[(size_t)target[(size_t)b] + 1];
        }
    }
  for (int64_t b = 0; b < n_cblk; ++b)
    {
      if (!plan.ptr[(size_t)b + 1])
        return fail(err, PDH_EINVAL, "block " + std::to_string(plan.blk_pos[(size_t)b]) + " of coarse polytope " +
                                       std::to_string(plan.blk_slot[(size_t)b]) + " receives no contribution from the fine level");
      plan.ptr[(size_t)b + 1] += plan.ptr[(size_t)b];
    }
  plan.slot.resize((size_t)n_fblk);
  plan.pos.resize((size_t)n_fblk);
  plan.col.resize((size_t)n_fblk);
  std::vector<int64_t> at(plan.ptr.begin(), plan.ptr.end() - 1);
  for (int32_t F = 0; F < T.n_fine; ++F) // ascending (F, position): that order inside every coarse block
    for (int64_t b = fine->blk_ptr[F]; b < fine->blk_ptr[F + 1]; ++b)
      {
        const int64_t e = at[(size_t)target[(size_t)b]]++;
        plan.slot[(size_t)e] = F;
        plan.pos[(size_t)e] = (int32_t)(b - fine->blk_ptr[F]);
        plan.col[(size_t)e] = col[(size_t)b];
      }
  return PDH_OK;
}

// A row of a 1-D interpolation matrix that lies within 64 ulp of a unit vector belongs to a fine support point that IS a coarse one (the
// rows sum to 1 and the Lagrange polynomials are continuous; a point computed in double misses its node by a few ulp, which their slope,
// at most N1D^2, carries into the row): the exact row is the unit vector.  The long-double Horner form of pdh_transfer_matrices_1d leaves
// 1e-19 .. 1e-17 in the zeros - nothing to a transfer, which is held to the sum of its absolute products, but in P^T A P those are the
// whole of an entry that is structurally zero.
void pdh_galerkin_tables(int n1d, size_t n_matrices, const double *tab, double *out)
{
  const double tol = 64 * 2.220446049250313e-16;
  for (size_t r = 0; r < n_matrices * (size_t)n1d; ++r)
    {
      const double *row = tab + r * (size_t)n1d;
      double *dst = out + r * (size_t)n1d;
      int top = 0;
      for (int j = 1; j < n1d; ++j)
        if (std::fabs(row[j]) > std::fabs(row[top]))
          top = j;
      bool unit = std::fabs(row[top] - 1.0) <= tol;
      for (int j = 0; j < n1d && unit; ++j)
        unit = j == top || std::fabs(row[j]) <= tol;
      for (int j = 0; j < n1d; ++j)
        dst[j] = unit ? (j == top ? 1.0 : 0.0) : row[j];
    }
}

extern "C" int pdh_galerkin_matrices_1d(const pdh_transfer_desc *d, double *out)
{
  PDH_TRY(pdh_transfer_matrices_1d(d, out));
  pdh_galerkin_tables(d->degree + 1, (size_t)d->n_fine * d->dim, out, out);
  return PDH_OK;
}

extern "C" int pdh_galerkin_plan(const pdh_transfer_desc *d, const pdh_galerkin_level *fine, const pdh_galerkin_level *coarse,
                                 int64_t *plan_ptr, int32_t *plan_slot, int32_t *plan_pos)
{
  PDH_TRY(pdh_check_transfer(d));
  if (!plan_ptr || !plan_slot || !plan_pos)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_galerkin_plan: plan_ptr, plan_slot and plan_pos are required");
  const PdhGalerkinPair T{d->dim, d->degree, d->n_fine, d->n_coarse, d->n_fine_rows, d->n_coarse_rows, d->parent, d->fine_dof_offset,
                          d->coarse_dof_offset};
  PdhGalerkinPlan plan;
  PDH_TRY(pdh_plan_galerkin(pdh_noctx_error(), T, fine, coarse, plan));
  std::copy(plan.ptr.begin(), plan.ptr.end(), plan_ptr);
  std::copy(plan.slot.begin(), plan.slot.end(), plan_slot);
  std::copy(plan.pos.begin(), plan.pos.end(), plan_pos);
  return PDH_OK;
}
