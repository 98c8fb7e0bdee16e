// pdh_transfer_plan.cpp — the host-only planner of a level transfer (pdh_transfer.h): the refusals of pdh_check_transfer, the 1-D
// matrices of every fine polytope and the children CSR that fixes the summation order of the restriction; and of a p-transfer
// (pdh_ptransfer.h): the refusals of pdh_check_ptransfer, the one 1-D matrix of FE_DGQ and the index map of FE_AggloDGP.  Plain C++ like
// pdh_plan.cpp: no HIP header, no HIP call; the 1-D basis and the multi-index lists are those behind the kernels' tables (pdh_basis.h).
#include "pdh_transfer.h"
#include "pdh_ptransfer.h"

#include "pdh_basis.h"
#include "pdh_plan_internal.h"

#include <algorithm>
#include <numeric>

namespace
{
int n_dofs(const pdh_transfer_desc *d)
{
  int n = 1;
  for (int c = 0; c < d->dim; ++c)
    n *= d->degree + 1;
  return n;
}

// dof ranges [off, off + n) of one level: inside [0, n_rows), pairwise disjoint
int check_dof_ranges(std::string &err, const char *level, const int32_t *off, int count, int n, int64_t n_rows)
{
  std::vector<int32_t> order((size_t)count);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return off[a] < off[b]; });
  for (int k = 0; k < count; ++k)
    {
      const int a = order[(size_t)k];
      if (off[a] < 0 || (int64_t)off[a] + n > n_rows)
        return fail(err, PDH_EINVAL, std::string("the dofs of ") + level + " polytope " + std::to_string(a) + " leave [0, n_rows)");
      if (k > 0 && (int64_t)off[order[(size_t)k - 1]] + n > off[a])
        return fail(err, PDH_EINVAL, std::string("the dofs of ") + level + " polytopes " + std::to_string(order[(size_t)k - 1]) + " and " +
                                       std::to_string(a) + " overlap");
    }
  return PDH_OK;
}

int check_boxes(std::string &err, const char *level, const double *bbox, int count, int dim)
{
  for (int a = 0; a < count; ++a)
    for (int c = 0; c < dim; ++c)
      {
        const double lo = bbox[(size_t)a * 2 * dim + c], hi = bbox[(size_t)a * 2 * dim + dim + c];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo))
          return fail(err, PDH_EINVAL, std::string("the box of ") + level + " polytope " + std::to_string(a) + " is degenerate");
      }
  return PDH_OK;
}

// every refusal of pdh_check_transfer, in the order of include/polydeal_hip.h
int validate(std::string &err, const pdh_transfer_desc *d)
{
  if (!d)
    return fail(err, PDH_EINVAL, "the transfer description is NULL");
  if (d->dim != 2 && d->dim != 3)
    return fail(err, PDH_EINVAL, "dim must be 2 or 3");
  if (d->basis == PDH_BASIS_AGGLODGP)
    return fail(err, PDH_EUNSUPPORTED, "FE_AggloDGP has no support points: the injection needs FE_DGQ");
  if (d->basis != PDH_BASIS_DGQ)
    return fail(err, PDH_EINVAL, "unknown basis");
  // (in 2-D this is also the bound of 64 dofs per polytope: (p + 1)^2 <= 64)
  if (d->degree < 1 || d->degree > 7)
    return fail(err, PDH_EUNSUPPORTED, "the degree of a transfer must be in [1,7]");
  if (d->n_fine <= 0 || d->n_coarse <= 0)
    return fail(err, PDH_EINVAL, "n_fine and n_coarse must be positive");
  if (d->n_coarse >= d->n_fine)
    return fail(err, PDH_EINVAL, "the coarse level must have fewer polytopes than the fine one");
  if (!d->fine_bbox || !d->coarse_bbox || !d->fine_dof_offset || !d->coarse_dof_offset || !d->parent)
    return fail(err, PDH_EINVAL, "bbox, dof_offset (both levels) and parent are required");
  const int dim = d->dim, n = n_dofs(d);
  std::vector<int32_t> n_children((size_t)d->n_coarse, 0);
  for (int F = 0; F < d->n_fine; ++F)
    {
      if (d->parent[F] < 0 || d->parent[F] >= d->n_coarse)
        return fail(err, PDH_EINVAL, "the parent of fine polytope " + std::to_string(F) + " is out of range");
      ++n_children[(size_t)d->parent[F]];
    }
  for (int C = 0; C < d->n_coarse; ++C)
    if (!n_children[(size_t)C])
      return fail(err, PDH_EINVAL, "coarse polytope " + std::to_string(C) + " has no children");
  PDH_TRY(check_boxes(err, "fine", d->fine_bbox, d->n_fine, dim));
  PDH_TRY(check_boxes(err, "coarse", d->coarse_bbox, d->n_coarse, dim));
  for (int F = 0; F < d->n_fine; ++F)
    for (int c = 0; c < dim; ++c)
      {
        const double *bf = d->fine_bbox + (size_t)F * 2 * dim, *bc = d->coarse_bbox + (size_t)d->parent[F] * 2 * dim;
        const double slack = 1e-12 * (bc[dim + c] - bc[c]);
        if (bf[c] < bc[c] - slack || bf[dim + c] > bc[dim + c] + slack)
          return fail(err, PDH_EINVAL, "the box of fine polytope " + std::to_string(F) + " is not inside the box of its parent " +
                                         std::to_string(d->parent[F]));
      }
  PDH_TRY(check_dof_ranges(err, "fine", d->fine_dof_offset, d->n_fine, n, d->n_fine_rows));
  return check_dof_ranges(err, "coarse", d->coarse_dof_offset, d->n_coarse, n, d->n_coarse_rows);
}

// B_c[i][j] = l_j(xi_i), xi_i the i-th support point of the fine box in the unit coordinates of the parent's box; Horner in the centred
// variable like the kernels (pdh_basis.h), in long double
void matrices_1d(const pdh_transfer_desc *d, double *out)
{
  const int dim = d->dim, p = d->degree, n1d = p + 1;
  const pdh::Basis1D basis = pdh::lagrange_basis(p);
  const std::vector<long double> nodes = pdh::gauss_lobatto_nodes(p);
  for (int F = 0; F < d->n_fine; ++F)
    for (int c = 0; c < dim; ++c)
      {
        const double *bf = d->fine_bbox + (size_t)F * 2 * dim, *bc = d->coarse_bbox + (size_t)d->parent[F] * 2 * dim;
        const long double lo_f = bf[c], h_f = (long double)bf[dim + c] - bf[c], lo_c = bc[c], h_c = (long double)bc[dim + c] - bc[c];
        double *B = out + ((size_t)F * dim + c) * n1d * n1d;
        for (int i = 0; i < n1d; ++i)
          {
            const long double t = (lo_f + nodes[(size_t)i] * h_f - lo_c) / h_c - 0.5L;
            for (int j = 0; j < n1d; ++j)
              {
                long double v = basis.coef[(size_t)j][(size_t)p];
                for (int m = p - 1; m >= 0; --m)
                  v = v * t + basis.coef[(size_t)j][(size_t)m];
                B[i * n1d + j] = (double)v;
              }
          }
      }
}

void children_csr(const pdh_transfer_desc *d, std::vector<int32_t> &ptr, std::vector<int32_t> &idx)
{
  ptr.assign((size_t)d->n_coarse + 1, 0);
  for (int F = 0; F < d->n_fine; ++F)
    ++ptr[(size_t)d->parent[F] + 1];
  for (int C = 0; C < d->n_coarse; ++C)
    ptr[(size_t)C + 1] += ptr[(size_t)C];
  idx.resize((size_t)d->n_fine);
  std::vector<int32_t> at(ptr.begin(), ptr.end() - 1);
  for (int F = 0; F < d->n_fine; ++F) // ascending F: ascending inside every parent
    idx[(size_t)at[(size_t)d->parent[F]]++] = F;
}

// ---- p-transfers ----
int p_basis(const pdh_ptransfer_desc *d) { return d->basis == PDH_BASIS_DGQ ? 0 : 1; }

// every refusal of pdh_check_ptransfer, in the order of include/polydeal_hip.h
int validate_p(std::string &err, const pdh_ptransfer_desc *d)
{
  if (!d)
    return fail(err, PDH_EINVAL, "the p-transfer description is NULL");
  if (d->dim != 2 && d->dim != 3)
    return fail(err, PDH_EINVAL, "dim must be 2 or 3");
  if (d->basis != PDH_BASIS_DGQ && d->basis != PDH_BASIS_AGGLODGP)
    return fail(err, PDH_EINVAL, "unknown basis");
  // (in 2-D this is also the bound of 64 fine dofs per polytope: (p + 1)^2 <= 64)
  if (d->coarse_degree < 1 || d->fine_degree > 7 || d->coarse_degree >= d->fine_degree)
    return fail(err, PDH_EUNSUPPORTED, "the degrees of a p-transfer must be 1 <= coarse_degree < fine_degree <= 7");
  if (d->n_polytopes <= 0)
    return fail(err, PDH_EINVAL, "n_polytopes must be positive");
  if (!d->fine_dof_offset || !d->coarse_dof_offset)
    return fail(err, PDH_EINVAL, "dof_offset (both levels) is required");
  PDH_TRY(check_dof_ranges(err, "fine", d->fine_dof_offset, d->n_polytopes, pdh::n_dofs_per_cell(d->dim, d->fine_degree, p_basis(d)), d->n_fine_rows));
  return check_dof_ranges(err, "coarse", d->coarse_dof_offset, d->n_polytopes, pdh::n_dofs_per_cell(d->dim, d->coarse_degree, p_basis(d)),
                          d->n_coarse_rows);
}

// B[i][j] = l^q_j(node^p_i): Horner in the centred variable, in long double, rounded once - exactly as matrices_1d does
void p_matrix_1d(int p, int q, double *out)
{
  const pdh::Basis1D basis = pdh::lagrange_basis(q);
  const std::vector<long double> nodes = pdh::gauss_lobatto_nodes(p);
  for (int i = 0; i <= p; ++i)
    {
      const long double t = nodes[(size_t)i] - 0.5L;
      for (int j = 0; j <= q; ++j)
        {
          long double v = basis.coef[(size_t)j][(size_t)q];
          for (int m = q - 1; m >= 0; --m)
            v = v * t + basis.coef[(size_t)j][(size_t)m];
          out[i * (q + 1) + j] = (double)v;
        }
    }
}

// map[j] = the fine dof with the multi-index of coarse dof j (FE_AggloDGP: every coarse multi-index is a fine one)
std::vector<int32_t> p_index_map(int dim, int p, int q)
{
  const std::vector<uint32_t> fine = pdh::multi_indices(dim, p, 1), coarse = pdh::multi_indices(dim, q, 1);
  std::vector<int32_t> map(coarse.size(), -1);
  for (size_t j = 0; j < coarse.size(); ++j)
    map[j] = (int32_t)(std::find(fine.begin(), fine.end(), coarse[j]) - fine.begin());
  return map;
}
} // namespace

int pdh_plan_ptransfer(std::string &err, const pdh_ptransfer_desc *d, PdhPTransferPlan &plan)
{
  PDH_TRY(validate_p(err, d));
  plan.n_f = pdh::n_dofs_per_cell(d->dim, d->fine_degree, p_basis(d));
  plan.n_c = pdh::n_dofs_per_cell(d->dim, d->coarse_degree, p_basis(d));
  if (d->basis == PDH_BASIS_DGQ)
    {
      plan.B.resize((size_t)(d->fine_degree + 1) * (d->coarse_degree + 1));
      p_matrix_1d(d->fine_degree, d->coarse_degree, plan.B.data());
      return PDH_OK;
    }
  plan.map = p_index_map(d->dim, d->fine_degree, d->coarse_degree);
  plan.inv.assign((size_t)plan.n_f, -1);
  for (size_t j = 0; j < plan.map.size(); ++j)
    plan.inv[(size_t)plan.map[j]] = (int32_t)j;
  return PDH_OK;
}

extern "C" int pdh_check_ptransfer(const pdh_ptransfer_desc *d) { return validate_p(pdh_noctx_error(), d); }

extern "C" int pdh_ptransfer_matrix_1d(const pdh_ptransfer_desc *d, double *out)
{
  PDH_TRY(validate_p(pdh_noctx_error(), d));
  if (d->basis != PDH_BASIS_DGQ)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_ptransfer_matrix_1d: FE_AggloDGP has an index map (pdh_ptransfer_index_map), no 1-D matrix");
  if (!out)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_ptransfer_matrix_1d: out is required");
  p_matrix_1d(d->fine_degree, d->coarse_degree, out);
  return PDH_OK;
}

extern "C" int pdh_ptransfer_index_map(const pdh_ptransfer_desc *d, int32_t *out)
{
  PDH_TRY(validate_p(pdh_noctx_error(), d));
  if (d->basis != PDH_BASIS_AGGLODGP)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_ptransfer_index_map: FE_DGQ has a 1-D matrix (pdh_ptransfer_matrix_1d), no index map");
  if (!out)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_ptransfer_index_map: out is required");
  const std::vector<int32_t> map = p_index_map(d->dim, d->fine_degree, d->coarse_degree);
  std::copy(map.begin(), map.end(), out);
  return PDH_OK;
}

int pdh_plan_transfer(std::string &err, const pdh_transfer_desc *d, PdhTransferPlan &plan)
{
  PDH_TRY(validate(err, d));
  const int n1d = d->degree + 1;
  plan.tab.resize((size_t)d->n_fine * d->dim * n1d * n1d);
  matrices_1d(d, plan.tab.data());
  children_csr(d, plan.child_ptr, plan.child_idx);
  return PDH_OK;
}

extern "C" int pdh_check_transfer(const pdh_transfer_desc *d) { return validate(pdh_noctx_error(), d); }

extern "C" int pdh_transfer_matrices_1d(const pdh_transfer_desc *d, double *out)
{
  PDH_TRY(validate(pdh_noctx_error(), d));
  if (!out)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_transfer_matrices_1d: out is required");
  matrices_1d(d, out);
  return PDH_OK;
}

extern "C" int pdh_transfer_children(const pdh_transfer_desc *d, int32_t *child_ptr, int32_t *child_idx)
{
  PDH_TRY(validate(pdh_noctx_error(), d));
  if (!child_ptr || !child_idx)
    return fail(pdh_noctx_error(), PDH_EINVAL, "pdh_transfer_children: child_ptr and child_idx are required");
  std::vector<int32_t> ptr, idx;
  children_csr(d, ptr, idx);
  std::copy(ptr.begin(), ptr.end(), child_ptr);
  std::copy(idx.begin(), idx.end(), child_idx);
  return PDH_OK;
}
