// pdh_capi_matfree.cpp — device driver of the C ABI, the matrix-free SIP operator (kernels: pdh_matfree.h): the set-up that leaves the
// finished 1-D tables of every owned polytope in HBM, and y = A x from them.  Which of its products a smoother takes from the tables is
// pdh_set_smoother_operator's (pdh_capi_solve.cpp: pdh_smoother_vmult).
#include "pdh_ctx.h"
#include "pdh_launch.h"

extern "C" int pdh_setup_matrix_free(pdh_ctx *ctx, pdh_matrix_free_info *info)
{
  PDH_TRY(need_problem(ctx, "pdh_setup_matrix_free"));
  pdh_ctx::Problem &pr = ctx->prob;
  if (pr.row_kernel != RowKernel::terms)
    { // what the planner said, or what kept it from looking
      const PdhDev &D = pr.dev;
      const std::string why = pr.ghost         ? "the problem was set in PDH_EXCHANGE_GHOST mode"
                              : D.dim != 3     ? "the problem is not 3-D"
                              : D.n1d > 4      ? "the degree is above 3"
                              : pr.why_terms.empty() ? "the plan of the problem built no term tables"
                                                     : pr.why_terms;
      return fail(ctx, PDH_EUNSUPPORTED, "pdh_setup_matrix_free: the matrix-free operator needs the term tables of 3-D FE_DGQ / FE_AggloDGP of "
                                         "degree 1 .. 3 on agglomerates of Cartesian cells - " + why);
    }
  const PdhTerms &T = pr.terms;
  const int rec = pdht::matfree_rec_doubles(pr.dev.n1d, T.maxsf, T.maxsi, T.maxcell);
  if (!pr.d_mf_tables)
    {
      PDH_HIP(ctx, hipSetDevice(ctx->device));
      const size_t count = (size_t)std::max(pr.n_owned, 1) * rec;
      double *tables = nullptr;
      PDH_TRY(device_buffer(ctx, count, &tables, "matrix-free operator: tables"));
      PDH_HIP(ctx, hipMemsetAsync(tables, 0, count * sizeof(double), ctx->stream)); // (records behind a polytope's own counts, pad entries)
      PDH_HIP(ctx, pdh_launch_mf_tables(&pr.dev, &T, tables, pr.n_owned, ctx->stream));
      PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      pr.d_mf_tables = tables;
      pr.mf_table_bytes = (int64_t)(count * sizeof(double));
    }
  if (info)
    {
      info->table_bytes = pr.mf_table_bytes;
      info->doubles_per_polytope = rec;
      info->max_cells = T.maxcell;
      info->max_subfaces = T.maxsf;
      info->max_interior_subfaces = T.maxsi;
    }
  return PDH_OK;
}

extern "C" int pdh_matrix_free_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y)
{
  PDH_TRY(pdh_vmult_vectors_check(ctx, "pdh_matrix_free_vmult", d_x, d_y));
  if (!ctx->prob.d_mf_tables)
    return fail(ctx, PDH_ESTATE, "pdh_matrix_free_vmult: the matrix-free operator is not set up (pdh_setup_matrix_free)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, pdh_launch_mf_vmult(&A, ctx->prob.dev.n1d, &ctx->prob.terms, ctx->prob.d_mf_tables, d_x, d_y, nullptr, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_matrix_free_vmult(pdh_ctx *ctx, const double *x, double *y)
{
  PDH_TRY(pdh_vmult_vectors_check(ctx, "pdh_matrix_free_vmult", x, y));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_x = nullptr, *d_y = nullptr;
  PDH_TRY(stage_in(ctx, "pdh_matrix_free_vmult", ctx->io.in0, x, (size_t)ctx->prob.n_rows_total, &d_x));
  PDH_TRY(stage(ctx, "pdh_matrix_free_vmult", ctx->io.in1, (size_t)ctx->prob.n_rows_owned, &d_y));
  PDH_TRY(pdh_matrix_free_vmult_device(ctx, d_x, d_y));
  PDH_HIP(ctx, hipMemcpyAsync(y, d_y, ctx->prob.n_rows_owned * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}
