// pdh_capi_solve.cpp — device driver of the C ABI, solving with the resident matrix (kernels: pdh_solve.hip): y = A x, the Jacobi /
// block Jacobi inverses, CG, and the Chebyshev smoother / preconditioner.  The one CG recurrence (CgRun) serves the solver and the
// eigenvalue estimate of the Chebyshev set-up; the host arithmetic of the latter is the planner's (pdh_plan.h).  The dense direct solve
// (kernels: pdh_dense.hip) is one more preconditioner; the V-cycle (pdh_capi_mg.cpp) composes the helpers of this unit.  The smoother may
// read a float32 copy of the matrix and of the block inverses instead (pdh_set_smoother_precision; kernels: pdh_shadow.hip).
#include "pdh_ctx.h"
#include "pdh_cg_run.h"
#include "pdh_dense.h"
#include "pdh_launch.h"
#include "pdh_shadow.h"

#include <cmath>

PdhSolveArgs pdh_solve_args(const pdh_ctx *ctx)
{
  PdhSolveArgs A;
  A.values = ctx->prob.dev.values;
  A.row_base = ctx->prob.dev.row_base;
  A.row_len = ctx->prob.dev.row_len;
  A.diag_L = ctx->prob.dev.diag_L;
  A.own_row = ctx->prob.dev.own_row;
  A.blk_ptr = ctx->prob.d_blk_ptr;
  A.blk_dof = ctx->prob.d_blk_dof;
  A.n = ctx->prob.dev.n;
  A.diag_first = ctx->prob.dev.diag_first;
  A.n_owned = ctx->prob.n_owned;
  A.max_row_len = ctx->prob.max_row_len;
  return A;
}

static bool overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
  const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
  return pa < pb + nb * (int64_t)sizeof(double) && pb < pa + na * (int64_t)sizeof(double);
}

static constexpr int PDH_VMULT_LDS_CAP = 64 * 1024; // column set of one polytope in LDS (8192 columns)

int pdh_row_fits_lds(pdh_ctx *ctx)
{
  if ((int64_t)ctx->prob.max_row_len * (int64_t)sizeof(double) > PDH_VMULT_LDS_CAP)
    return fail(ctx, PDH_EUNSUPPORTED, "a row has more than 8192 entries (the column set of a polytope must fit 64 KB of LDS)");
  return PDH_OK;
}

// The solvers run on a context that owns all rows without the exchange variant.  The two families of messages differ in their
// wording only: `runs_on` / `it` / `tail` are "the solver runs on" / "the solver" / " (no distributed Krylov solver)" for CG and
// "it needs" / "it" / "" for the Chebyshev set-up.
static int all_rows_checks(pdh_ctx *ctx, const char *who, const char *runs_on, const char *it, const char *tail)
{
  if (ctx->prob.ghost)
    return fail(ctx, PDH_EUNSUPPORTED, std::string(who) + ": the problem was set in PDH_EXCHANGE_GHOST mode; " + runs_on +
                                         " a context that owns all rows with PDH_EXCHANGE_NONE" + tail);
  if (ctx->prob.n_rows_owned != ctx->prob.n_rows_total)
    return fail(ctx, PDH_EUNSUPPORTED, std::string(who) + ": the context owns rows " + std::to_string(ctx->prob.n_rows_owned) + " of " +
                                         std::to_string(ctx->prob.n_rows_total) + "; " + it + " needs all rows in one context" + tail);
  return PDH_OK;
}

int pdh_vmult_vectors_check(pdh_ctx *ctx, const char *name, const void *x, const void *y)
{
  PDH_TRY(need_problem(ctx, name));
  if (!x || !y)
    return fail(ctx, PDH_EINVAL, "x and y are required");
  if (overlap(x, ctx->prob.n_rows_total, y, ctx->prob.n_rows_owned))
    return fail(ctx, PDH_EINVAL, "x and y overlap");
  return PDH_OK;
}

static int vmult_checks(pdh_ctx *ctx, const void *x, const void *y)
{
  PDH_TRY(pdh_vmult_vectors_check(ctx, "pdh_vmult", x, y));
  return pdh_row_fits_lds(ctx);
}

extern "C" int pdh_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y)
{
  PDH_TRY(vmult_checks(ctx, d_x, d_y));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, pdh_launch_vmult(&A, d_x, d_y, nullptr, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_vmult(pdh_ctx *ctx, const double *x, double *y)
{
  PDH_TRY(vmult_checks(ctx, x, y));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_x = nullptr, *d_y = nullptr;
  PDH_TRY(stage_in(ctx, "pdh_vmult", ctx->io.in0, x, (size_t)ctx->prob.n_rows_total, &d_x));
  PDH_TRY(stage(ctx, "pdh_vmult", ctx->io.in1, (size_t)ctx->prob.n_rows_owned, &d_y));
  PDH_TRY(pdh_vmult_device(ctx, d_x, d_y));
  PDH_HIP(ctx, hipMemcpyAsync(y, d_y, ctx->prob.n_rows_owned * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// r = b - A x: k_vmult into r, then one subtraction over the owned rows
extern "C" int pdh_residual_device(pdh_ctx *ctx, const double *d_b, const double *d_x, double *d_r)
{
  PDH_TRY(need_problem(ctx, "pdh_residual_device"));
  if (!d_b || !d_x || !d_r)
    return fail(ctx, PDH_EINVAL, "b, x and r are required");
  if (overlap(d_x, ctx->prob.n_rows_total, d_r, ctx->prob.n_rows_owned) || overlap(d_b, ctx->prob.n_rows_owned, d_r, ctx->prob.n_rows_owned))
    return fail(ctx, PDH_EINVAL, "r overlaps x or b");
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, pdh_launch_vmult(&A, d_x, d_r, nullptr, ctx->stream));
  PDH_HIP(ctx, pdh_launch_residual_sub(ctx->prob.n_rows_owned, d_b, d_r, ctx->stream));
  return PDH_OK;
}

// every set-up call replaces the preconditioner: an attached V-cycle is let go of, and a pdh_mg that has this context as a level sees
// the new epoch
static void new_setup(pdh_ctx *ctx)
{
  pdh_mg_detach(ctx);
  ctx->mg_gone = false;
  ++ctx->prec_epoch;
  ctx->prob.sol.f32 = false; // the smoother precision and operator belong to one set-up (pdh_set_smoother_precision / _operator)
  ctx->prob.sol.matrix_free = false;
}

extern "C" int pdh_setup_preconditioner(pdh_ctx *ctx, int kind)
{
  PDH_TRY(need_problem(ctx, "pdh_setup_preconditioner"));
  if (kind != PDH_PREC_NONE && kind != PDH_PREC_JACOBI && kind != PDH_PREC_BLOCK_JACOBI)
    return fail(ctx, PDH_EINVAL, "kind must be PDH_PREC_NONE, PDH_PREC_JACOBI or PDH_PREC_BLOCK_JACOBI");
  if (kind == PDH_PREC_BLOCK_JACOBI && ctx->prob.dev.n > 64)
    return fail(ctx, PDH_EUNSUPPORTED, "block Jacobi needs at most 64 dofs per polytope (use PDH_PREC_JACOBI)");
  new_setup(ctx);
  ctx->prec_kind = kind;
  ctx->prec_gen = ctx->values_gen;
  ctx->prec_ok = false; // until the set-up below has succeeded
  if (kind == PDH_PREC_NONE)
    {
      ctx->prec_ok = true;
      return PDH_OK;
    }
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = ctx->prob.dev.n;
  pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  double *dinv = S.dinv.get<double>(kind == PDH_PREC_BLOCK_JACOBI ? ctx->prob.n_owned * n * n : ctx->prob.n_rows_owned);
  int32_t *flag = S.flag.get<int32_t>(ctx->prob.n_owned);
  if (!dinv || !flag)
    return fail(ctx, PDH_EDEVICE, "pdh_setup_preconditioner: out of device memory");
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, kind == PDH_PREC_BLOCK_JACOBI ? pdh_launch_block_inverse(&A, dinv, flag, ctx->stream)
                                             : pdh_launch_diag_inverse(&A, dinv, flag, ctx->stream));
  std::vector<int32_t> h_flag((size_t)ctx->prob.n_owned);
  if (ctx->prob.n_owned)
    PDH_HIP(ctx, hipMemcpyAsync(h_flag.data(), flag, h_flag.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < ctx->prob.n_owned; ++s)
    if (h_flag[s])
      { // slots are in polytope order: the first flagged slot is the lowest polytope number
        int32_t agg = -1;
        PDH_HIP(ctx, hipMemcpy(&agg, ctx->prob.dev.own_agg + s, sizeof(int32_t), hipMemcpyDeviceToHost));
        return fail(ctx, PDH_EINVAL,
                    kind == PDH_PREC_BLOCK_JACOBI
                      ? "block Jacobi: the diagonal block of polytope " + std::to_string(agg) + " is not positive definite"
                      : "Jacobi: a diagonal entry of polytope " + std::to_string(agg) + " is zero or not finite");
      }
  ctx->prec_ok = true;
  return PDH_OK;
}

int pdh_prec_checks(pdh_ctx *ctx)
{
  if (ctx->mg_gone)
    return fail(ctx, PDH_ESTATE, "the multigrid preconditioner of this context was destroyed: the context fell back to PDH_PREC_NONE, set a "
                                 "preconditioner up again (pdh_setup_preconditioner takes PDH_PREC_NONE)");
  if (ctx->prec_kind == PDH_PREC_MULTIGRID)
    return ctx->mg ? pdh_mg_checks(ctx->mg) : fail(ctx, PDH_ESTATE, "the multigrid preconditioner is not attached");
  if (ctx->prec_kind != PDH_PREC_NONE && (!ctx->prec_ok || ctx->prec_gen != ctx->values_gen))
    return fail(ctx, PDH_ESTATE, ctx->prec_ok ? "the values changed since pdh_setup_preconditioner: set it up again"
                                              : "the last pdh_setup_preconditioner failed");
  return PDH_OK;
}

// One application of the Chebyshev polynomial to b, queued on the stream: x <- x + p(P^-1 A) P^-1 (b - A x) (zero: x <- p(..) P^-1 b,
// x not read).  d, r and q are the context's own vectors - never CG's residual.  rcg / part: see pdh_launch_cheb_update.
int pdh_cheb_apply(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *b, double *x, bool zero, const double *rcg, double *part,
                   hipStream_t stream)
{
  const pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  double *d = S.cheb_d.ptr<double>(), *r = S.cheb_r.ptr<double>(), *q = S.q.ptr<double>();
  const double *dinv = S.dinv.ptr<double>();
  const int m = (int)S.cheb_c2.size();
  if (!d || !r || !q || !dinv || m < 1)
    return fail(report, PDH_ESTATE, "the Chebyshev preconditioner is not set up");
  // PDH_SMOOTHER_F32: the products read the shadow rows, the block branch of the update the float inverses (point Jacobi stays double)
  const float *dinv32 = S.f32 && S.cheb_inner == PDH_PREC_BLOCK_JACOBI ? S.sh_dinv.ptr<float>() : nullptr;
  if (!zero)
    PDH_TRY(pdh_smoother_vmult(ctx, report, A, x, q, stream));
  for (int k = 0; k < m; ++k)
    {
      if (k > 0)
        PDH_TRY(pdh_smoother_vmult(ctx, report, A, d, q, stream));
      const double *qk = (k == 0 && zero) ? nullptr : q, *rcgk = k == m - 1 ? rcg : nullptr;
      if (dinv32)
        PDH_HIP(report, pdh_launch_cheb_update_f32(&A, k == 0, dinv32, b, qk, d, r, x, S.cheb_c1[k], S.cheb_c2[k], k == 0 && zero, rcgk, part, stream));
      else
        PDH_HIP(report, pdh_launch_cheb_update(&A, k == 0, S.cheb_inner, dinv, b, qk, d, r, x, S.cheb_c1[k], S.cheb_c2[k], k == 0 && zero, rcgk,
                                               part, stream));
    }
  return PDH_OK;
}

static int cheb_apply(pdh_ctx *ctx, const PdhSolveArgs &A, const double *b, double *x, bool zero, const double *rcg, double *part)
{
  return pdh_cheb_apply(ctx, ctx, A, b, x, zero, rcg, part, ctx->stream);
}

// z = G r of PDH_PREC_DIRECT (r and z disjoint)
static int direct_apply(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *r, double *z, const double *rcg, double *part,
                        hipStream_t stream)
{
  const pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  if (!S.dense_g.ptr<double>() || S.dense_n != ctx->prob.n_rows_owned)
    return fail(report, PDH_ESTATE, "the direct solve is not set up");
  PDH_HIP(report, pdh_launch_dense_symv(&A, S.dense_g.ptr<double>(), S.dense_ld, S.dense_n, r, z, rcg, part, stream));
  return PDH_OK;
}

int pdh_prec_apply(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *r, double *z, const double *rcg, double *part,
                   hipStream_t stream)
{
  if (ctx->prec_kind == PDH_PREC_CHEBYSHEV)
    return pdh_cheb_apply(ctx, report, A, r, z, true, rcg, part, stream);
  if (ctx->prec_kind == PDH_PREC_DIRECT)
    return direct_apply(ctx, report, A, r, z, rcg, part, stream);
  if (rcg)
    return fail(report, PDH_EINVAL, "pdh_prec_apply: no partials from this kind");
  PDH_HIP(report, pdh_launch_cg_update(&A, PDH_UPD_APPLY, ctx->prec_kind, ctx->prob.sol.dinv.ptr<double>(), nullptr, nullptr, nullptr, nullptr,
                                       const_cast<double *>(r), z, nullptr, nullptr, stream));
  return PDH_OK;
}

extern "C" int pdh_precondition_device(pdh_ctx *ctx, const double *d_r, double *d_z)
{
  PDH_TRY(need_problem(ctx, "pdh_precondition_device"));
  if (!d_r || !d_z)
    return fail(ctx, PDH_EINVAL, "r and z are required");
  // in place is served (a slot's r is read before its z is written); a shifted z would overwrite r of slots not read yet
  if (d_r != d_z && overlap(d_r, ctx->prob.n_rows_owned, d_z, ctx->prob.n_rows_owned))
    return fail(ctx, PDH_EINVAL, "r and z overlap partially (they must be the same array or disjoint)");
  PDH_TRY(pdh_prec_checks(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = pdh_solve_args(ctx);
  if (ctx->prec_kind == PDH_PREC_DIRECT || ctx->prec_kind == PDH_PREC_MULTIGRID)
    { // every wave reads all of r (the cycle: r again after z was written): the in-place call works on a copy of r
      const int64_t N = ctx->prob.n_rows_owned;
      if (d_r == d_z)
        {
          double *tmp = ctx->prob.sol.dense_tmp.get<double>((size_t)N);
          if (!tmp)
            return fail(ctx, PDH_EDEVICE, "pdh_precondition_device: out of device memory");
          PDH_HIP(ctx, hipMemcpyAsync(tmp, d_r, N * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
          d_r = tmp;
        }
      if (ctx->prec_kind == PDH_PREC_MULTIGRID)
        return pdh_mg_cycle(ctx->mg, d_r, d_z, true, nullptr, nullptr);
      return direct_apply(ctx, ctx, A, d_r, d_z, nullptr, nullptr, ctx->stream);
    }
  return pdh_prec_apply(ctx, ctx, A, d_r, d_z, nullptr, nullptr, ctx->stream);
}

extern "C" int pdh_solve_cg_device(pdh_ctx *ctx, const pdh_cg_control *c, const double *d_b, double *d_x, pdh_cg_result *res)
{
  PDH_TRY(need_problem(ctx, "pdh_solve_cg"));
  if (!c || !d_b || !d_x || !res)
    return fail(ctx, PDH_EINVAL, "control, b, x and result are required");
  if (c->max_iter < 0 || !(c->rel_tol >= 0.0) || !(c->abs_tol >= 0.0))
    return fail(ctx, PDH_EINVAL, "max_iter, rel_tol and abs_tol must be non-negative");
  PDH_TRY(all_rows_checks(ctx, "pdh_solve_cg", "the solver runs on", "the solver", " (no distributed Krylov solver)"));
  if (overlap(d_b, ctx->prob.n_rows_total, d_x, ctx->prob.n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  PDH_TRY(pdh_prec_checks(ctx));
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const bool chained = ctx->prec_kind == PDH_PREC_CHEBYSHEV || ctx->prec_kind == PDH_PREC_DIRECT || ctx->prec_kind == PDH_PREC_MULTIGRID;
  CgRun cg(ctx, chained ? PDH_PREC_NONE : ctx->prec_kind, chained ? ctx->prec_kind : PDH_PREC_NONE);
  if (!cg.ok())
    return fail(ctx, PDH_EDEVICE, "pdh_solve_cg: out of device memory");
  PDH_TRY(cg.start(d_b, d_x, PDH_CG_RR, 2));
  double rr = ctx->pinned[0];
  const double bnorm = std::sqrt(ctx->pinned[1]);
  const double stop = std::max(c->abs_tol, c->rel_tol * bnorm);
  res->residual0 = std::sqrt(rr);
  int it = 0;
  // test, then one step.  Only ||r||^2 crosses PCIe (8 bytes, pinned).
  for (; it < c->max_iter && std::sqrt(rr) > stop; ++it)
    {
      PDH_TRY(cg.step(d_x, PDH_CG_RR, 1));
      rr = ctx->pinned[0];
    }
  res->iterations = it;
  res->residual = std::sqrt(rr);
  if (!(res->residual <= stop))
    return fail(ctx, PDH_ENOCONV, "pdh_solve_cg: no convergence in " + std::to_string(it) + " iterations (||r|| = " +
                                    std::to_string(res->residual) + ", bound " + std::to_string(stop) + ")");
  return PDH_OK;
}

extern "C" int pdh_solve_cg(pdh_ctx *ctx, const pdh_cg_control *c, const double *b, double *x, pdh_cg_result *res)
{
  PDH_TRY(need_problem(ctx, "pdh_solve_cg"));
  if (!b || !x)
    return fail(ctx, PDH_EINVAL, "b and x are required");
  if (overlap(b, ctx->prob.n_rows_total, x, ctx->prob.n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = ctx->prob.n_rows_total;
  double *d_b = nullptr, *d_x = nullptr;
  PDH_TRY(stage_in(ctx, "pdh_solve_cg", ctx->io.in0, b, (size_t)N, &d_b));
  PDH_TRY(stage_in(ctx, "pdh_solve_cg", ctx->io.in1, x, (size_t)N, &d_x));
  const int rc = pdh_solve_cg_device(ctx, c, d_b, d_x, res);
  if (rc != PDH_OK && rc != PDH_ENOCONV)
    return rc;
  const std::string msg = ctx->err;
  PDH_HIP(ctx, hipMemcpyAsync(x, d_x, N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (rc == PDH_ENOCONV)
    ctx->err = msg;
  return rc;
}

// ---- Chebyshev smoother / preconditioner (include/polydeal_hip.h: pdh_setup_chebyshev) ----------------------------------------------
// Largest Ritz value of P^-1 A after k steps of P-preconditioned CG on A x = b0 from x = 0 (P = the inner preconditioner, set up and
// current): the solver's recurrence, but alpha_j, beta_j and ||r||^2 come back every step.  steps: CG steps that entered the
// Lanczos matrix.
static int cheb_estimate(pdh_ctx *ctx, int kind, int k, double *est, int *steps)
{
  const int64_t N = ctx->prob.n_rows_owned;
  CgRun cg(ctx, kind, PDH_PREC_NONE);
  double *d_b = ctx->io.in0.get<double>((size_t)N), *d_x = ctx->io.in1.get<double>((size_t)N);
  if (!cg.ok() || !d_b || !d_x)
    return fail(ctx, PDH_EDEVICE, "pdh_setup_chebyshev: out of device memory");
  std::vector<double> b0((size_t)N);
  for (int64_t i = 0; i < N; ++i)
    b0[(size_t)i] = (double)(uint32_t)(2654435761ull * (uint64_t)i) / 4294967296.0 - 0.5;
  PDH_HIP(ctx, hipMemcpyAsync(d_b, b0.data(), N * sizeof(double), hipMemcpyHostToDevice, cg.st));
  PDH_HIP(ctx, hipMemsetAsync(d_x, 0, N * sizeof(double), cg.st));
  PDH_TRY(cg.start(d_b, d_x, 0, PDH_CG_NSCALARS));
  double rr = ctx->pinned[PDH_CG_RR];
  std::vector<double> alpha, beta;
  for (int it = 0; it < k && rr > 0.0; ++it)
    {
      PDH_TRY(cg.step(d_x, 0, PDH_CG_NSCALARS));
      const double a = ctx->pinned[PDH_CG_ALPHA], b = ctx->pinned[PDH_CG_BETA];
      if (!(a > 0.0) || !std::isfinite(a) || !(b >= 0.0) || !std::isfinite(b))
        break; // p^T A p <= 0 or a breakdown: the steps so far
      alpha.push_back(a);
      beta.push_back(b);
      rr = ctx->pinned[PDH_CG_RR];
    }
  const int m = (int)alpha.size();
  if (m < 1)
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: the eigenvalue estimate took no CG step (no rows, or the matrix is not positive "
                                 "definite on the test vector)");
  std::vector<double> dg, od;
  pdh_lanczos_tridiagonal(alpha, beta, dg, od);
  double lo = 0.0, hi = 0.0;
  if (pdh_tridiagonal_eigenvalues(m, dg.data(), od.data(), &lo, &hi) != PDH_OK)
    return fail(ctx, PDH_EINVAL, std::string("pdh_setup_chebyshev: ") + pdh_last_error(nullptr));
  *est = hi;
  *steps = m;
  return PDH_OK;
}

extern "C" int pdh_setup_chebyshev(pdh_ctx *ctx, const pdh_chebyshev_control *c, pdh_chebyshev_info *info)
{
  PDH_TRY(need_problem(ctx, "pdh_setup_chebyshev"));
  if (!c)
    return fail(ctx, PDH_EINVAL, "control is required");
  if (c->inner != PDH_PREC_JACOBI && c->inner != PDH_PREC_BLOCK_JACOBI)
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: inner must be PDH_PREC_JACOBI or PDH_PREC_BLOCK_JACOBI");
  if (c->degree < 1)
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: degree must be at least 1");
  if (!(c->smoothing_range > 1.0) || !std::isfinite(c->smoothing_range))
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: smoothing_range must be finite and greater than 1");
  if (std::isnan(c->max_eigenvalue) || std::isinf(c->max_eigenvalue))
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: max_eigenvalue is not finite");
  const bool given = c->max_eigenvalue > 0.0;
  if (!given && (c->eig_cg_n_iterations < 1 || c->eig_cg_n_iterations > 256))
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: eig_cg_n_iterations must be 1 .. 256 (or give max_eigenvalue > 0)");
  PDH_TRY(all_rows_checks(ctx, "pdh_setup_chebyshev", "it needs", "it", ""));
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_TRY(pdh_setup_preconditioner(ctx, c->inner)); // the inner inverse; prec_kind = inner for the estimate
  ctx->prec_ok = false;                             // until the whole set-up has succeeded
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double est = c->max_eigenvalue;
  int steps = 0;
  if (!given)
    PDH_TRY(cheb_estimate(ctx, c->inner, c->eig_cg_n_iterations, &est, &steps));
  if (!(est > 0.0) || !std::isfinite(est))
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: the eigenvalue estimate " + std::to_string(est) + " is not positive");
  const int64_t N = ctx->prob.n_rows_owned;
  pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  if (!S.cheb_d.get<double>(N) || !S.cheb_r.get<double>(N) || !S.q.get<double>(N))
    return fail(ctx, PDH_EDEVICE, "pdh_setup_chebyshev: out of device memory");
  double lo = 0.0, hi = 0.0;
  pdh_chebyshev_coefficients(c->degree, est, c->smoothing_range, &lo, &hi, S.cheb_c1, S.cheb_c2);
  S.cheb_inner = c->inner;
  ctx->prec_kind = PDH_PREC_CHEBYSHEV;
  ctx->prec_gen = ctx->values_gen;
  ctx->prec_ok = true;
  if (info)
    {
      info->estimate = est;
      info->lambda_lo = lo;
      info->lambda_hi = hi;
      info->cg_iterations = steps;
      info->degree = c->degree;
      info->inner = c->inner;
    }
  return PDH_OK;
}

extern "C" int pdh_chebyshev_step_device(pdh_ctx *ctx, const double *d_b, double *d_x, int zero_initial_guess)
{
  PDH_TRY(need_problem(ctx, "pdh_chebyshev_step_device"));
  if (!d_b || !d_x)
    return fail(ctx, PDH_EINVAL, "b and x are required");
  if (overlap(d_b, ctx->prob.n_rows_total, d_x, ctx->prob.n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  if (ctx->prec_kind != PDH_PREC_CHEBYSHEV)
    return fail(ctx, PDH_ESTATE, "pdh_chebyshev_step_device: the preconditioner set up last is not PDH_PREC_CHEBYSHEV");
  PDH_TRY(pdh_prec_checks(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  return cheb_apply(ctx, pdh_solve_args(ctx), d_b, d_x, zero_initial_guess != 0, nullptr, nullptr);
}

// ---- single-precision smoother matrices (include/polydeal_hip.h: pdh_set_smoother_precision; kernels and layout: pdh_shadow.h) ---------
int pdh_smoother_vmult(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *x, double *y, hipStream_t stream)
{
  const pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  if (S.matrix_free)
    { // PDH_SMOOTHER_OP_MATRIX_FREE: neither the values nor the shadow rows are read
      if (!ctx->prob.d_mf_tables)
        return fail(report, PDH_ESTATE, "the matrix-free operator is not set up");
      PDH_HIP(report, pdh_launch_mf_vmult(&A, ctx->prob.dev.n1d, &ctx->prob.terms, ctx->prob.d_mf_tables, x, y, nullptr, stream));
      return PDH_OK;
    }
  if (!S.f32)
    {
      PDH_HIP(report, pdh_launch_vmult(&A, x, y, nullptr, stream));
      return PDH_OK;
    }
  const PdhShadowArgs Sh{S.sh_values.ptr<float>(), S.sh_base.ptr<int64_t>()};
  if (!Sh.values || !Sh.base)
    return fail(report, PDH_ESTATE, "the single-precision smoother matrix is not set up");
  PDH_HIP(report, pdh_launch_vmult_f32(&A, &Sh, x, y, stream));
  return PDH_OK;
}

// the per-slot bases of the shadow rows, once per resident problem: they follow the row lengths, which a problem keeps
static int shadow_bases(pdh_ctx *ctx)
{
  pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  if (S.sh_count > 0)
    return PDH_OK;
  const size_t n_owned = (size_t)ctx->prob.n_owned;
  int64_t *d_base = S.sh_base.get<int64_t>(n_owned);
  if (!d_base)
    return fail(ctx, PDH_EDEVICE, "pdh_set_smoother_precision: out of device memory");
  std::vector<int32_t> row_len(n_owned);
  std::vector<int64_t> base(n_owned);
  if (n_owned)
    PDH_HIP(ctx, hipMemcpy(row_len.data(), ctx->prob.dev.row_len, n_owned * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t count = 0;
  for (size_t s = 0; s < n_owned; ++s)
    {
      base[s] = count;
      count += (int64_t)ctx->prob.dev.n * pdh_shadow_stride(row_len[s]);
    }
  if (n_owned)
    PDH_HIP(ctx, hipMemcpy(d_base, base.data(), n_owned * sizeof(int64_t), hipMemcpyHostToDevice));
  S.sh_count = std::max<int64_t>(count, 1);
  return PDH_OK;
}

extern "C" int pdh_set_smoother_precision(pdh_ctx *ctx, int precision)
{
  PDH_TRY(need_problem(ctx, "pdh_set_smoother_precision"));
  if (precision != PDH_SMOOTHER_F64 && precision != PDH_SMOOTHER_F32)
    return fail(ctx, PDH_EINVAL, "pdh_set_smoother_precision: precision must be PDH_SMOOTHER_F64 or PDH_SMOOTHER_F32");
  if (ctx->prec_kind == PDH_PREC_MULTIGRID)
    return fail(ctx, PDH_ESTATE, "pdh_set_smoother_precision: the context has a multigrid preconditioner attached; choose the precision of "
                                 "every level before pdh_mg_create");
  if (ctx->prec_kind != PDH_PREC_CHEBYSHEV || ctx->mg_gone)
    return fail(ctx, PDH_ESTATE, "pdh_set_smoother_precision: the preconditioner set up last is not PDH_PREC_CHEBYSHEV");
  PDH_TRY(pdh_prec_checks(ctx));
  pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  if (precision == PDH_SMOOTHER_F64)
    {
      S.f32 = false; // (the buffers stay, grow-only like the others)
      ++ctx->prec_epoch;
      return PDH_OK;
    }
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_TRY(shadow_bases(ctx));
  const bool block = S.cheb_inner == PDH_PREC_BLOCK_JACOBI;
  const int64_t n = ctx->prob.dev.n, n_inv = block ? ctx->prob.n_owned * n * n : 0;
  float *values = S.sh_values.get<float>((size_t)S.sh_count);
  float *dinv32 = block ? S.sh_dinv.get<float>((size_t)n_inv) : nullptr;
  if (!values || (block && !dinv32))
    return fail(ctx, PDH_EDEVICE, "pdh_set_smoother_precision: out of device memory"); // (F64 stays in force, the set-up valid)
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, pdh_launch_shadow_rows(&A, S.sh_base.ptr<int64_t>(), values, ctx->stream));
  if (block)
    PDH_HIP(ctx, pdh_launch_shadow_round(S.dinv.ptr<double>(), dinv32, n_inv, ctx->stream));
  S.f32 = true;
  ++ctx->prec_epoch;
  return PDH_OK;
}

extern "C" int pdh_smoother_precision(pdh_ctx *ctx)
{
  PDH_TRY(need_problem(ctx, "pdh_smoother_precision"));
  return ctx->prob.sol.f32 ? PDH_SMOOTHER_F32 : PDH_SMOOTHER_F64;
}

extern "C" int pdh_smoother_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y)
{
  PDH_TRY(vmult_checks(ctx, d_x, d_y));
  if (!ctx->prob.sol.f32)
    return fail(ctx, PDH_ESTATE, "pdh_smoother_vmult_device: PDH_SMOOTHER_F32 is not in force (pdh_set_smoother_precision)");
  if (ctx->prec_gen != ctx->values_gen)
    return fail(ctx, PDH_ESTATE, "the values changed since pdh_set_smoother_precision: set the smoother up again");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = pdh_solve_args(ctx);
  const pdh_ctx::Problem::Solver &S = ctx->prob.sol; // (the shadow on its own, whichever operator the smoother applies)
  const PdhShadowArgs Sh{S.sh_values.ptr<float>(), S.sh_base.ptr<int64_t>()};
  PDH_HIP(ctx, pdh_launch_vmult_f32(&A, &Sh, d_x, d_y, ctx->stream));
  return PDH_OK;
}

// ---- the operator of the smoother's products (include/polydeal_hip.h: pdh_set_smoother_operator; kernels: pdh_matfree.h) ----------------
extern "C" int pdh_set_smoother_operator(pdh_ctx *ctx, int op)
{
  PDH_TRY(need_problem(ctx, "pdh_set_smoother_operator"));
  if (op != PDH_SMOOTHER_OP_STORED && op != PDH_SMOOTHER_OP_MATRIX_FREE)
    return fail(ctx, PDH_EINVAL, "pdh_set_smoother_operator: op must be PDH_SMOOTHER_OP_STORED or PDH_SMOOTHER_OP_MATRIX_FREE");
  if (ctx->prec_kind == PDH_PREC_MULTIGRID)
    return fail(ctx, PDH_ESTATE, "pdh_set_smoother_operator: the context has a multigrid preconditioner attached; choose the operator of "
                                 "every level before pdh_mg_create");
  if (ctx->prec_kind != PDH_PREC_CHEBYSHEV || ctx->mg_gone)
    return fail(ctx, PDH_ESTATE, "pdh_set_smoother_operator: the preconditioner set up last is not PDH_PREC_CHEBYSHEV");
  PDH_TRY(pdh_prec_checks(ctx));
  if (op == PDH_SMOOTHER_OP_MATRIX_FREE)
    {
      if (!ctx->prob.d_mf_tables)
        return fail(ctx, PDH_ESTATE, "pdh_set_smoother_operator: the matrix-free operator is not set up (pdh_setup_matrix_free)");
      // the tables are the SIP assembly of the resident description: they do not stand for values written by anything else
      if (!ctx->prob.has_values || ctx->prob.galerkin_values)
        return fail(ctx, PDH_ESTATE, ctx->prob.galerkin_values
                                       ? "pdh_set_smoother_operator: the values of this context were written by pdh_galerkin_device; the "
                                         "matrix-free operator is the SIP assembly of the resident description"
                                       : "pdh_set_smoother_operator: the values of this context were never assembled");
    }
  ctx->prob.sol.matrix_free = op == PDH_SMOOTHER_OP_MATRIX_FREE;
  ++ctx->prec_epoch;
  return PDH_OK;
}

extern "C" int pdh_smoother_operator(pdh_ctx *ctx)
{
  PDH_TRY(need_problem(ctx, "pdh_smoother_operator"));
  return ctx->prob.sol.matrix_free ? PDH_SMOOTHER_OP_MATRIX_FREE : PDH_SMOOTHER_OP_STORED;
}

// ---- dense direct solve (include/polydeal_hip.h: pdh_setup_direct; steps and layout: pdh_dense.h) ---------------------------------------
extern "C" int pdh_setup_direct(pdh_ctx *ctx, pdh_direct_info *info)
{
  PDH_TRY(need_problem(ctx, "pdh_setup_direct"));
  PDH_TRY(all_rows_checks(ctx, "pdh_setup_direct", "it needs", "it", ""));
  const int64_t N = ctx->prob.n_rows_owned;
  if (N > PDH_DENSE_MAX_ROWS)
    return fail(ctx, PDH_EUNSUPPORTED, "pdh_setup_direct: the problem has " + std::to_string(N) + " rows, the dense direct solve takes at most " +
                                         std::to_string(PDH_DENSE_MAX_ROWS));
  if (N < 1)
    return fail(ctx, PDH_EINVAL, "pdh_setup_direct: the problem has no rows");
  new_setup(ctx);
  ctx->prec_kind = PDH_PREC_DIRECT;
  ctx->prec_gen = ctx->values_gen;
  ctx->prec_ok = false; // until the set-up below has succeeded
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  const int ld = pdh_dense_ld(N);
  const size_t nn = (size_t)ld * ld;
  DevBuf work; // U, Wd, dg [ld], piv [2]: gone when the set-up returns
  double *G = S.dense_g.get<double>(nn), *U = work.get<double>(2 * nn + ld + 2);
  int32_t *flag = S.flag.get<int32_t>((size_t)std::max(ctx->prob.n_owned, 1));
  if (!G || !U || !flag)
    return fail(ctx, PDH_EDEVICE, "pdh_setup_direct: out of device memory");
  double *Wd = U + nn, *dg = Wd + nn, *piv = dg + ld;
  S.dense_ld = ld;
  S.dense_n = (int)N;
  const PdhSolveArgs A = pdh_solve_args(ctx);
  PDH_HIP(ctx, hipMemsetAsync(U, 0, nn * sizeof(double), ctx->stream));
  PDH_HIP(ctx, pdh_launch_dense_gather(&A, U, ld, (int)N, ctx->stream));
  PDH_HIP(ctx, pdh_launch_dense_cholesky(U, ld, (int)N, dg, piv, flag, ctx->stream));
  int32_t h_flag = 0;
  double h_piv[2] = {0.0, 0.0};
  PDH_HIP(ctx, hipMemcpyAsync(&h_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(h_piv, piv, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (h_flag)
    return fail(ctx, PDH_EINVAL, "pdh_setup_direct: the matrix is not positive definite (the Cholesky pivot of row " + std::to_string(h_flag - 1) +
                                   " is <= 0 or not finite)");
  PDH_HIP(ctx, pdh_launch_dense_inverse(U, dg, ld, (int)N, Wd, G, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `work` is freed on return
  ctx->prec_ok = true;
  if (info)
    {
      info->n_rows = (int32_t)N;
      info->pivot_min = h_piv[0];
      info->pivot_max = h_piv[1];
    }
  return PDH_OK;
}
