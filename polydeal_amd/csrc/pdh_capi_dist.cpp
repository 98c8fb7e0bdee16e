// pdh_capi_dist.cpp — device driver of the C ABI, solving over several ranks (kernels: pdh_dist.hip; plan: pdh_halo_plan.cpp): the halo of
// a rank's local vector, y = A v on local vectors, and CG by reverse communication.  The recurrence is CgRun's (pdh_cg_run.h), the one
// of pdh_solve_cg: this unit queues its pieces between the requests it hands to the caller's transport and calls no transport itself.
#include "pdh_cg_run.h"
#include "pdh_ctx.h"
#include "pdh_dist.h"
#include "pdh_launch.h"

#include <cmath>

static bool overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
  const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
  return pa < pb + nb * (int64_t)sizeof(double) && pb < pa + na * (int64_t)sizeof(double);
}

template <class T>
static int fill(pdh_ctx *ctx, DevBuf &buf, const std::vector<T> &h, const char *what)
{
  T *d = buf.get<T>(h.size());
  if (!d)
    return fail(ctx, PDH_EDEVICE, std::string("pdh_halo_setup: out of device memory (") + what + ")");
  if (!h.empty())
    PDH_HIP(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return PDH_OK;
}

extern "C" int pdh_halo_setup(pdh_ctx *ctx, int n_ranks, const int32_t *row_splits, int64_t *send_count, int64_t *recv_count,
                              pdh_halo_info *info)
{
  PDH_TRY(need_problem(ctx, "pdh_halo_setup"));
  if (!send_count || !recv_count || !info)
    return fail(ctx, PDH_EINVAL, "pdh_halo_setup: send_count, recv_count and info are required");
  if (ctx->prob.ghost)
    return fail(ctx, PDH_EUNSUPPORTED, "pdh_halo_setup: the problem was set in PDH_EXCHANGE_GHOST mode; the vector halo serves "
                                       "PDH_EXCHANGE_NONE only");
  if (ctx->prob.dcg)
    return fail(ctx, PDH_ESTATE, "pdh_halo_setup: a pdh_dcg run is open on this context");
  pdh_ctx::Problem &P = ctx->prob;
  pdh_ctx::Problem::Halo &H = P.halo;
  H.ready = false;
  // the owned range is contiguous and made of whole polytopes: it starts at the lowest first dof of an owned slot
  int32_t row_begin = 0;
  const int n = P.dev.n;
  if (P.n_owned > 0)
    row_begin = *std::min_element(P.h_slot_dof.begin(), P.h_slot_dof.end());
  else if (n_ranks >= 1 && row_splits)
    row_begin = row_splits[0]; // (a context without rows: any empty range will do)
  const int32_t row_end = (int32_t)(row_begin + P.n_rows_owned);
  PdhHaloPlan plan;
  PDH_TRY(pdh_plan_halo(ctx->err, n, row_begin, row_end, P.n_owned, P.h_blk_ptr.data(), P.h_blk_dof.data(), P.h_slot_dof.data(), n_ranks,
                        row_splits, plan));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a second set-up replaces tables a queued kernel may still read)
  std::vector<int32_t> slots(plan.slots_all);
  slots.insert(slots.end(), plan.slots_interior.begin(), plan.slots_interior.end());
  slots.insert(slots.end(), plan.slots_boundary.begin(), plan.slots_boundary.end());
  PDH_TRY(fill(ctx, H.blk_loc, plan.blk_loc, "block table"));
  PDH_TRY(fill(ctx, H.pack_src, plan.pack_src, "send blocks"));
  PDH_TRY(fill(ctx, H.slots, slots, "slot lists"));
  H.n_ranks = n_ranks;
  H.n_interior = (int)plan.slots_interior.size();
  H.n_boundary = (int)plan.slots_boundary.size();
  H.n_owned_rows = plan.n_owned_rows;
  H.n_ghost_rows = plan.n_ghost_rows;
  H.n_send = (int64_t)plan.pack_src.size() * n;
  H.n_recv = plan.n_ghost_rows;
  for (int r = 0; r < n_ranks; ++r)
    {
      send_count[r] = plan.send_count[(size_t)r];
      recv_count[r] = plan.recv_count[(size_t)r];
    }
  info->n_owned_rows = H.n_owned_rows;
  info->n_ghost_rows = H.n_ghost_rows;
  info->n_interior = H.n_interior;
  info->n_boundary = H.n_boundary;
  H.ready = true;
  return PDH_OK;
}

static int need_halo(pdh_ctx *ctx, const char *name)
{
  PDH_TRY(need_problem(ctx, name));
  return ctx->prob.halo.ready ? PDH_OK : fail(ctx, PDH_ESTATE, std::string(name) + ": the halo is not set up (pdh_halo_setup)");
}

static hipError_t pack(pdh_ctx *ctx, const double *d_v, double *d_send)
{
  const pdh_ctx::Problem::Halo &H = ctx->prob.halo;
  const int n = ctx->prob.dev.n;
  return pdh_launch_halo_pack(n, H.n_send / n, H.pack_src.ptr<int64_t>(), d_v, d_send, ctx->stream);
}

extern "C" int pdh_halo_pack_device(pdh_ctx *ctx, const double *d_v, double *d_send)
{
  PDH_TRY(need_halo(ctx, "pdh_halo_pack_device"));
  const pdh_ctx::Problem::Halo &H = ctx->prob.halo;
  if (!d_v || (!d_send && H.n_send > 0))
    return fail(ctx, PDH_EINVAL, "pdh_halo_pack_device: d_v and d_send are required");
  if (H.n_send > 0 && overlap(d_v, H.n_owned_rows + H.n_ghost_rows, d_send, H.n_send))
    return fail(ctx, PDH_EINVAL, "pdh_halo_pack_device: d_v and d_send overlap");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, pack(ctx, d_v, d_send));
  return PDH_OK;
}

// the product on the local vector over one of the three slot lists
static hipError_t vmult_local(pdh_ctx *ctx, const PdhSolveArgs &A, int which, const double *d_v, double *d_y, double *part)
{
  const pdh_ctx::Problem::Halo &H = ctx->prob.halo;
  PdhSolveArgs L = A;
  L.blk_dof = H.blk_loc.ptr<int32_t>();
  const int32_t *slots = H.slots.ptr<int32_t>();
  const int n_all = ctx->prob.n_owned;
  if (which == PDH_ROWS_INTERIOR)
    return pdh_launch_vmult_local(&L, slots + n_all, H.n_interior, d_v, d_y, part, ctx->stream);
  if (which == PDH_ROWS_BOUNDARY)
    return pdh_launch_vmult_local(&L, slots + n_all + H.n_interior, H.n_boundary, d_v, d_y, part, ctx->stream);
  return pdh_launch_vmult_local(&L, slots, n_all, d_v, d_y, part, ctx->stream);
}

extern "C" int pdh_vmult_local_device(pdh_ctx *ctx, const double *d_v, double *d_y, int which)
{
  PDH_TRY(need_halo(ctx, "pdh_vmult_local_device"));
  const pdh_ctx::Problem::Halo &H = ctx->prob.halo;
  if (!d_v || !d_y)
    return fail(ctx, PDH_EINVAL, "v and y are required");
  if (which != PDH_ROWS_ALL && which != PDH_ROWS_INTERIOR && which != PDH_ROWS_BOUNDARY)
    return fail(ctx, PDH_EINVAL, "pdh_vmult_local_device: which must be PDH_ROWS_ALL, PDH_ROWS_INTERIOR or PDH_ROWS_BOUNDARY");
  if (overlap(d_v, H.n_owned_rows + H.n_ghost_rows, d_y, H.n_owned_rows))
    return fail(ctx, PDH_EINVAL, "v and y overlap");
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, vmult_local(ctx, pdh_solve_args(ctx), which, d_v, d_y, nullptr));
  return PDH_OK;
}

// ---- CG by reverse communication ------------------------------------------------------------------------------------------------------
// The open run: CgRun plus where the run stands.  `asked`: the request handed out last.  Stage of the sums on their way: 0 the start
// (rz, rr, bb), 1 p^T A p, 2 (rz, rr).  first: the halo on its way is that of x0 (held in the local vector p until p = z replaces it).
struct PdhDcgRun
{
  CgRun cg;
  pdh_cg_control ctl;
  const double *b;
  double *x;
  int asked = PDH_DCG_DONE, stage = 0, it = 0;
  bool first = true;
  double rr = 0.0, stop = 0.0, residual0 = 0.0;
  uint64_t values_gen = 0, prec_epoch = 0;
  PdhDcgRun(pdh_ctx *c, int kind, int64_t n_ghost, const pdh_cg_control &ctl_, const double *b_, double *x_)
    : cg(c, kind, PDH_PREC_NONE, n_ghost), ctl(ctl_), b(b_), x(x_), values_gen(c->values_gen), prec_epoch(c->prec_epoch)
  {}
};

static void ask_halo(pdh_ctx *ctx, PdhDcgRun &R, int kind, pdh_dcg_request *next)
{
  *next = pdh_dcg_request{};
  next->kind = kind;
  next->d_send = kind == PDH_DCG_HALO_BEGIN ? ctx->prob.halo.send.ptr<double>() : nullptr;
  next->d_recv = R.cg.p + R.cg.N;
  R.asked = kind;
}

static int ask_sum(pdh_ctx *ctx, PdhDcgRun &R, int stage, pdh_dcg_request *next)
{
  double *red = ctx->prob.halo.red.ptr<double>();
  PDH_TRY(R.cg.local_sum(stage, red));
  *next = pdh_dcg_request{};
  next->kind = PDH_DCG_ALLREDUCE;
  next->d_scalars = red;
  next->n_scalars = stage == 0 ? 3 : stage == 1 ? 1 : 2;
  R.asked = PDH_DCG_ALLREDUCE;
  R.stage = stage;
  return PDH_OK;
}

// the stop test of pdh_solve_cg: go on with the halo of p, or end the run
static int test_and_go(pdh_ctx *ctx, PdhDcgRun &R, pdh_dcg_request *next, pdh_cg_result *res, bool *done)
{
  if (R.it < R.ctl.max_iter && std::sqrt(R.rr) > R.stop)
    {
      PDH_HIP(ctx, pack(ctx, R.cg.p, ctx->prob.halo.send.ptr<double>()));
      R.first = false;
      ask_halo(ctx, R, PDH_DCG_HALO_BEGIN, next);
      return PDH_OK;
    }
  *done = true;
  *next = pdh_dcg_request{};
  next->kind = PDH_DCG_DONE;
  res->iterations = R.it;
  res->residual0 = R.residual0;
  res->residual = std::sqrt(R.rr);
  if (!(res->residual <= R.stop))
    return fail(ctx, PDH_ENOCONV, "pdh_dcg: no convergence in " + std::to_string(R.it) + " iterations (||r|| = " +
                                    std::to_string(res->residual) + ", bound " + std::to_string(R.stop) + ")");
  return PDH_OK;
}

static const char *unsupported_kind(const pdh_ctx *ctx)
{
  const pdh_ctx::Problem::Solver &S = ctx->prob.sol;
  switch (ctx->prec_kind)
    {
    case PDH_PREC_CHEBYSHEV:
      return S.matrix_free ? "PDH_PREC_CHEBYSHEV with the matrix-free smoother operator"
                           : S.f32 ? "PDH_PREC_CHEBYSHEV with the float32 smoother" : "PDH_PREC_CHEBYSHEV";
    case PDH_PREC_DIRECT: return "PDH_PREC_DIRECT";
    case PDH_PREC_MULTIGRID: return "PDH_PREC_MULTIGRID";
    default: return nullptr;
    }
}

extern "C" int pdh_dcg_begin(pdh_ctx *ctx, const pdh_cg_control *c, const double *d_b, double *d_x, pdh_dcg_request *next)
{
  PDH_TRY(need_problem(ctx, "pdh_dcg_begin"));
  if (!c || !d_b || !d_x || !next)
    return fail(ctx, PDH_EINVAL, "control, b, x and next are required");
  if (c->max_iter < 0 || !(c->rel_tol >= 0.0) || !(c->abs_tol >= 0.0))
    return fail(ctx, PDH_EINVAL, "max_iter, rel_tol and abs_tol must be non-negative");
  PDH_TRY(need_halo(ctx, "pdh_dcg_begin"));
  if (ctx->prob.dcg)
    return fail(ctx, PDH_ESTATE, "pdh_dcg_begin: a run is open on this context (it ends at PDH_DCG_DONE or at an error)");
  if (const char *kind = unsupported_kind(ctx))
    return fail(ctx, PDH_EUNSUPPORTED, std::string("pdh_dcg_begin: ") + kind + " is not a rank-local preconditioner (its inner products would "
                                         "each need a halo); CG over the ranks takes PDH_PREC_NONE, PDH_PREC_JACOBI and PDH_PREC_BLOCK_JACOBI");
  const pdh_ctx::Problem::Halo &H = ctx->prob.halo;
  if (overlap(d_b, H.n_owned_rows, d_x, H.n_owned_rows))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  PDH_TRY(pdh_prec_checks(ctx));
  PDH_TRY(pdh_row_fits_lds(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  auto run = std::make_shared<PdhDcgRun>(ctx, ctx->prec_kind, H.n_ghost_rows, *c, d_b, d_x);
  double *send = ctx->prob.halo.send.get<double>((size_t)H.n_send), *red = ctx->prob.halo.red.get<double>(3);
  if (!run->cg.ok() || !send || !red)
    return fail(ctx, PDH_EDEVICE, "pdh_dcg_begin: out of device memory");
  // the local vector of x0 lives in p until the first direction replaces it
  CgRun &cg = run->cg;
  PDH_HIP(ctx, hipMemcpyAsync(cg.p, d_x, cg.N * sizeof(double), hipMemcpyDeviceToDevice, cg.st));
  PDH_HIP(ctx, pack(ctx, cg.p, send));
  ask_halo(ctx, *run, PDH_DCG_HALO_BEGIN, next);
  ctx->prob.dcg = run;
  return PDH_OK;
}

static int resume(pdh_ctx *ctx, PdhDcgRun &R, pdh_dcg_request *next, pdh_cg_result *res, bool *done)
{
  CgRun &cg = R.cg;
  if (R.asked == PDH_DCG_HALO_BEGIN)
    { // the move is under way: the rows that need no ghost value
      PDH_HIP(ctx, vmult_local(ctx, cg.A, PDH_ROWS_INTERIOR, cg.p, cg.q, R.first ? nullptr : cg.pq_part()));
      ask_halo(ctx, R, PDH_DCG_HALO_END, next);
      return PDH_OK;
    }
  if (R.asked == PDH_DCG_HALO_END)
    {
      PDH_HIP(ctx, vmult_local(ctx, cg.A, PDH_ROWS_BOUNDARY, cg.p, cg.q, R.first ? nullptr : cg.pq_part()));
      if (R.first)
        PDH_TRY(cg.first_residual(R.b));
      return ask_sum(ctx, R, R.first ? 0 : 1, next);
    }
  // PDH_DCG_ALLREDUCE: the sums of all ranks are in `red`
  const double *red = ctx->prob.halo.red.ptr<double>();
  PDH_TRY(cg.finish(R.stage, red));
  if (R.stage == 1)
    {
      PDH_TRY(cg.update(R.x));
      return ask_sum(ctx, R, 2, next);
    }
  PDH_TRY(cg.direction(R.stage == 0 ? 1 : 0));
  if (R.stage == 0)
    {
      PDH_TRY(cg.read_back(PDH_CG_RR, 2));
      R.rr = ctx->pinned[0];
      R.stop = std::max(R.ctl.abs_tol, R.ctl.rel_tol * std::sqrt(ctx->pinned[1]));
      R.residual0 = std::sqrt(R.rr);
    }
  else
    {
      PDH_TRY(cg.read_back(PDH_CG_RR, 1));
      R.rr = ctx->pinned[0];
      ++R.it;
    }
  return test_and_go(ctx, R, next, res, done);
}

extern "C" int pdh_dcg_resume(pdh_ctx *ctx, pdh_dcg_request *next, pdh_cg_result *res)
{
  PDH_TRY(need_problem(ctx, "pdh_dcg_resume"));
  if (!next || !res)
    return fail(ctx, PDH_EINVAL, "next and result are required");
  std::shared_ptr<PdhDcgRun> run = ctx->prob.dcg;
  if (!run)
    return fail(ctx, PDH_ESTATE, "pdh_dcg_resume: no run is open on this context (pdh_dcg_begin)");
  int rc = PDH_OK;
  bool done = false;
  if (run->values_gen != ctx->values_gen)
    rc = fail(ctx, PDH_ESTATE, "pdh_dcg_resume: the values changed during the run; it is closed");
  else if (run->prec_epoch != ctx->prec_epoch)
    rc = fail(ctx, PDH_ESTATE, "pdh_dcg_resume: the preconditioner changed during the run; it is closed");
  else if (hipSetDevice(ctx->device) != hipSuccess)
    rc = fail(ctx, PDH_EDEVICE, "pdh_dcg_resume: hipSetDevice");
  else
    rc = resume(ctx, *run, next, res, &done);
  if (rc != PDH_OK || done)
    ctx->prob.dcg.reset(); // (the vectors are the context's grow-only buffers: nothing else to free)
  return rc;
}
