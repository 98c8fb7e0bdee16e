// pdh_capi_mg.cpp — device driver of the C ABI, the multigrid V-cycle (no kernel of its own): it composes the Chebyshev smoother, the
// residual and the preconditioner apply of pdh_capi_solve.cpp and the level transfers of pdh_capi_transfer.cpp, every launch of every
// level on the FINEST context's stream.  The reference: the V-cycle of examples/simplex_agglomerated_multigrid.cc:378-515.
#include "pdh_ctx.h"
#include "pdh_launch.h"

struct pdh_mg
{
  struct Level
  {
    pdh_ctx *ctx = nullptr;
    int64_t n_rows = 0;
    uint64_t values_gen = 0, prec_epoch = 0; // as pdh_mg_create found them
    DevBuf b, x, r;                          // the mg's own level vectors (finest: r only; coarsest: b and x)
  };
  int n = 0;
  Level *levels = nullptr;               // [n] coarse to fine
  std::vector<pdh_transfer *> transfers; // [l]: level l <-> l + 1
  pdh_ctx *finest = nullptr;
  bool attached = false;
  ~pdh_mg() { delete[] levels; }
};

void pdh_mg_detach(pdh_ctx *ctx)
{
  if (!ctx || !ctx->mg)
    return;
  ctx->mg->attached = false;
  ctx->mg = nullptr;
  if (ctx->prec_kind == PDH_PREC_MULTIGRID)
    ctx->prec_kind = PDH_PREC_NONE;
}

static std::string level_name(int l, int n_levels) { return "level " + std::to_string(l) + " of " + std::to_string(n_levels); }

int pdh_mg_checks(pdh_mg *mg)
{
  pdh_ctx *report = mg->finest;
  const int n = mg->n;
  if (!mg->attached || report->mg != mg)
    return fail(report, PDH_ESTATE, "the multigrid preconditioner is detached: the preconditioner of the finest context (" + level_name(n - 1, n) +
                                      ") was replaced since pdh_mg_create");
  for (int l = 0; l < n; ++l)
    {
      const pdh_mg::Level &L = mg->levels[(size_t)l];
      if (!L.ctx->prob.resident || L.ctx->values_gen != L.values_gen)
        return fail(report, PDH_ESTATE, "multigrid: the values of " + level_name(l, n) + " changed since pdh_mg_create: create the pdh_mg again");
      if (L.ctx->prec_epoch != L.prec_epoch)
        return fail(report, PDH_ESTATE, "multigrid: the preconditioner of " + level_name(l, n) + " changed since pdh_mg_create: create the pdh_mg again");
    }
  return PDH_OK;
}

extern "C" int pdh_mg_create(int n_levels, pdh_ctx *const *levels, pdh_transfer *const *transfers, pdh_mg **out)
{
  if (!out)
    return fail(nullptr, PDH_EINVAL, "pdh_mg_create: out is required");
  *out = nullptr;
  if (!levels || n_levels < 1 || !levels[n_levels - 1])
    return fail(nullptr, PDH_EINVAL, "pdh_mg_create: levels and the finest context are required");
  pdh_ctx *fin = levels[n_levels - 1]; // every refusal is reported here
  if (n_levels < 2 || n_levels > 16)
    return fail(fin, PDH_EINVAL, "pdh_mg_create: " + std::to_string(n_levels) + " levels; a hierarchy has 2 .. 16");
  if (!transfers)
    return fail(fin, PDH_EINVAL, "pdh_mg_create: transfers are required");
  for (int l = 0; l < n_levels; ++l)
    {
      pdh_ctx *c = levels[l];
      const std::string who = "pdh_mg_create: " + level_name(l, n_levels);
      if (!c)
        return fail(fin, PDH_EINVAL, who + " is NULL");
      for (int m = 0; m < l; ++m)
        if (levels[m] == c)
          return fail(fin, PDH_EINVAL, who + " is the context of level " + std::to_string(m) + " too");
      if (c->device != fin->device)
        return fail(fin, PDH_EINVAL, who + " lives on device " + std::to_string(c->device) + ", the finest on device " + std::to_string(fin->device));
      if (!c->prob.resident)
        return fail(fin, PDH_ESTATE, who + " has no resident problem");
      if (c->prob.ghost || c->prob.n_rows_owned != c->prob.n_rows_total)
        return fail(fin, PDH_EINVAL, who + " does not own all rows with PDH_EXCHANGE_NONE");
      if (pdh_row_fits_lds(c) != PDH_OK)
        return fail(fin, PDH_EINVAL, who + ": " + std::string(c->err)); // (a copy: c may be fin)
      const bool current = c->prec_ok && !c->mg_gone && c->prec_gen == c->values_gen;
      if (l > 0 && c->prec_kind != PDH_PREC_CHEBYSHEV)
        return fail(fin, PDH_ESTATE, who + " needs PDH_PREC_CHEBYSHEV as its smoother (pdh_setup_chebyshev)");
      if (l == 0 && (c->prec_kind == PDH_PREC_NONE || c->prec_kind == PDH_PREC_MULTIGRID))
        return fail(fin, PDH_ESTATE, who + ", the coarsest, needs a preconditioner set up as its solver (pdh_setup_direct, or pdh_setup_chebyshev / "
                                           "pdh_setup_preconditioner beyond 1024 rows)");
      if (!current)
        return fail(fin, PDH_ESTATE, who + ": its preconditioner is not current (the values changed since its set-up, or the set-up failed)");
    }
  for (int l = 0; l + 1 < n_levels; ++l)
    {
      const std::string who = "pdh_mg_create: transfer " + std::to_string(l) + " (" + level_name(l, n_levels) + " <-> " + std::to_string(l + 1) + ")";
      if (!transfers[l])
        return fail(fin, PDH_EINVAL, who + " is NULL");
      pdh_ctx *tc = nullptr;
      int64_t nf = 0, nc = 0;
      pdh_transfer_info(transfers[l], &tc, &nf, &nc);
      if (tc != levels[l + 1])
        return fail(fin, PDH_EINVAL, who + " was not created on the context of its finer level");
      if (nf != levels[l + 1]->prob.n_rows_total || nc != levels[l]->prob.n_rows_total)
        return fail(fin, PDH_EINVAL, who + " connects " + std::to_string(nc) + " and " + std::to_string(nf) + " rows, the levels have " +
                                       std::to_string(levels[l]->prob.n_rows_total) + " and " + std::to_string(levels[l + 1]->prob.n_rows_total));
    }
  PDH_HIP(fin, hipSetDevice(fin->device));
  pdh_mg *mg = new pdh_mg;
  mg->finest = fin;
  mg->n = n_levels;
  mg->levels = new pdh_mg::Level[(size_t)n_levels];
  mg->transfers.assign(transfers, transfers + (n_levels - 1));
  for (int l = 0; l < n_levels; ++l)
    {
      pdh_mg::Level &L = mg->levels[(size_t)l];
      L.ctx = levels[l];
      L.n_rows = levels[l]->prob.n_rows_total;
      L.values_gen = levels[l]->values_gen;
      L.prec_epoch = levels[l]->prec_epoch;
      const bool ok = L.r.get<double>((size_t)L.n_rows) && (l == n_levels - 1 || (L.b.get<double>((size_t)L.n_rows) && L.x.get<double>((size_t)L.n_rows)));
      if (!ok)
        {
          delete mg;
          return fail(fin, PDH_EDEVICE, "pdh_mg_create: out of device memory");
        }
    }
  for (int l = 0; l < n_levels; ++l) // what the levels' own streams still hold (set-up, assembly) is done before the first cycle
    if (hipStreamSynchronize(levels[l]->stream) != hipSuccess)
      {
        delete mg;
        return fail(fin, PDH_EDEVICE, "pdh_mg_create: hipStreamSynchronize of " + level_name(l, n_levels));
      }
  pdh_mg_detach(fin); // an earlier mg of the same finest context
  fin->mg = mg;
  fin->mg_gone = false;
  fin->prec_kind = PDH_PREC_MULTIGRID; // (its Chebyshev data stays: the smoother of the finest level; no new epoch)
  mg->attached = true;
  *out = mg;
  return PDH_OK;
}

extern "C" void pdh_mg_destroy(pdh_mg *mg)
{
  if (!mg)
    return;
  pdh_ctx *fin = mg->finest;
  (void)hipSetDevice(fin->device);
  if (mg->attached && fin->mg == mg)
    {
      (void)hipStreamSynchronize(fin->stream); // a cycle may still be queued on the vectors freed below
      pdh_mg_detach(fin);
      fin->mg_gone = true;
      fin->prec_ok = false;
    }
  delete mg;
}

int pdh_mg_cycle(pdh_mg *mg, const double *b, double *x, bool zero, const double *rcg, double *part)
{
  pdh_ctx *fin = mg->finest;
  const hipStream_t st = fin->stream; // as it stands at this call, for every level
  const int n = mg->n;
  std::vector<PdhSolveArgs> A((size_t)n);
  for (int l = 0; l < n; ++l)
    A[(size_t)l] = pdh_solve_args(mg->levels[(size_t)l].ctx);
  auto bl = [&](int l) { return l == n - 1 ? b : mg->levels[(size_t)l].b.ptr<double>(); };
  auto xl = [&](int l) { return l == n - 1 ? x : mg->levels[(size_t)l].x.ptr<double>(); };
  for (int l = n - 1; l >= 1; --l)
    {
      pdh_mg::Level &L = mg->levels[(size_t)l];
      double *r = L.r.ptr<double>();
      PDH_TRY(pdh_cheb_apply(L.ctx, fin, A[(size_t)l], bl(l), xl(l), l < n - 1 || zero, nullptr, nullptr, st)); // pre-smoothing
      PDH_TRY(pdh_smoother_vmult(L.ctx, fin, A[(size_t)l], xl(l), r, st)); // r = b - A x, with the matrix the level's smoother reads
      PDH_HIP(fin, pdh_launch_residual_sub(L.n_rows, bl(l), r, st));
      PDH_HIP(fin, pdh_transfer_launch(mg->transfers[(size_t)l - 1], true, 0, r, mg->levels[(size_t)l - 1].b.ptr<double>(), st));
    }
  PDH_TRY(pdh_prec_apply(mg->levels[0].ctx, fin, A[0], bl(0), xl(0), nullptr, nullptr, st)); // the coarsest level's solver
  for (int l = 1; l < n; ++l)
    {
      pdh_mg::Level &L = mg->levels[(size_t)l];
      PDH_HIP(fin, pdh_transfer_launch(mg->transfers[(size_t)l - 1], false, 1, xl(l - 1), xl(l), st)); // x += P x_coarse
      const bool last = l == n - 1;
      PDH_TRY(pdh_cheb_apply(L.ctx, fin, A[(size_t)l], bl(l), xl(l), false, last ? rcg : nullptr, last ? part : nullptr, st)); // post-smoothing
    }
  return PDH_OK;
}

extern "C" int pdh_mg_vcycle_device(pdh_mg *mg, const double *d_b, double *d_x, int zero_initial_guess)
{
  if (!mg)
    return fail(nullptr, PDH_EINVAL, "mg is NULL");
  pdh_ctx *fin = mg->finest;
  if (!d_b || !d_x)
    return fail(fin, PDH_EINVAL, "b and x are required");
  const int64_t N = mg->levels[mg->n - 1].n_rows;
  const char *pb = reinterpret_cast<const char *>(d_b), *px = reinterpret_cast<const char *>(d_x);
  if (pb < px + N * (int64_t)sizeof(double) && px < pb + N * (int64_t)sizeof(double))
    return fail(fin, PDH_EINVAL, "b and x overlap");
  PDH_TRY(pdh_mg_checks(mg));
  PDH_HIP(fin, hipSetDevice(fin->device));
  return pdh_mg_cycle(mg, d_b, d_x, zero_initial_guess != 0, nullptr, nullptr);
}
