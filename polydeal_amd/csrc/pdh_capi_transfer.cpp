// pdh_capi_transfer.cpp — device driver of the C ABI, level transfers (kernels: pdh_transfer.hip; planner: pdh_transfer_plan.cpp).  A
// transfer owns its tables on the device of the context it was created on and launches on that context's stream; it needs no resident
// problem there.  The Galerkin product of the two levels a transfer connects (kernel: pdh_galerkin.hip; planner: pdh_galerkin_plan.cpp)
// is the one entry that does: it reads the resident rows of the transfer's context and writes those of the coarse one.  A p-transfer
// (pdh_ptransfer_create; kernels: pdh_ptransfer.hip) is the same pdh_transfer of another kind: every entry dispatches on it.
#include "pdh_ctx.h"
#include "pdh_galerkin.h"
#include "pdh_launch.h"
#include "pdh_ptransfer.h"
#include "pdh_transfer.h"

struct pdh_transfer
{
  enum Kind { H_NESTED, P_DGQ, P_AGGLODGP };
  pdh_ctx *ctx = nullptr;
  Kind kind = H_NESTED;
  int dim = 0, n1d = 0;
  int64_t n_fine_rows = 0, n_coarse_rows = 0;
  PdhTransferArgs args{};   // H_NESTED
  PdhPTransferArgs pargs{}; // P_*
  std::vector<void *> allocs;                              // every hipMalloc of the set-up; args points into these
  DevBuf in{DevBuf::slack}, out{DevBuf::slack};            // staging copies of pdh_prolongate / pdh_restrict
  // pdh_galerkin_device: host copies of what its planner reads of the description, and the plan on the device - valid for the coarse
  // context and the two problems (pdh_ctx::problem_epoch) it was built for
  int degree = 0;
  std::vector<int32_t> parent, fine_off, coarse_off;
  std::vector<double> h_tab; // the tables as uploaded: the product applies its own copy of them (pdh_galerkin_tables)
  struct Galerkin
  {
    pdh_ctx *coarse = nullptr;
    uint64_t fine_epoch = 0, coarse_epoch = 0;
    std::vector<void *> allocs;
    PdhGalerkinArgs args{};
    void drop()
    {
      for (void *d : allocs)
        (void)hipFree(d);
      allocs.clear();
      coarse = nullptr;
    }
  } gal;
  ~pdh_transfer()
  {
    gal.drop();
    for (void *d : allocs)
      (void)hipFree(d);
  }
};

extern "C" int pdh_transfer_create(pdh_ctx *ctx, const pdh_transfer_desc *d, pdh_transfer **out)
{
  PDH_TRY(need_ctx(ctx));
  if (!out)
    return fail(ctx, PDH_EINVAL, "out is required");
  *out = nullptr;
  PdhTransferPlan plan;
  PDH_TRY(pdh_plan_transfer(ctx->err, d, plan));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  pdh_transfer *t = new pdh_transfer;
  t->ctx = ctx;
  t->dim = d->dim;
  t->n1d = d->degree + 1;
  t->n_fine_rows = d->n_fine_rows;
  t->n_coarse_rows = d->n_coarse_rows;
  t->degree = d->degree;
  t->parent.assign(d->parent, d->parent + d->n_fine);
  t->fine_off.assign(d->fine_dof_offset, d->fine_dof_offset + d->n_fine);
  t->coarse_off.assign(d->coarse_dof_offset, d->coarse_dof_offset + d->n_coarse);
  PdhTransferArgs &A = t->args;
  A.n_fine = d->n_fine;
  A.n_coarse = d->n_coarse;
  int rc = upload_in(ctx, t->allocs, plan.tab.data(), plan.tab.size(), &A.tab, "transfer tables");
  t->h_tab = std::move(plan.tab);
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, d->parent, (size_t)d->n_fine, &A.parent, "parent");
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, plan.child_ptr.data(), plan.child_ptr.size(), &A.child_ptr, "child_ptr");
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, plan.child_idx.data(), plan.child_idx.size(), &A.child_idx, "child_idx");
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, d->fine_dof_offset, (size_t)d->n_fine, &A.fine_off, "fine_dof_offset");
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, d->coarse_dof_offset, (size_t)d->n_coarse, &A.coarse_off, "coarse_dof_offset");
  if (rc != PDH_OK)
    {
      delete t;
      return rc;
    }
  *out = t;
  return PDH_OK;
}

extern "C" int pdh_ptransfer_create(pdh_ctx *ctx, const pdh_ptransfer_desc *d, pdh_transfer **out)
{
  PDH_TRY(need_ctx(ctx));
  if (!out)
    return fail(ctx, PDH_EINVAL, "out is required");
  *out = nullptr;
  PdhPTransferPlan plan;
  PDH_TRY(pdh_plan_ptransfer(ctx->err, d, plan));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  pdh_transfer *t = new pdh_transfer;
  t->ctx = ctx;
  t->kind = d->basis == PDH_BASIS_DGQ ? pdh_transfer::P_DGQ : pdh_transfer::P_AGGLODGP;
  t->dim = d->dim;
  t->n1d = d->fine_degree + 1;
  t->degree = d->fine_degree;
  t->n_fine_rows = d->n_fine_rows;
  t->n_coarse_rows = d->n_coarse_rows;
  PdhPTransferArgs &A = t->pargs;
  A.n_polytopes = d->n_polytopes;
  A.nf1d = d->fine_degree + 1;
  A.nc1d = d->coarse_degree + 1;
  A.n_f = plan.n_f;
  A.n_c = plan.n_c;
  std::copy(plan.B.begin(), plan.B.end(), A.B);
  int rc = upload_in(ctx, t->allocs, d->fine_dof_offset, (size_t)d->n_polytopes, &A.fine_off, "fine_dof_offset");
  if (rc == PDH_OK)
    rc = upload_in(ctx, t->allocs, d->coarse_dof_offset, (size_t)d->n_polytopes, &A.coarse_off, "coarse_dof_offset");
  if (rc == PDH_OK && t->kind == pdh_transfer::P_AGGLODGP)
    rc = upload_in(ctx, t->allocs, plan.map.data(), plan.map.size(), &A.map, "index map");
  if (rc == PDH_OK && t->kind == pdh_transfer::P_AGGLODGP)
    rc = upload_in(ctx, t->allocs, plan.inv.data(), plan.inv.size(), &A.inv, "inverse index map");
  if (rc != PDH_OK)
    {
      delete t;
      return rc;
    }
  *out = t;
  return PDH_OK;
}

extern "C" void pdh_transfer_destroy(pdh_transfer *t)
{
  if (!t)
    return;
  (void)hipSetDevice(t->ctx->device);
  delete t;
}

// for the V-cycle (pdh_capi_mg.cpp): what a transfer connects, and one of its launches on a stream of the caller's
void pdh_transfer_info(const pdh_transfer *t, pdh_ctx **ctx, int64_t *n_fine_rows, int64_t *n_coarse_rows)
{
  *ctx = t->ctx;
  *n_fine_rows = t->n_fine_rows;
  *n_coarse_rows = t->n_coarse_rows;
}

hipError_t pdh_transfer_launch(const pdh_transfer *t, bool restriction, int add, const double *src, double *dst, hipStream_t stream)
{
  if (t->kind != pdh_transfer::H_NESTED)
    return pdh_launch_ptransfer(t->dim, t->kind == pdh_transfer::P_DGQ, restriction, add, &t->pargs, src, dst, stream);
  return restriction ? pdh_launch_restrict(t->dim, t->n1d, add, &t->args, src, dst, stream)
                     : pdh_launch_prolongate(t->dim, t->n1d, add, &t->args, src, dst, stream);
}

static bool overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
  const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
  return pa < pb + nb * (int64_t)sizeof(double) && pb < pa + na * (int64_t)sizeof(double);
}

static int transfer_checks(pdh_transfer *t, const void *coarse, const void *fine)
{
  if (!t)
    return fail(nullptr, PDH_EINVAL, "transfer is NULL");
  if (!coarse || !fine)
    return fail(t->ctx, PDH_EINVAL, "the coarse and the fine vector are required");
  if (overlap(coarse, t->n_coarse_rows, fine, t->n_fine_rows))
    return fail(t->ctx, PDH_EINVAL, "the coarse and the fine vector overlap");
  return PDH_OK;
}

static int prolongate_device(pdh_transfer *t, const double *d_coarse, double *d_fine, int add)
{
  PDH_TRY(transfer_checks(t, d_coarse, d_fine));
  PDH_HIP(t->ctx, hipSetDevice(t->ctx->device));
  PDH_HIP(t->ctx, pdh_transfer_launch(t, false, add, d_coarse, d_fine, t->ctx->stream));
  return PDH_OK;
}

static int restrict_device(pdh_transfer *t, const double *d_fine, double *d_coarse, int add)
{
  PDH_TRY(transfer_checks(t, d_coarse, d_fine));
  PDH_HIP(t->ctx, hipSetDevice(t->ctx->device));
  PDH_HIP(t->ctx, pdh_transfer_launch(t, true, add, d_fine, d_coarse, t->ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_prolongate_device(pdh_transfer *t, const double *d_coarse, double *d_fine) { return prolongate_device(t, d_coarse, d_fine, 0); }
extern "C" int pdh_prolongate_and_add_device(pdh_transfer *t, const double *d_coarse, double *d_fine)
{
  return prolongate_device(t, d_coarse, d_fine, 1);
}
extern "C" int pdh_restrict_device(pdh_transfer *t, const double *d_fine, double *d_coarse) { return restrict_device(t, d_fine, d_coarse, 0); }
extern "C" int pdh_restrict_and_add_device(pdh_transfer *t, const double *d_fine, double *d_coarse)
{
  return restrict_device(t, d_fine, d_coarse, 1);
}

// host pointers: `n_in` doubles in, the device entry, `n_out` doubles back
template <class Call>
static int staged(pdh_transfer *t, const char *who, const double *in, int64_t n_in, double *out, int64_t n_out, Call &&call)
{
  pdh_ctx *ctx = t->ctx;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_in = nullptr, *d_out = nullptr;
  PDH_TRY(stage_in(ctx, who, t->in, in, (size_t)n_in, &d_in));
  PDH_TRY(stage(ctx, who, t->out, (size_t)n_out, &d_out));
  PDH_HIP(ctx, hipMemsetAsync(d_out, 0, n_out * sizeof(double), ctx->stream)); // rows that belong to no polytope come back as zeros
  PDH_TRY(call(d_in, d_out));
  PDH_HIP(ctx, hipMemcpyAsync(out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_prolongate(pdh_transfer *t, const double *coarse, double *fine)
{
  PDH_TRY(transfer_checks(t, coarse, fine));
  return staged(t, "pdh_prolongate", coarse, t->n_coarse_rows, fine, t->n_fine_rows,
                [&](const double *d_c, double *d_f) { return pdh_prolongate_device(t, d_c, d_f); });
}

extern "C" int pdh_restrict(pdh_transfer *t, const double *fine, double *coarse)
{
  PDH_TRY(transfer_checks(t, coarse, fine));
  return staged(t, "pdh_restrict", fine, t->n_fine_rows, coarse, t->n_coarse_rows,
                [&](const double *d_f, double *d_c) { return pdh_restrict_device(t, d_f, d_c); });
}

// ---- the Galerkin product ----
static pdh_galerkin_level galerkin_level(const pdh_ctx *ctx)
{
  const pdh_ctx::Problem &pr = ctx->prob;
  pdh_galerkin_level L;
  L.n_slots = pr.n_owned;
  L.n_rows_owned = (int32_t)pr.n_rows_owned;
  L.n_rows = (int32_t)pr.n_rows_total;
  L.exchange_mode = pr.ghost ? PDH_EXCHANGE_GHOST : PDH_EXCHANGE_NONE;
  L.device = ctx->device;
  L.blk_ptr = pr.h_blk_ptr.data();
  L.blk_dof = pr.h_blk_dof.data();
  L.dof_offset = pr.h_slot_dof.data();
  return L;
}

// the plan of (t, coarse) on the device: kept while both problems are the ones it was built for
static int galerkin_plan(pdh_transfer *t, pdh_ctx *coarse)
{
  pdh_ctx *fine = t->ctx;
  pdh_transfer::Galerkin &G = t->gal;
  if (G.coarse == coarse && G.fine_epoch == fine->problem_epoch && G.coarse_epoch == coarse->problem_epoch)
    return PDH_OK;
  G.drop();
  const pdh_galerkin_level Lf = galerkin_level(fine), Lc = galerkin_level(coarse);
  const PdhGalerkinPair T{t->dim, t->degree, t->args.n_fine, t->args.n_coarse, t->n_fine_rows, t->n_coarse_rows, t->parent.data(),
                          t->fine_off.data(), t->coarse_off.data()};
  PdhGalerkinPlan plan;
  PDH_TRY(pdh_plan_galerkin(fine->err, T, &Lf, &Lc, plan));
  if (fine->prob.dev.n != coarse->prob.dev.n || fine->prob.dev.n1d != t->n1d || fine->prob.dev.dim != t->dim ||
      coarse->prob.dev.n1d != t->n1d || coarse->prob.dev.dim != t->dim)
    return fail(fine, PDH_EINVAL, "the element of the transfer and those of the two resident problems differ");
  PdhGalerkinArgs &A = G.args;
  A = PdhGalerkinArgs{};
  A.n_blocks = (int32_t)plan.blk_slot.size();
  std::vector<double> tab(t->h_tab.size());
  pdh_galerkin_tables(t->n1d, (size_t)t->args.n_fine * t->dim, t->h_tab.data(), tab.data());
  int rc = upload_in(fine, G.allocs, tab.data(), tab.size(), &A.tab, "Galerkin tables");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.ptr.data(), plan.ptr.size(), &A.plan_ptr, "Galerkin plan");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.slot.data(), plan.slot.size(), &A.plan_slot, "Galerkin plan: slots");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.pos.data(), plan.pos.size(), &A.plan_pos, "Galerkin plan: positions");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.col.data(), plan.col.size(), &A.plan_col, "Galerkin plan: column polytopes");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.blk_slot.data(), plan.blk_slot.size(), &A.blk_slot, "Galerkin plan: coarse slots");
  if (rc == PDH_OK)
    rc = upload_in(fine, G.allocs, plan.blk_pos.data(), plan.blk_pos.size(), &A.blk_pos, "Galerkin plan: coarse positions");
  if (rc != PDH_OK)
    {
      G.drop();
      return rc;
    }
  G.coarse = coarse;
  G.fine_epoch = fine->problem_epoch;
  G.coarse_epoch = coarse->problem_epoch;
  return PDH_OK;
}

extern "C" int pdh_galerkin_device(pdh_transfer *t, pdh_ctx *coarse)
{
  if (!t)
    return fail(nullptr, PDH_EINVAL, "transfer is NULL");
  pdh_ctx *fine = t->ctx;
  if (!coarse)
    return fail(fine, PDH_EINVAL, "pdh_galerkin_device: the coarse context is NULL");
  if (coarse == fine)
    return fail(fine, PDH_EINVAL, "pdh_galerkin_device: the coarse context is the transfer's own");
  if (t->kind != pdh_transfer::H_NESTED)
    return fail(fine, PDH_EUNSUPPORTED, "pdh_galerkin_device: a p-transfer has no Galerkin product here; coarse degrees are re-assembled on their own "
                                        "description");
  if (!fine->prob.resident)
    return fail(fine, PDH_ESTATE, "pdh_galerkin_device called before pdh_set_problem on the fine context");
  if (!fine->prob.has_values)
    return fail(fine, PDH_ESTATE, "pdh_galerkin_device: the values of the fine context were never assembled");
  if (!coarse->prob.resident)
    return fail(fine, PDH_ESTATE, "pdh_galerkin_device called before pdh_set_problem on the coarse context");
  PDH_HIP(fine, hipSetDevice(fine->device));
  PDH_TRY(galerkin_plan(t, coarse));
  // whatever reads or writes the coarse values on the coarse context's stream, and the fine values on the fine one's, is over first
  PDH_HIP(fine, hipStreamSynchronize(coarse->stream));
  PdhGalerkinArgs A = t->gal.args;
  const pdh_ctx::Problem &pf = fine->prob, &pc = coarse->prob;
  A.fine_values = pf.dev.values;
  A.coarse_values = pc.dev.values;
  A.f_row_base = pf.dev.row_base, A.f_row_len = pf.dev.row_len, A.f_diag_L = pf.dev.diag_L;
  A.c_row_base = pc.dev.row_base, A.c_row_len = pc.dev.row_len, A.c_diag_L = pc.dev.diag_L;
  A.f_diag_first = pf.dev.diag_first, A.c_diag_first = pc.dev.diag_first;
  ++coarse->values_gen;
  PDH_HIP(fine, pdh_launch_galerkin(t->dim, t->n1d, &A, fine->stream));
  PDH_HIP(fine, hipStreamSynchronize(fine->stream));
  coarse->prob.has_values = true;
  coarse->prob.galerkin_values = true; // (not the SIP assembly of the coarse description: the smoother goes back to the stored operator)
  coarse->prob.sol.matrix_free = false;
  return PDH_OK;
}
