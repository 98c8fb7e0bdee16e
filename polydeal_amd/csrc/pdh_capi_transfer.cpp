// pdh_capi_transfer.cpp — device driver of the C ABI, level transfers (kernels: pdh_transfer.hip; planner: pdh_transfer_plan.cpp).  A
// transfer owns its tables on the device of the context it was created on and launches on that context's stream; it needs no resident
// problem there.
#include "pdh_ctx.h"
#include "pdh_launch.h"
#include "pdh_transfer.h"

struct pdh_transfer
{
  pdh_ctx *ctx = nullptr;
  int dim = 0, n1d = 0;
  int64_t n_fine_rows = 0, n_coarse_rows = 0;
  PdhTransferArgs args{};
  std::vector<void *> allocs;                              // every hipMalloc of the set-up; args points into these
  DevBuf in{DevBuf::slack}, out{DevBuf::slack};            // staging copies of pdh_prolongate / pdh_restrict
  ~pdh_transfer()
  {
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
  PdhTransferArgs &A = t->args;
  A.n_fine = d->n_fine;
  A.n_coarse = d->n_coarse;
  int rc = upload_in(ctx, t->allocs, plan.tab.data(), plan.tab.size(), &A.tab, "transfer tables");
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
  PDH_HIP(t->ctx, pdh_launch_prolongate(t->dim, t->n1d, add, &t->args, d_coarse, d_fine, t->ctx->stream));
  return PDH_OK;
}

static int restrict_device(pdh_transfer *t, const double *d_fine, double *d_coarse, int add)
{
  PDH_TRY(transfer_checks(t, d_coarse, d_fine));
  PDH_HIP(t->ctx, hipSetDevice(t->ctx->device));
  PDH_HIP(t->ctx, pdh_launch_restrict(t->dim, t->n1d, add, &t->args, d_fine, d_coarse, t->ctx->stream));
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
