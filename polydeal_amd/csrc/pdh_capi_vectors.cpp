// pdh_capi_vectors.cpp — device driver of the C ABI, the vectors of a resident problem: right-hand side, evaluation at points, the
// fused error sums, and basis values on boxes.  The host-pointer variants stage their arrays in the context's buffers (pdh_ctx.h:
// stage_in) and call the *_device variant.
#include "pdh_basis.h"
#include "pdh_ctx.h"
#include "pdh_launch.h"

#include <cstring>

// ---- right-hand side -------------------------------------------------------------------------------------------------
// packed boundary point -> the caller's face point (-1: interior), for the Nitsche datum; once per problem
static int ensure_ap_src(pdh_ctx *ctx)
{
  if (ctx->prob.d_ap_src)
    return PDH_OK;
  std::vector<int64_t> ap_src((size_t)std::max<int64_t>(ctx->prob.n_ap, 1), -1);
  // Cartesian description: the packed points are the generated ones (pdh_cartgen.hip: lower tangential axis fastest); the caller
  // samples g_bdry at the points of the equivalent points description, QProjector's order (y, z), (z, x), (x, y) - on the faces of
  // axis 1 the two tangential indices are swapped
  const int64_t nqf = ctx->prob.cart_nqf, m2 = nqf * nqf;
  auto caller = [&](int64_t q) {
    if (!nqf || (ctx->prob.cart_fq_face[(size_t)(q / m2)] >> 1) != 1)
      return q;
    const int64_t l = q % m2;
    return q - l + (l / nqf) + nqf * (l % nqf);
  };
  host_parallel_for(ctx->prob.face_runs.size(), [&](size_t r) {
    const auto &fr = ctx->prob.face_runs[r];
    if (fr.boundary)
      for (int32_t t = 0; t < fr.count; ++t)
        ap_src[fr.ap_begin + t] = caller(fr.fq_begin + t);
  });
  // the boundary points of a slot are one contiguous run (all boundary sub-faces form ONE polytopal face, reference
  // source/agglomeration_handler.cc:1575-1613): the kernel visits only that range
  std::vector<int64_t> bd((size_t)std::max(ctx->prob.n_owned, 1) * 2, 0);
  for (const auto &fr : ctx->prob.face_runs)
    if (fr.boundary && fr.slot >= 0 && fr.slot < ctx->prob.n_owned)
      {
        int64_t &b = bd[(size_t)fr.slot * 2], &e = bd[(size_t)fr.slot * 2 + 1];
        if (e == b)
          b = fr.ap_begin, e = fr.ap_begin + fr.count;
        else
          b = std::min(b, fr.ap_begin), e = std::max(e, fr.ap_begin + fr.count); // (several runs: their hull; interior points in between carry no datum)
      }
  PDH_TRY(upload(ctx, bd, &ctx->prob.d_bd_rng, "boundary ranges of the right-hand side"));
  return upload(ctx, ap_src, &ctx->prob.d_ap_src, "caller face points of the right-hand side");
}

extern "C" int pdh_assemble_rhs_device(pdh_ctx *ctx, const double *d_f_vol, const double *d_g_bdry, double *d_rhs)
{
  PDH_TRY(need_problem(ctx, "pdh_assemble_rhs"));
  if (!d_rhs)
    return fail(ctx, PDH_EINVAL, "rhs is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int rc_map = ensure_ap_src(ctx);
  if (rc_map != PDH_OK)
    return rc_map;
  PDH_HIP(ctx, pdh_launch_rhs(ctx->prob.dev.dim, ctx->prob.dev.n1d, &ctx->prob.dev, ctx->prob.n_owned, d_f_vol, d_g_bdry, d_rhs, ctx->prob.d_vq_src,
                              ctx->prob.d_ap_src, ctx->prob.d_bd_rng, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_assemble_rhs(pdh_ctx *ctx, const double *f_vol, const double *g_bdry, double *rhs)
{
  PDH_TRY(need_problem(ctx, "pdh_assemble_rhs"));
  if (!rhs)
    return fail(ctx, PDH_EINVAL, "rhs is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  // the caller's samples go up as they are (caller order; the kernel indexes them through the maps made at set_problem)
  const char *who = "pdh_assemble_rhs";
  double *d_f = nullptr, *d_g = nullptr, *d_rhs = nullptr;
  PDH_TRY(stage(ctx, who, ctx->io.ptr, (size_t)ctx->prob.n_rows_owned, &d_rhs));
  if (f_vol)
    PDH_TRY(stage_in(ctx, who, ctx->io.in0, f_vol, (size_t)ctx->prob.n_vq_caller, &d_f));
  if (g_bdry)
    PDH_TRY(stage_in(ctx, who, ctx->io.in1, g_bdry, (size_t)ctx->prob.n_fq_caller, &d_g));
  const int rc = pdh_assemble_rhs_device(ctx, d_f, d_g, d_rhs);
  if (rc != PDH_OK)
    return rc;
  PDH_HIP(ctx, hipMemcpyAsync(rhs, d_rhs, ctx->prob.n_rows_owned * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
// the caller's pt_ptr [n + 1]: starts at 0, does not decrease
static int check_pt_ptr(pdh_ctx *ctx, const int64_t *pt_ptr, int n)
{
  if (pt_ptr[0] != 0)
    return fail(ctx, PDH_EINVAL, "pt_ptr[0] must be 0");
  for (int a = 0; a < n; ++a)
    if (pt_ptr[a + 1] < pt_ptr[a])
      return fail(ctx, PDH_EINVAL, "pt_ptr must be non-decreasing");
  return PDH_OK;
}

extern "C" int pdh_evaluate_device(pdh_ctx *ctx, const double *d_solution, const int64_t *d_pt_ptr, const double *d_pts,
                                   int64_t n_points, double *d_u, double *d_grad)
{
  PDH_TRY(need_problem(ctx, "pdh_evaluate"));
  if (!d_solution || !d_pt_ptr || !d_pts || !d_u || n_points < 0)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts and u are required");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, pdh_launch_eval(ctx->prob.dev.dim, ctx->prob.dev.n1d, d_grad ? 1 : 0, &ctx->prob.dev, ctx->prob.n_owned, d_solution, d_pt_ptr, d_pts,
                               n_points, d_u, d_grad, 1, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_evaluate(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, double *u,
                            double *grad)
{
  PDH_TRY(need_problem(ctx, "pdh_evaluate"));
  if (!solution || !pt_ptr || !pts || !u)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts and u are required");
  const int nA = ctx->prob.n_agg_total, dim = ctx->prob.dev.dim;
  PDH_TRY(check_pt_ptr(ctx, pt_ptr, nA));
  const int64_t N = pt_ptr[nA];
  if (N == 0)
    return PDH_OK;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const char *who = "pdh_evaluate";
  double *d_sol = nullptr, *d_pts = nullptr, *d_u = nullptr, *d_g = nullptr;
  int64_t *d_ptr = nullptr;
  PDH_TRY(stage_in(ctx, who, ctx->io.in0, solution, (size_t)ctx->prob.n_rows_owned, &d_sol));
  PDH_TRY(stage_in(ctx, who, ctx->io.in1, pts, (size_t)N * dim, &d_pts));
  PDH_TRY(stage_in(ctx, who, ctx->io.ptr, pt_ptr, (size_t)nA + 1, &d_ptr));
  PDH_TRY(stage(ctx, who, ctx->io.out, (size_t)N, &d_u));
  if (grad)
    PDH_TRY(stage(ctx, who, ctx->io.grad, (size_t)N * dim, &d_g));
  const int rc = pdh_evaluate_device(ctx, d_sol, d_ptr, d_pts, N, d_u, d_g);
  if (rc != PDH_OK)
    return rc;
  // only the points of polytopes owned here are produced; the others are left untouched in the caller's arrays
  std::vector<double> hu((size_t)N), hg(grad ? (size_t)N * dim : 0);
  PDH_HIP(ctx, hipMemcpyAsync(hu.data(), d_u, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (grad)
    PDH_HIP(ctx, hipMemcpyAsync(hg.data(), d_g, (size_t)N * dim * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  std::vector<int32_t> own((size_t)ctx->prob.n_owned);
  PDH_HIP(ctx, hipMemcpyAsync(own.data(), ctx->prob.dev.own_agg, own.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int a : own)
    for (int64_t q = pt_ptr[a]; q < pt_ptr[a + 1]; ++q)
      {
        u[q] = hu[q];
        if (grad)
          for (int c = 0; c < dim; ++c)
            grad[(size_t)c * N + q] = hg[(size_t)c * N + q];
      }
  return PDH_OK;
}

// ---- PolyUtils::compute_global_error fused on the device (reference include/poly_utils.h:1647-1750) -----------------------
extern "C" int pdh_global_error_device(pdh_ctx *ctx, const double *d_solution, const int64_t *d_pt_ptr, const double *d_pts,
                                       int64_t n_points, const double *d_w, const double *d_exact_u, const double *d_exact_grad,
                                       double *sums)
{
  PDH_TRY(need_problem(ctx, "pdh_global_error"));
  if (!d_solution || !d_pt_ptr || !d_pts || !d_w || !d_exact_u || !d_exact_grad || !sums || n_points < 0)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts, w, exact_u, exact_grad and sums are required");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  sums[0] = sums[1] = 0.0;
  if (ctx->prob.n_owned == 0)
    return PDH_OK;
  double *d_err = nullptr;
  PDH_TRY(stage(ctx, "pdh_global_error", ctx->io.err, (size_t)ctx->prob.n_owned * 2, &d_err));
  PDH_HIP(ctx, pdh_launch_eval_err(ctx->prob.dev.dim, ctx->prob.dev.n1d, &ctx->prob.dev, ctx->prob.n_owned, d_solution, d_pt_ptr, d_pts, n_points, d_w,
                                   d_exact_u, d_exact_grad, d_err, ctx->stream));
  // 16 bytes per polytope come back; they are added in slot order (the result does not depend on the launch)
  std::vector<double> h((size_t)ctx->prob.n_owned * 2);
  PDH_HIP(ctx, hipMemcpyAsync(h.data(), d_err, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int sl = 0; sl < ctx->prob.n_owned; ++sl)
    {
      sums[0] += h[2 * (size_t)sl];
      sums[1] += h[2 * (size_t)sl + 1];
    }
  return PDH_OK;
}

extern "C" int pdh_global_error(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, const double *w,
                                const double *exact_u, const double *exact_grad, double *sums)
{
  PDH_TRY(need_problem(ctx, "pdh_global_error"));
  if (!solution || !pt_ptr || !pts || !w || !exact_u || !exact_grad || !sums)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts, w, exact_u, exact_grad and sums are required");
  const int nA = ctx->prob.n_agg_total, dim = ctx->prob.dev.dim;
  PDH_TRY(check_pt_ptr(ctx, pt_ptr, nA));
  const int64_t N = pt_ptr[nA];
  sums[0] = sums[1] = 0.0;
  if (N == 0)
    return PDH_OK;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const char *who = "pdh_global_error";
  double *d_sol = nullptr, *d_pts = nullptr, *d_eu = nullptr, *d_eg = nullptr;
  int64_t *d_ptr = nullptr;
  PDH_TRY(stage_in(ctx, who, ctx->io.in0, solution, (size_t)ctx->prob.n_rows_owned, &d_sol));
  PDH_TRY(stage_in(ctx, who, ctx->io.in1, pts, (size_t)N * dim, &d_pts));
  PDH_TRY(stage_in(ctx, who, ctx->io.ptr, pt_ptr, (size_t)nA + 1, &d_ptr));
  PDH_TRY(stage_in(ctx, who, ctx->io.out, exact_u, (size_t)N, &d_eu, (size_t)N * 2)); // exact_u | w
  PDH_HIP(ctx, hipMemcpyAsync(d_eu + N, w, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_TRY(stage_in(ctx, who, ctx->io.grad, exact_grad, (size_t)N * dim, &d_eg));
  return pdh_global_error_device(ctx, d_sol, d_ptr, d_pts, N, d_eu + N, d_eu, d_eg, sums);
}

// ---- basis values on boxes (injection matrices) -----------------------------------------------------------------------
extern "C" int pdh_shape_values_device(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *d_bbox,
                                       const int64_t *d_pt_ptr, const double *d_pts, int64_t n_points, double *d_values)
{
  PDH_TRY(need_ctx(ctx));
  if (dim < 2 || dim > 3 || degree < 0 || (basis != PDH_BASIS_DGQ && basis != PDH_BASIS_AGGLODGP))
    return fail(ctx, PDH_EINVAL, "dim must be 2 or 3, degree >= 0, basis DGQ or AGGLODGP");
  const int n = pdh::n_dofs_per_cell(dim, degree, basis);
  const int n1d = degree + 1;
  if (n1d > 8 || (dim == 2 && n > 64))
    return fail(ctx, PDH_EUNSUPPORTED, "no kernel instantiated for this (dim, basis, degree)");
  if (n_boxes <= 0 || n_points <= 0)
    return PDH_OK;
  if (!d_bbox || !d_pt_ptr || !d_pts || !d_values)
    return fail(ctx, PDH_EINVAL, "bbox, pt_ptr, pts and values are required");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int key = (dim * 16 + degree) * 2 + basis;
  if (ctx->shape_key != key)
    {
      const auto mi = pdh::multi_indices(dim, degree, basis);
      std::vector<int32_t> midx(512, (int32_t)0xffffffffu); // (n <= 8^3)
      for (int i = 0; i < n; ++i)
        midx[i] = (int32_t)mi[i];
      int32_t *d_midx = ctx->shape_midx.get<int32_t>(512);
      if (!d_midx)
        return fail(ctx, PDH_EDEVICE, "pdh_shape_values: out of device memory");
      PDH_HIP(ctx, hipMemcpy(d_midx, midx.data(), 512 * sizeof(int32_t), hipMemcpyHostToDevice));
      ctx->shape_key = key;
    }
  PdhDev D;
  std::memset(&D, 0, sizeof(D));
  D.dim = dim;
  D.n = n;
  D.n1d = n1d;
  const pdh::Basis1D b1 = (basis == PDH_BASIS_DGQ) ? pdh::lagrange_basis(degree) : pdh::legendre_basis(degree);
  for (int k = 0; k < n1d; ++k)
    for (int m = 0; m < n1d; ++m)
      D.tab.coef[k][m] = (double)b1.coef[k][m];
  D.bbox = d_bbox;
  D.midx = ctx->shape_midx.ptr<int32_t>();
  PDH_HIP(ctx, pdh_launch_shape(dim, n1d, &D, n_boxes, d_pt_ptr, d_pts, n_points, d_values, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_shape_values(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *bbox,
                                const int64_t *pt_ptr, const double *pts, double *values)
{
  PDH_TRY(need_ctx(ctx));
  if (dim < 2 || dim > 3 || degree < 0 || (basis != PDH_BASIS_DGQ && basis != PDH_BASIS_AGGLODGP))
    return fail(ctx, PDH_EINVAL, "dim must be 2 or 3, degree >= 0, basis DGQ or AGGLODGP");
  if (n_boxes < 0 || (n_boxes > 0 && (!bbox || !pt_ptr || !pts || !values)))
    return fail(ctx, PDH_EINVAL, "bbox, pt_ptr, pts and values are required");
  const int n = pdh::n_dofs_per_cell(dim, degree, basis);
  if (degree + 1 > 8 || (dim == 2 && n > 64))
    return fail(ctx, PDH_EUNSUPPORTED, "no kernel instantiated for this (dim, basis, degree)");
  if (n_boxes == 0)
    return PDH_OK;
  for (int b = 0; b < n_boxes; ++b)
    {
      if (pt_ptr[b + 1] < pt_ptr[b])
        return fail(ctx, PDH_EINVAL, "pt_ptr must be non-decreasing");
      for (int c = 0; c < dim; ++c)
        if (!(bbox[(size_t)b * 2 * dim + dim + c] > bbox[(size_t)b * 2 * dim + c]))
          return fail(ctx, PDH_EINVAL, "degenerate bounding box");
    }
  if (pt_ptr[0] != 0)
    return fail(ctx, PDH_EINVAL, "pt_ptr[0] must be 0");
  const int64_t N = pt_ptr[n_boxes];
  if (N == 0)
    return PDH_OK;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const char *who = "pdh_shape_values";
  double *d_bbox = nullptr, *d_pts = nullptr, *d_out = nullptr;
  int64_t *d_ptr = nullptr;
  PDH_TRY(stage_in(ctx, who, ctx->io.in0, bbox, (size_t)n_boxes * 2 * dim, &d_bbox));
  PDH_TRY(stage_in(ctx, who, ctx->io.in1, pts, (size_t)N * dim, &d_pts));
  PDH_TRY(stage_in(ctx, who, ctx->io.ptr, pt_ptr, (size_t)n_boxes + 1, &d_ptr));
  PDH_TRY(stage(ctx, who, ctx->io.out, (size_t)N * n, &d_out));
  const int rc = pdh_shape_values_device(ctx, dim, degree, basis, n_boxes, d_bbox, d_ptr, d_pts, N, d_out);
  if (rc != PDH_OK)
    return rc;
  PDH_HIP(ctx, hipMemcpyAsync(values, d_out, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}
