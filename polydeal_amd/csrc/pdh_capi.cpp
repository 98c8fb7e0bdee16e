// pdh_capi.cpp — the device driver of the C ABI declared in include/polydeal_hip.h, first of three units: contexts (create / destroy,
// version), set-up of the resident problem (upload_*, record_problem, set_problem_impl), the assembly (pdh_assemble_device with its
// streams and graph), exchange, stream, profiling, stats and checksum.  pdh_capi_vectors.cpp holds the right-hand side, evaluation,
// error sums and shape values, pdh_capi_solve.cpp y = A x, the preconditioners, CG and Chebyshev; pdh_ctx.h (internal) the context,
// its device buffers and the guards all three share.
//
// Host work of SETUP (what the reference does once per mesh in AgglomerationHandler::distribute_agglomerated_dofs /
// setup_connectivity_of_agglomeration / create_agglomeration_sparsity_pattern, source/agglomeration_handler.cc:326-379, 495-527,
// 910-1022) - validation, repacking of the face tables per owning polytope, block positions inside CSR rows, the choice of the row
// kernel and its tables - is the planner's (pdh_plan.h, host-only); pdh_set_problem uploads what it built.
// The assembly itself (pdh_assemble_device) only launches the HIP kernels.
#include "pdh_basis.h"
#include "pdh_combos.h"
#include "pdh_ctx.h"
#include "pdh_kernels.h" // pdh::Sched, for the MFMA work counts (the only driver unit that sees a kernel header)
#include "pdh_moment_tables.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static pdh_resolve_fn g_resolve[PDH_N_GROUPS] = {pdh_resolve_g0, pdh_resolve_g1, pdh_resolve_g2, pdh_resolve_g3,
                                                 pdh_resolve_g4, pdh_resolve_g5, pdh_resolve_g6, pdh_resolve_g7};

// number of MFMA instructions one 4-point step of a product issues, from the kernels' own schedule
template <int NT, int LB>
static constexpr int sched_instr(bool sym)
{
  int c = 0;
  for (int a = 0; a < NT; ++a)
    for (int b = 0; b < NT; ++b)
      for (int r = 0; r < 4; ++r)
        if ((sym ? pdh::Sched<NT, LB>::sym_mask(a, b, r) : pdh::Sched<NT, LB>::full_mask(a, b, r)) != 0u)
          ++c;
  return c;
}
static int sched_instr_rt(int nt, int lb, bool sym)
{
  switch (nt * 4 + (lb - 1))
    {
#define PDH_C(NT, LB)                                                                              \
  case NT * 4 + (LB - 1):                                                                          \
    return sched_instr<NT, LB>(sym);
      PDH_C(1, 1) PDH_C(1, 2) PDH_C(1, 3) PDH_C(1, 4) PDH_C(2, 1) PDH_C(2, 2) PDH_C(2, 3) PDH_C(2, 4)
      PDH_C(3, 1) PDH_C(3, 2) PDH_C(3, 3) PDH_C(3, 4) PDH_C(4, 1) PDH_C(4, 2) PDH_C(4, 3) PDH_C(4, 4)
#undef PDH_C
    }
  return 0;
}

// Free what the problem owns, then start from a fresh Problem: no pointer or count of the dropped one survives (its solver
// buffers go with the assignment).
static void free_problem(pdh_ctx *ctx)
{
  for (void *p : ctx->prob.allocs)
    (void)hipFree(p);
  ctx->prob.drop_graph();
  ctx->prob = pdh_ctx::Problem{};
}

#ifndef PDH_SRC_HASH
#define PDH_SRC_HASH "unhashed"
#endif
// "polydeal_hip <version>+<hash of the library's sources and build flags> gfx950" (Makefile: SRC_HASH)
extern "C" const char *pdh_version(void) { return "polydeal_hip 0.4+" PDH_SRC_HASH " gfx950"; }

extern "C" const char *pdh_last_error(const pdh_ctx *ctx) { return ctx ? ctx->err.c_str() : pdh_noctx_error().c_str(); }

extern "C" int pdh_create(pdh_ctx **out, int device_id)
{
  if (!out)
    return fail(nullptr, PDH_EINVAL, "pdh_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, PDH_EDEVICE,
                std::string("pdh_create: no HIP device available (") + hipGetErrorString(e) +
                  "); this library has no CPU fallback");
  if (device_id < 0 || device_id >= ndev)
    return fail(nullptr, PDH_EINVAL, "pdh_create: device_id out of range");
  PDH_HIP(nullptr, hipSetDevice(device_id));
  pdh_ctx *ctx = new pdh_ctx;
  ctx->device = device_id;
  if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess)
    {
      delete ctx;
      return fail(nullptr, PDH_EDEVICE, "pdh_create: second stream / events");
    }
  if (hipStreamCreate(&ctx->own_stream) != hipSuccess)
    {
      delete ctx;
      return fail(nullptr, PDH_EDEVICE, "pdh_create: hipStreamCreate failed");
    }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return PDH_OK;
}

extern "C" void pdh_destroy(pdh_ctx *ctx)
{
  if (!ctx)
    return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  pdh_mg_detach(ctx); // (a pdh_mg is destroyed before its contexts; one still attached here must not be reached through this one)
  free_problem(ctx);
  for (DevBuf *b : {&ctx->io.in0, &ctx->io.in1, &ctx->io.ptr, &ctx->io.out, &ctx->io.grad, &ctx->io.err, &ctx->shape_midx, &ctx->checksum})
    b->release(); // (before the streams go, as ever)
  if (ctx->pinned)
    (void)hipHostFree(ctx->pinned);
  for (auto &ev : ctx->events)
    if (ev)
      (void)hipEventDestroy(ev);
  (void)hipStreamDestroy(ctx->own_stream);
  if (ctx->stream2)
    (void)hipStreamDestroy(ctx->stream2);
  if (ctx->ev_fork)
    (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join)
    (void)hipEventDestroy(ctx->ev_join);
  delete ctx;
}

// Term kernels of the resident problem: cells before / after merging, sub-faces before / after (pdh_terms_tables.h); zeros if another
// kernel serves the problem.
extern "C" int pdh_terms_merge_stats(pdh_ctx *ctx, int64_t *out4)
{
  if (!ctx || !out4)
    return fail(ctx, PDH_EINVAL, "ctx and out4 are required");
  if (!ctx->prob.resident)
    return fail(ctx, PDH_ESTATE, "pdh_terms_merge_stats called before pdh_set_problem");
  for (int i = 0; i < 4; ++i)
    out4[i] = ctx->prob.row_kernel == RowKernel::terms ? ctx->prob.terms_merge[i] : 0;
  return PDH_OK;
}

// Own-side face points of every slot (PdhDev::ap_*), built in HBM: the caller's face arrays go up as they are (each face
// once), k_pack_faces writes one SoA run per (polytope, face) with the sign of the normal, the weights and sigma resolved
// (tables Packed::pk_*).  The staging copies are released before this returns.
// Gauss-Legendre rule of n points on [0, 1] as the generators take it (pdh_cartgen.hip): zero-padded to PDH_MAX_N1D
struct GaussRule01
{
  double x[PDH_MAX_N1D] = {0}, w[PDH_MAX_N1D] = {0};
  explicit GaussRule01(int n)
  {
    std::vector<long double> gx, gw;
    pdh::gauss_legendre01(n, gx, gw);
    for (int i = 0; i < n; ++i)
      x[i] = (double)gx[i], w[i] = (double)gw[i];
  }
};

static int pack_faces_on_device(pdh_ctx *ctx, const pdh_problem *p, const Packed &K, PdhDev &D)
{
  const int dim = p->dim;
  const int64_t nap = K.n_ap, nqf = K.nqf_src, nruns = (int64_t)K.pk_at.size();
  double *out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t out_n[5] = {(size_t)dim * nap, (size_t)dim * nap, (size_t)nap, (size_t)nap, (size_t)nap};
  for (int k = 0; k < 5; ++k)
    PDH_TRY(device_buffer(ctx, out_n[k], &out[k], "packed face points"));
  D.ap_x = out[0], D.ap_n = out[1], D.ap_wself = out[2], D.ap_wcross = out[3], D.ap_sig = out[4];
  if (nruns == 0 || nap == 0)
    return PDH_OK;
  Staging st(ctx);
  const double *d_x = nullptr, *d_n = nullptr, *d_w = nullptr, *d_wo = nullptr;
  if (K.cart)
    { // the caller-order face arrays are generated here from (cell, local face) of every sub-face (pdh_cartgen.hip); JxW of side 1
      // equals JxW of side 0 on a conforming Cartesian grid (d_wo stays NULL)
      const pdh_cartesian_points *cp = K.cart;
      const int64_t nsf = nqf / ((int64_t)cp->nqf * cp->nqf);
      const double *d_box = nullptr;
      const int32_t *d_cell = nullptr, *d_face = nullptr;
      double *x = nullptr, *n = nullptr, *w = nullptr;
      PDH_TRY(st.upload(cp->cell_box, (size_t)cp->n_cells * 6, &d_box, "cell boxes"));
      PDH_TRY(st.upload(cp->fq_cell, (size_t)nsf, &d_cell, "cells of the sub-faces"));
      PDH_TRY(st.upload(cp->fq_face, (size_t)nsf, &d_face, "local faces of the sub-faces"));
      PDH_TRY(st.alloc((size_t)dim * nqf, &x, "face points"));
      PDH_TRY(st.alloc((size_t)dim * nqf, &n, "face normals"));
      PDH_TRY(st.alloc((size_t)nqf, &w, "face weights"));
      const GaussRule01 g(cp->nqf);
      PDH_HIP(ctx, pdh_launch_gen_faces(cp->nqf, g.x, g.w, d_box, d_cell, d_face, nqf, x, n, w, ctx->stream));
      d_x = x, d_n = n, d_w = w;
    }
  else
    {
      PDH_TRY(st.upload(p->fq_x, (size_t)dim * nqf, &d_x, "face points"));
      PDH_TRY(st.upload(p->fq_n, (size_t)dim * nqf, &d_n, "face normals"));
      PDH_TRY(st.upload(p->fq_w, (size_t)nqf, &d_w, "face weights"));
      if (p->fq_w_out)
        PDH_TRY(st.upload(p->fq_w_out, (size_t)nqf, &d_wo, "face weights of side 1"));
    }
  const int64_t *d_at = nullptr, *d_fq = nullptr;
  const int32_t *d_cnt = nullptr, *d_fl = nullptr;
  const double *d_sg = nullptr;
  PDH_TRY(st.upload(K.pk_at.data(), K.pk_at.size(), &d_at, "face runs: packed position"));
  PDH_TRY(st.upload(K.pk_fq.data(), K.pk_fq.size(), &d_fq, "face runs: caller position"));
  PDH_TRY(st.upload(K.pk_cnt.data(), K.pk_cnt.size(), &d_cnt, "face runs: counts"));
  PDH_TRY(st.upload(K.pk_flags.data(), K.pk_flags.size(), &d_fl, "face runs: flags"));
  PDH_TRY(st.upload(K.pk_sig.data(), K.pk_sig.size(), &d_sg, "face runs: sigma"));
  PDH_HIP(ctx, pdh_launch_pack_faces(dim, nqf, d_x, d_n, d_w, d_wo, nruns, d_at, d_fq, d_cnt, d_fl, d_sg, nap, out[0], out[1], out[2],
                                     out[3], out[4], ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// pdh_set_problem_cartesian: the volume points of the owned slots, generated slot by slot from the cells' boxes (pdh_cartgen.hip)
static int generate_volume_points(pdh_ctx *ctx, const Packed &K, PdhDev &D)
{
  const pdh_cartesian_points *cart = K.cart;
  const int64_t m3 = (int64_t)cart->nq * cart->nq * cart->nq, ngroups = K.n_vq / m3;
  std::vector<int32_t> gcell((size_t)std::max<int64_t>(ngroups, 1));
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      const int64_t g0 = K.vq_ptr[sl] / m3, g1 = K.vq_ptr[sl + 1] / m3, src = K.vq_src[sl] / m3;
      for (int64_t g = g0; g < g1; ++g)
        gcell[(size_t)g] = cart->vq_cell[src + (g - g0)];
    }
  double *x = nullptr, *w = nullptr;
  PDH_TRY(device_buffer(ctx, (size_t)3 * K.n_vq, &x, "volume points"));
  PDH_TRY(device_buffer(ctx, (size_t)K.n_vq, &w, "volume weights"));
  Staging st(ctx);
  const double *d_box = nullptr;
  const int32_t *d_gcell = nullptr;
  PDH_TRY(st.upload(cart->cell_box, (size_t)cart->n_cells * 6, &d_box, "cell boxes"));
  PDH_TRY(st.upload(gcell.data(), gcell.size(), &d_gcell, "cells of the volume rules"));
  const GaussRule01 g(cart->nq);
  PDH_HIP(ctx, pdh_launch_gen_volume(cart->nq, g.x, g.w, d_box, d_gcell, K.n_vq, x, K.n_vq, w, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  D.vq_x = x, D.vq_w = w;
  return PDH_OK;
}

// Device state every kernel reads: boxes, points, faces, the maps of the blocks, the values (with the send region of the
// ghost-block exchange behind them), the moment tables (3-D, degree 1 .. 3).
static int upload_problem(pdh_ctx *ctx, const pdh_problem *p, const Packed &K)
{
  PdhDev &D = ctx->prob.dev;
  std::memset(&D, 0, sizeof(D));
  D.dim = p->dim;
  D.n = K.n;
  D.n1d = K.n1d;
  D.diag_first = p->diag_first ? 1 : 0;
  D.reaction_c = p->reaction_c;
  D.tab = K.tab;
  D.vq_stride = K.vq_stride_h;
  D.ap_stride = K.n_ap;
  const std::vector<double> bbox(p->bbox, p->bbox + (size_t)p->n_agg * 2 * p->dim);
  PDH_UP(bbox, D.bbox);
  PDH_UP(K.midx, D.midx);
  PDH_UP(K.vq_ptr, D.vq_ptr);
  if (K.cart)
    PDH_TRY(generate_volume_points(ctx, K, D));
  else
    {
      PDH_TRY(upload(ctx, K.vqx_h, (size_t)p->dim * K.vq_stride_h, &D.vq_x, "D.vq_x"));
      PDH_TRY(upload(ctx, K.vqw_h, (size_t)K.n_vq, &D.vq_w, "D.vq_w"));
    }
  PDH_UP(K.ap_ptr, D.ap_ptr);
  PDH_TRY(pack_faces_on_device(ctx, p, K, D));
  PDH_UP(K.own_agg, D.own_agg);
  PDH_UP(K.own_row, D.own_row);
  PDH_UP(K.row_base, D.row_base);
  PDH_UP(K.row_len, D.row_len);
  PDH_UP(K.diag_L, D.diag_L);
  PDH_UP(K.it_own, D.it_own);
  PDH_UP(K.it_nbr, D.it_nbr);
  PDH_UP(K.it_pbeg, D.it_pbeg);
  PDH_UP(K.it_pcnt, D.it_pcnt);
  PDH_UP(K.it_pos, D.it_pos);
  PDH_UP(K.it_nbr_slot, D.it_nbr_slot);
  PDH_UP(K.it_pos_t, D.it_pos_t);
  PDH_TRY(upload(ctx, K.blk_ptr, &ctx->prob.d_blk_ptr, "ctx->d_blk_ptr"));
  PDH_TRY(upload(ctx, K.blk_dof, &ctx->prob.d_blk_dof, "ctx->d_blk_dof"));
  if (K.ghost)
    {
      PDH_TRY(upload(ctx, K.r21_src, &ctx->prob.d_r21_src, "ctx->d_r21_src"));
      PDH_TRY(upload(ctx, K.r21_dst, &ctx->prob.d_r21_dst, "ctx->d_r21_dst"));
      PDH_TRY(upload(ctx, K.r21_rlen, &ctx->prob.d_r21_rlen, "ctx->d_r21_rlen"));
      PDH_TRY(upload(ctx, K.r22_ptr, &ctx->prob.d_r22_ptr, "ctx->d_r22_ptr"));
      PDH_TRY(upload(ctx, K.r22_src, &ctx->prob.d_r22_src, "ctx->d_r22_src"));
      PDH_TRY(upload(ctx, K.r22_slot, &ctx->prob.d_r22_slot, "ctx->d_r22_slot"));
    }
  PDH_TRY(device_buffer(ctx, (size_t)(K.n_values + K.n_send), &D.values, "values"));
  // (the per-point map of the packed boundary points to the caller's face points - 8 bytes per packed face point - is needed by
  // the right-hand side only: built and uploaded at its first call, ensure_ap_src)
  PDH_TRY(upload(ctx, K.vq_src, &ctx->prob.d_vq_src, "ctx->d_vq_src"));
  if (p->dim == 3 && K.n1d >= 2 && K.n1d <= 4)
    {
      const std::vector<double> mt = pdh::moment_tables(p->degree, p->basis);
      if ((int)mt.size() != pdhm::moment_table_doubles(K.n1d))
        return fail(ctx, PDH_EDEVICE, "moment tables: the host's and the kernels' sizes differ");
      PDH_TRY(upload(ctx, mt, &ctx->prob.d_mtab, "ctx->d_mtab"));
    }
  return PDH_OK;
}

// Host side of the resident problem: sizes, the caller-order maps of the right-hand side, the kernels' launch shapes and work.
static void record_problem(pdh_ctx *ctx, const pdh_problem *p, const Packed &K)
{
  ctx->prob.ghost = K.ghost;
  ctx->prob.n_send = K.n_send;
  ctx->prob.n_recv = K.n_recv;
  ctx->prob.send_count = K.send_count;
  ctx->prob.recv_count = K.recv_count;
  ctx->prob.n_r21 = (int)K.r21_src.size();
  ctx->prob.n_r22 = (int)K.r22_slot.size();
  ctx->prob.n_values = K.n_values;
  ctx->prob.n_owned = K.n_owned;
  ctx->prob.n_diag_slots = (int)K.own_agg.size();
  ctx->prob.n_items = (int)K.it_own.size();
  ctx->prob.n_vq = K.n_vq;
  ctx->prob.n_ap = K.n_ap;
  ctx->prob.NT = K.NT;
  ctx->prob.tiled = K.tiled;
  ctx->prob.basis = p->basis;
  ctx->prob.n_vq_caller = p->vq_ptr[p->n_agg];
  ctx->prob.n_fq_caller = p->n_faces ? p->fq_ptr[p->n_faces] : 0;
  ctx->prob.cart_fq_face.clear();
  ctx->prob.cart_nqf = 0;
  if (K.cart && K.cart->nqf > 0)
    {
      ctx->prob.cart_nqf = K.cart->nqf;
      ctx->prob.cart_fq_face.assign(K.cart->fq_face, K.cart->fq_face + ctx->prob.n_fq_caller / ((int64_t)K.cart->nqf * K.cart->nqf));
    }
  ctx->prob.face_runs.clear();
  ctx->prob.face_runs.reserve(K.run_ap.size());
  for (size_t r = 0; r < K.run_ap.size(); ++r)
    ctx->prob.face_runs.push_back({K.run_ap[r], K.run_fq[r], K.run_cnt[r], K.run_bdry[r], K.run_slot[r]});
  ctx->prob.n_rows_owned = (int64_t)K.n_owned * K.n;
  ctx->prob.n_rows_total = p->n_rows;
  ctx->prob.max_row_len = K.max_row_len;
  ctx->prob.h_blk_ptr = K.blk_ptr;
  ctx->prob.h_blk_dof = K.blk_dof;
  ctx->prob.h_slot_dof.resize((size_t)K.n_owned);
  for (int s = 0; s < K.n_owned; ++s)
    ctx->prob.h_slot_dof[(size_t)s] = p->dof_offset[K.own_agg[(size_t)s]];
  ctx->prob.n_agg_total = p->n_agg;
  // executed work: k-steps of 4 points per chunk (64 points in k_diag for NT >= 3, else 32; 32 in k_offdiag)
  const int64_t i_sym = sched_instr_rt(K.NT, K.LB, true), i_full = sched_instr_rt(K.NT, K.LB, false);
  const int ch_d = (K.NT >= 3) ? 64 : 32, ch_o = 32;
  auto ksteps = [](int64_t npts, int ch) {
    int64_t s = (npts / ch) * (ch / 4);
    const int64_t rem = npts % ch;
    return s + (rem + 3) / 4;
  };
  int64_t kv = 0, kf = 0, ko = 0;
  for (size_t sl = 0; sl < K.own_agg.size(); ++sl)
    {
      kv += ksteps(K.vq_ptr[sl + 1] - K.vq_ptr[sl], ch_d);
      kf += ksteps(K.ap_ptr[sl + 1] - K.ap_ptr[sl], ch_d);
    }
  for (size_t it = 0; it < K.it_pcnt.size(); ++it)
    ko += ksteps(K.it_pcnt[it], ch_o);
  ctx->prob.mfma_diag = kv * (p->dim + (p->reaction_c != 0.0 ? 1 : 0)) * i_sym + kf * 2 * i_sym;
  ctx->prob.mfma_offdiag = ko * 2 * i_full;
  if (K.tiled)
    { // tiles ti < tj of the own block and all tiles of a coupling block are full 64 x 64 products (64 instructions per k-step), the
      // tiles ti == tj symmetric ones (the schedule of a full n = 64 block)
      const int64_t nt = (K.n + 63) / 64, i64 = sched_instr_rt(4, 4, true);
      ctx->prob.mfma_diag = (kv * (p->dim + (p->reaction_c != 0.0 ? 1 : 0)) + kf * 2) * (64 * (nt * (nt - 1) / 2) + i64 * nt);
      ctx->prob.mfma_offdiag = ko * 2 * 64 * nt * nt;
    }
}

// pdh_rows.h: face tables and per-slot records, the work counter of the persistent waves, the stamps of -DPDHR_STAMP builds and,
// for the MULTI instantiation, a scratch row per resident wave (cus: compute units of the device)
static int upload_rows_state(pdh_ctx *ctx, const Packed &K, const KernelPlan &plan, int cus)
{
  const RowsHost &RH = plan.rows;
  PdhRows &R = ctx->prob.rows;
  PDH_UP(RH.fr_ptr, R.fr_ptr);
  PDH_UP(RH.fr_pbeg, R.fr_pbeg);
  PDH_UP(RH.fr_pcnt, R.fr_pcnt);
  PDH_UP(RH.fr_nbr, R.fr_nbr);
  PDH_UP(RH.fr_axis, R.fr_axis);
  PDH_UP(RH.fr_blk, R.fr_blk);
  PDH_UP(RH.fr_flags, R.fr_flags);
  PDH_UP(RH.fr_coord, R.fr_coord);
  PDH_UP(RH.fr_sigma, R.fr_sigma);
  PDH_UP(RH.fr_nsign, R.fr_nsign);
  PDH_UP(RH.meta, R.meta);
  PDH_TRY(device_buffer(ctx, 16, &R.sched, "row kernel: work counter"));
  PDH_HIP(ctx, hipMemset(R.sched, 0, 16 * sizeof(unsigned int)));
  const size_t n_stamps = (size_t)std::max(K.n_owned, 1) * 16;
  PDH_TRY(device_buffer(ctx, n_stamps, &R.stamps, "row kernel: stamps"));
  PDH_HIP(ctx, hipMemset(R.stamps, 0, n_stamps * sizeof(long long)));
  if (RH.multi)
    {
      // MULTI instantiation: the coupling moments of a polytope's interior entries (8 x 8 doubles each, up to 40 of
      // them) are parked between P2 and P5 in a per-wave row of this buffer instead of LDS (pdh_rows.h) - 8 waves per
      // CU at most (256 VGPRs), a few tens of MB that stay in L2 / the memory-side cache
      const int waves = cus * 8;
      // (with tensor sub-face rules the row holds 16 + 16 factors per interior sub-face instead, pdh_rows.h: FACT)
      const size_t stride = std::max<size_t>((size_t)RH.maxf * 64, (size_t)RH.maxs * 32 + 64);
      PDH_TRY(device_buffer(ctx, (size_t)waves * stride, &R.m2c_scratch, "row kernel: MULTI scratch"));
      R.scratch_waves = waves;
      R.scratch_stride = (int64_t)stride;
    }
  R.tensor_only = plan.tensor_only ? 1 : 0;
  R.multi = RH.multi ? 1 : 0;
  R.maxe = RH.maxe;
  R.maxf = RH.maxf;
  R.vq_tensor_n = plan.vq_n;
  R.fq_tensor_n = RH.fq_tensor_n;
  return PDH_OK;
}

// Term kernels: their tables, the records of 1-D rules the kernels read (gathered on the device from the point arrays), the
// stamps of -DPDHT_STAMP builds, the work counter of pdh_terms_wg.h
static int upload_terms_state(pdh_ctx *ctx, const Packed &K, const KernelPlan &plan)
{
  const TermsHost &TH = plan.terms;
  PdhTerms &T = ctx->prob.terms;
  PDH_UP(TH.meta, T.meta);
  PDH_UP(TH.sf_pt, T.sf_pt);
  PDH_UP(TH.sf_info, T.sf_info);
  PDH_UP(TH.sf_ivl, T.sf_ivl);
  PDH_UP(TH.cell_ivl, T.cell_ivl);
  T.maxruns = TH.maxruns, T.maxsf = TH.maxsf, T.maxsi = TH.maxsi, T.maxcell = TH.maxcell;
  T.vq_tensor_n = plan.vq_n, T.fq_tensor_n = plan.rows.fq_tensor_n;
  T.lds_bytes = TH.lds_bytes;
  T.split = TH.split;
  T.task_pts = TH.task_pts;
  // the 1-D rules the kernels read, gathered on the device from the point arrays (zero-filled: slots behind a rule)
  T.tpm = TH.task_pts > 4 ? 8 : 4;
  T.tstride = pdht::terms_task_doubles(T.maxsf, T.maxcell, T.tpm);
  const size_t n_tdata = (size_t)std::max(K.n_owned, 1) * T.tstride;
  double *tdata = nullptr;
  PDH_TRY(device_buffer(ctx, n_tdata, &tdata, "term kernel: records of 1-D rules"));
  PDH_HIP(ctx, hipMemsetAsync(tdata, 0, n_tdata * sizeof(double), ctx->stream));
  T.tdata = tdata;
  PDH_HIP(ctx, pdh_launch_terms_gather(&ctx->prob.dev, &T, tdata, K.n_owned, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n_stamps = (size_t)std::max(K.n_owned, 1) * 16;
  PDH_TRY(device_buffer(ctx, n_stamps, &T.stamps, "term kernel: stamps"));
  PDH_HIP(ctx, hipMemset(T.stamps, 0, n_stamps * sizeof(long long)));
  PDH_TRY(device_buffer(ctx, 16, &T.sched, "term kernel: work counter"));
  PDH_HIP(ctx, hipMemset(T.sched, 0, 16 * sizeof(unsigned int)));
  ctx->prob.terms_merge[0] = TH.n_cells_in, ctx->prob.terms_merge[1] = TH.n_cells_out;
  ctx->prob.terms_merge[2] = TH.n_sf_in, ctx->prob.terms_merge[3] = TH.n_sf_out;
  return PDH_OK;
}

// Every launch pdh_set_algorithm can ask of the resident problem (pdh_ctx::Problem::direct / moment / row), resolved by the units that
// instantiate the kernels
// (why_row: set where the row kernel the plan chose could not be resolved - the set-up fails with it)
static void resolve_launches(pdh_ctx *ctx, const Packed &K, const PlanSwitches &sw, int cus, const char **why_row)
{
  *why_row = nullptr;
  pdh_ctx::Problem &pr = ctx->prob;
  const PdhDev &D = pr.dev;
  const bool reaction = D.reaction_c != 0.0;
  if (K.tiled)
    pdh_resolve_tiled(D.dim, D.n1d, D.n, reaction, pr.n_diag_slots, pr.n_items, pr.direct);
  else // (pack_problem refused what no group instantiates)
    g_resolve[combo_group(D.dim, D.n1d, K.NT, K.LB)](D.dim, D.n1d, K.NT, K.LB, reaction, pr.n_diag_slots, pr.n_items, pr.direct);
  if (pr.d_mtab)
    pdh_resolve_moment(D.n1d, D.n, pr.n_diag_slots, pr.n_items, pr.moment);
  if (pr.row_kernel == RowKernel::rows)
    pr.row = pdh_resolve_rows(&D, &pr.rows, pr.n_owned, cus, sw.rows_waves_per_cu, sw.rows_lds_pad, sw.rows_verbose, &pr.row_zero_sched);
  else if (pr.row_kernel == RowKernel::terms)
    {
      const char *why = nullptr;
      pr.row = pdh_resolve_terms(&D, &pr.terms, pr.n_owned, cus, sw.terms_wg_waves, sw.terms_wg_batch, pdht::WG_STORE_AUX,
                                 pdht::WG_DRAIN ? 1 : 0, &why);
      if (!pr.row.kernel)
        *why_row = why;
    }
}

static int set_problem_impl(pdh_ctx *ctx, const pdh_problem *p, int32_t row_begin, int32_t row_end, const pdh_cartesian_points *cart);

extern "C" int pdh_set_problem_local(pdh_ctx *ctx, const pdh_problem *p, int32_t row_begin, int32_t row_end)
{
  return set_problem_impl(ctx, p, row_begin, row_end, nullptr);
}

extern "C" int pdh_set_problem_cartesian(pdh_ctx *ctx, const pdh_problem *p, const pdh_cartesian_points *points, int32_t row_begin,
                                         int32_t row_end)
{
  if (!points)
    return fail(ctx, PDH_EINVAL, "points is NULL");
  return set_problem_impl(ctx, p, row_begin, row_end, points);
}

static int set_problem_impl(pdh_ctx *ctx, const pdh_problem *p, int32_t row_begin, int32_t row_end, const pdh_cartesian_points *cart)
{
  PDH_TRY(need_ctx(ctx));
  if (cart && ctx->exchange_mode == PDH_EXCHANGE_GHOST)
    return fail(ctx, PDH_EUNSUPPORTED, "the cartesian description runs owner-computes-rows only (no ghost-block exchange)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_problem(ctx);
  ++ctx->values_gen;
  ++ctx->problem_epoch;
  struct FreeUnlessDone // every exit before the end leaves no problem resident
  {
    pdh_ctx *ctx;
    bool done = false;
    ~FreeUnlessDone()
    {
      if (!done)
        free_problem(ctx);
    }
  } guard{ctx};
  // the diagnostic switches as they stand now, for all of this set-up; PDH_TRACE_SETUP=1: wall time of its phases on stderr
  const PlanSwitches sw = read_plan_switches();
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!sw.trace)
      return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[pdh_set_problem] %-32s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  lap("wait for the stream, free the old problem");

  // 1. host: validate and repack, choose the row kernel
  std::unique_ptr<Packed> K_owner(new Packed);
  Packed &K = *K_owner;
  PDH_TRY(pack_problem(ctx->err, p, row_begin, row_end, K, ctx->exchange_mode, cart));
  lap("validate + repack (host)");
  auto plan = std::make_unique<KernelPlan>(plan_kernels(p, K, sw));
  lap("row kernel plan (host)");
  if (cart && plan->kernel != RowKernel::terms)
    return fail(ctx, PDH_EUNSUPPORTED, "cartesian description: the term kernels do not apply (a polytope's tables exceed their LDS budget, "
                                       "or the element has none): describe the problem with its points (pdh_set_problem)");
  // 2. device: the state every kernel reads
  PDH_TRY(upload_problem(ctx, p, K));
  record_problem(ctx, p, K);
  lap("upload: state of every kernel");
  // 3. device: the state of the row kernel the plan chose, of that one only
  int cus = 256; // (sizes the MULTI scratch and the row kernel's grid)
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  if (plan->kernel == RowKernel::rows)
    {
      PDH_TRY(upload_rows_state(ctx, K, *plan, cus));
      lap("upload: pdh_rows.h state");
    }
  else if (plan->kernel == RowKernel::terms)
    {
      PDH_TRY(upload_terms_state(ctx, K, *plan));
      lap("upload: term kernel state");
    }
  ctx->prob.row_kernel = plan->kernel;
  ctx->prob.why_terms = plan->why_terms;
  // 4. the launches of every form of the problem
  const char *why_row = nullptr;
  resolve_launches(ctx, K, sw, cus, &why_row);
  if (why_row) // (a launch that could not be resolved would answer a bare hipErrorInvalidValue at the first assembly)
    return fail(ctx, PDH_EUNSUPPORTED, std::string("the row kernel chosen for this problem cannot be launched on this device: ") + why_row);
  ctx->prob.resident = true;
  ctx->ev_used = 0;
  guard.done = true;
  K_owner.reset();
  plan.reset();
  lap("release host staging");
  return PDH_OK;
}

extern "C" int pdh_set_algorithm(pdh_ctx *ctx, int algorithm)
{
  PDH_TRY(need_ctx(ctx));
  if (algorithm != PDH_ALG_AUTO && algorithm != PDH_ALG_DIRECT && algorithm != PDH_ALG_MOMENT && algorithm != PDH_ALG_ROWS)
    return fail(ctx, PDH_EINVAL, "algorithm must be PDH_ALG_AUTO, PDH_ALG_DIRECT, PDH_ALG_MOMENT or PDH_ALG_ROWS");
  ctx->algorithm = algorithm;
  return PDH_OK;
}

extern "C" int pdh_algorithm_in_use(pdh_ctx *ctx)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (ctx->use_rows())
    return PDH_ALG_ROWS;
  const bool d = ctx->use_moment(0), o = ctx->use_moment(1);
  return d && o ? PDH_ALG_MOMENT : (d || o ? PDH_ALG_MIXED : PDH_ALG_DIRECT);
}

extern "C" int pdh_rows_kernel_in_use(pdh_ctx *ctx)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!ctx->use_rows())
    return PDH_ROWS_NONE;
  if (ctx->prob.row_kernel == RowKernel::terms)
    return PDH_ROWS_TERMS;
  if (ctx->prob.rows.multi)
    return PDH_ROWS_MULTI;
  return ctx->prob.dev.n == 64 ? PDH_ROWS_PIECES : PDH_ROWS_STREAMED;
}

extern "C" int pdh_set_problem(pdh_ctx *ctx, const pdh_problem *p)
{
  if (!p)
    return fail(ctx, PDH_EINVAL, "problem is NULL");
  return pdh_set_problem_local(ctx, p, 0, p->n_rows);
}

// four profiling events of one launch (pdh_ctx::events)
static int take_events(pdh_ctx *ctx, hipEvent_t (&e)[4])
{
  for (hipEvent_t &x : e)
    x = ctx->next_event();
  if (!e[0] || !e[1] || !e[2] || !e[3])
    return fail(ctx, PDH_EDEVICE, "hipEventCreate failed");
  return PDH_OK;
}

extern "C" int pdh_assemble_device(pdh_ctx *ctx)
{
  PDH_TRY(need_problem(ctx, "pdh_assemble_device"));
  ++ctx->values_gen;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  pdh_ctx::Problem &pr = ctx->prob;
  if (ctx->algorithm == PDH_ALG_MOMENT && !ctx->prob.d_mtab)
    return fail(ctx, PDH_EUNSUPPORTED, "the moment form exists for 3-D bases of degree 1..3 only");
  if (ctx->algorithm == PDH_ALG_ROWS && ctx->prob.row_kernel == RowKernel::none)
    return fail(ctx, PDH_EUNSUPPORTED, "the row kernel does not apply to the resident problem (3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3 on polytopes whose faces are unions of axis-aligned planes, no exchange variant; pdh_check_rows says why)");
  pr.has_values = true;
  pr.galerkin_values = false;
  if (ctx->use_rows())
    { // one launch writes everything; reported as kernel 0, kernel 1 takes no time
      hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
      if (ctx->profiling)
        {
          PDH_TRY(take_events(ctx, ev));
          PDH_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
        }
      if (pr.row_kernel == RowKernel::terms)
        // (always on the context's stream: the launches of a problem share its work counter, pdh_terms_wg.h)
        PDH_HIP(ctx, pdh_launch_terms(&pr.row, &pr.dev, &pr.terms, pr.n_owned, ctx->stream));
      else
        PDH_HIP(ctx, pdh_launch_rows(&pr.row, pr.row_zero_sched, &pr.dev, &pr.rows, pr.d_mtab, pr.n_owned, ctx->stream));
      if (ctx->profiling)
        {
          PDH_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
          PDH_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
          PDH_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
        }
      return PDH_OK;
    }
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (ctx->profiling)
    PDH_TRY(take_events(ctx, ev));
  hipEvent_t e0 = ev[0], e1 = ev[1], f0 = ev[2], f1 = ev[3];
  const bool ov = ctx->overlapped();
  hipStream_t sd = ctx->stream, so = ov ? ctx->stream2 : ctx->stream;
  // launch-bound sizes: replay the captured pair (see pdh_ctx::graph_exec)
  const bool graphable = !ctx->profiling && !ov && ctx->prob.n_values < pdh_ctx::small_values;
  if (graphable && ctx->prob.graph_state == 1 && (ctx->prob.graph_alg != ctx->algorithm || ctx->prob.graph_stream != ctx->stream))
    ctx->prob.drop_graph();
  if (graphable && ctx->prob.graph_state == 1)
    {
      PDH_HIP(ctx, hipGraphLaunch(ctx->prob.graph_exec, ctx->stream));
      return PDH_OK;
    }
  bool capturing = false;
  if (graphable && ctx->prob.graph_state == 0)
    {
      if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess)
        capturing = true;
      else
        {
          (void)hipGetLastError();
          ctx->prob.graph_state = -1;
        }
    }
  auto end_capture = [&](bool ok) {
    if (!capturing)
      return;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (ok && e == hipSuccess && g && hipGraphInstantiate(&ctx->prob.graph_exec, g, nullptr, nullptr, 0) == hipSuccess)
      {
        ctx->prob.graph_state = 1;
        ctx->prob.graph_alg = ctx->algorithm;
        ctx->prob.graph_stream = ctx->stream;
      }
    else
      {
        (void)hipGetLastError();
        ctx->prob.graph_exec = nullptr;
        ctx->prob.graph_state = -1;
      }
    if (g)
      (void)hipGraphDestroy(g);
  };
  // k = 0 own blocks, 1 coupling blocks, in the form the algorithm selects
  auto launch_blocks = [&](int k, int count, hipStream_t s) {
    if (ctx->use_moment(k))
      return pdh_launch_moment(&pr.moment[k], &pr.dev, pr.d_mtab, count, s);
    if (!pr.tiled)
      return pdh_launch_direct(&pr.direct[k], &pr.dev, count, s);
    const hipError_t e = pdh_launch_tiled(&pr.direct[k], &pr.dev, count, s);
    return k == 0 && e == hipSuccess ? pdh_launch_tiled(&pr.direct[2], &pr.dev, count, s) : e;
  };
  if (ov)
    {
      PDH_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
      PDH_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    }
  // diagonal blocks
  if (ctx->profiling)
    PDH_HIP(ctx, hipEventRecord(e0, sd));
  {
    const hipError_t le = launch_blocks(0, pr.n_diag_slots, sd);
    if (le != hipSuccess)
      {
        end_capture(false); // (a stream must not be left in capture mode)
        return fail(ctx, PDH_EDEVICE, std::string("diagonal-block kernel: ") + hipGetErrorString(le));
      }
  }
  if (ctx->profiling)
    PDH_HIP(ctx, hipEventRecord(e1, sd));
  // coupling blocks
  if (ctx->profiling)
    PDH_HIP(ctx, hipEventRecord(f0, so));
  {
    const hipError_t le = launch_blocks(1, pr.n_items, so);
    if (le != hipSuccess)
      {
        end_capture(false);
        return fail(ctx, PDH_EDEVICE, std::string("coupling-block kernel: ") + hipGetErrorString(le));
      }
  }
  if (ctx->profiling)
    PDH_HIP(ctx, hipEventRecord(f1, so));
  if (ov)
    {
      PDH_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
      PDH_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    }
  if (capturing)
    { // nothing ran yet: the launches above were recorded.  Replay them now - or, if the graph could not be built, launch plainly
      end_capture(true);
      if (ctx->prob.graph_state == 1)
        PDH_HIP(ctx, hipGraphLaunch(ctx->prob.graph_exec, ctx->stream));
      else
        return pdh_assemble_device(ctx);
    }
  return PDH_OK;
}

extern "C" int pdh_set_exchange_mode(pdh_ctx *ctx, int mode)
{
  PDH_TRY(need_ctx(ctx));
  if (mode != PDH_EXCHANGE_NONE && mode != PDH_EXCHANGE_GHOST)
    return fail(ctx, PDH_EINVAL, "mode must be PDH_EXCHANGE_NONE or PDH_EXCHANGE_GHOST");
  ctx->exchange_mode = mode; // takes effect at the next pdh_set_problem*
  return PDH_OK;
}

extern "C" int pdh_exchange_layout(pdh_ctx *ctx, int n_ranks, int64_t *send_count, int64_t *recv_count)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!ctx->prob.ghost)
    return fail(ctx, PDH_ESTATE, "the resident problem was not set in PDH_EXCHANGE_GHOST mode");
  if (n_ranks < (int)ctx->prob.send_count.size() || !send_count || !recv_count)
    return fail(ctx, PDH_EINVAL, "n_ranks is smaller than the number of ranks in agg_rank, or an output is NULL");
  for (int r = 0; r < n_ranks; ++r)
    {
      send_count[r] = r < (int)ctx->prob.send_count.size() ? ctx->prob.send_count[r] : 0;
      recv_count[r] = r < (int)ctx->prob.recv_count.size() ? ctx->prob.recv_count[r] : 0;
    }
  return PDH_OK;
}

extern "C" int pdh_exchange_get_send(pdh_ctx *ctx, double *d_send)
{
  if (!resident(ctx) || !ctx->prob.ghost)
    return fail(ctx, PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode");
  if (ctx->prob.n_send == 0)
    return PDH_OK;
  if (!d_send)
    return fail(ctx, PDH_EINVAL, "d_send is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipMemcpyAsync(d_send, ctx->prob.dev.values + ctx->prob.n_values, ctx->prob.n_send * sizeof(double), hipMemcpyDeviceToDevice,
                              ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_exchange_apply(pdh_ctx *ctx, const double *d_recv)
{
  if (!resident(ctx) || !ctx->prob.ghost)
    return fail(ctx, PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode");
  ++ctx->values_gen;
  if (ctx->prob.n_recv == 0)
    return PDH_OK;
  if (!d_recv)
    return fail(ctx, PDH_EINVAL, "d_recv is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, pdh_launch_ghost_apply(&ctx->prob.dev, d_recv, ctx->prob.n_r21, ctx->prob.d_r21_src, ctx->prob.d_r21_dst, ctx->prob.d_r21_rlen, ctx->prob.n_r22,
                                      ctx->prob.d_r22_ptr, ctx->prob.d_r22_src, ctx->prob.d_r22_slot, ctx->stream));
  return PDH_OK;
}

// Run the kernels on a stream of the caller (e.g. the framework's current stream, so that collectives issued there are
// ordered with the assembly without host synchronisation).  NULL restores the context's own stream.
extern "C" int pdh_set_stream(pdh_ctx *ctx, void *stream)
{
  PDH_TRY(need_ctx(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = stream ? (hipStream_t)stream : ctx->own_stream;
  return PDH_OK;
}

// Diagnostic (builds with -DPDHR_STAMP only): s_memtime stamps of the row kernel's phase boundaries and in-phase sums, [n_owned][16].
extern "C" int pdh_debug_rows_stamps(pdh_ctx *ctx, long long *out)
{
  const long long *src = !ctx || !ctx->prob.resident ? nullptr
                         : ctx->prob.row_kernel == RowKernel::terms ? ctx->prob.terms.stamps
                         : ctx->prob.row_kernel == RowKernel::rows ? ctx->prob.rows.stamps
                                                                : nullptr;
  if (!src || !out)
    return fail(ctx, PDH_ESTATE, "no row-kernel problem resident");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PDH_HIP(ctx, hipMemcpy(out, src, (size_t)ctx->prob.n_owned * 16 * sizeof(long long), hipMemcpyDeviceToHost));
  return PDH_OK;
}

#ifdef PDHT_VARIANTS
// Diagnostic (builds with -DPDHT_VARIANTS only): from now on the resident FE_DGQ(3) problem is assembled by k_terms_wg with this store
// policy of the writers - order 0 (piece-major: the one there is); aux 18 (sc1 nt), drain 1: the library's; aux 2 (nt), drain 0: the
// baseline it was chosen against - resolved like the launch of set-up (the switches as they stand now).  The variants of one context
// write the same allocation: tools/paired_bench.py.
extern "C" int pdh_debug_terms_wg_variant(pdh_ctx *ctx, int order, int aux, int drain)
{
  if (!ctx || !ctx->prob.resident || ctx->prob.row_kernel != RowKernel::terms || ctx->prob.dev.n1d != 4 || ctx->prob.dev.n != 64)
    return fail(ctx, PDH_ESTATE, "no FE_DGQ(3) term-kernel problem resident");
  if (order != 0)
    return fail(ctx, PDH_EINVAL, "order must be 0 (piece-major)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const PlanSwitches sw = read_plan_switches();
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  const char *why = nullptr;
  const PdhLaunch L = pdh_resolve_terms(&ctx->prob.dev, &ctx->prob.terms, ctx->prob.n_owned, cus, sw.terms_wg_waves, sw.terms_wg_batch, aux,
                                        drain, &why);
  if (!L.kernel)
    return fail(ctx, PDH_EUNSUPPORTED, why);
  ctx->prob.row = L;
  return PDH_OK;
}
#endif

extern "C" int pdh_set_overlap(pdh_ctx *ctx, int enabled)
{
  PDH_TRY(need_ctx(ctx));
  ctx->overlap = enabled != 0;
  return PDH_OK;
}

extern "C" int pdh_synchronize(pdh_ctx *ctx)
{
  PDH_TRY(need_ctx(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

extern "C" void *pdh_stream(pdh_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int pdh_assemble(pdh_ctx *ctx, double *values)
{
  if (!values)
    return fail(ctx, PDH_EINVAL, "values is NULL");
  int rc = pdh_assemble_device(ctx);
  if (rc != PDH_OK)
    return rc;
  PDH_HIP(ctx, hipMemcpyAsync(values, ctx->prob.dev.values, ctx->prob.n_values * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// Copy of the CSR values as they stand in HBM (after pdh_assemble_device / pdh_exchange_apply), without re-assembling.
extern "C" int pdh_copy_values(pdh_ctx *ctx, double *values)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!values)
    return fail(ctx, PDH_EINVAL, "values is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipMemcpyAsync(values, ctx->prob.dev.values, ctx->prob.n_values * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// sum, sum of |.|, max |.| and number of non-finite entries of the owned rows' values as they stand in HBM
extern "C" int pdh_values_checksum(pdh_ctx *ctx, double *out4)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!out4)
    return fail(ctx, PDH_EINVAL, "out4 is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d = ctx->checksum.get<double>(pdh_checksum_doubles());
  if (!d)
    return fail(ctx, PDH_EDEVICE, "pdh_values_checksum: out of device memory");
  hipError_t e = pdh_launch_checksum(ctx->prob.dev.values, ctx->prob.n_values, d, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out4, d, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess)
    return fail(ctx, PDH_EDEVICE, std::string("pdh_values_checksum: ") + hipGetErrorString(e));
  return PDH_OK;
}

extern "C" int pdh_assemble_sip_local(pdh_ctx *ctx, const pdh_problem *p, int32_t row_begin, int32_t row_end, double *values)
{
  int rc = pdh_set_problem_local(ctx, p, row_begin, row_end);
  if (rc != PDH_OK)
    return rc;
  return pdh_assemble(ctx, values);
}

extern "C" int pdh_assemble_sip(pdh_ctx *ctx, const pdh_problem *p, double *values)
{
  if (!p)
    return fail(ctx, PDH_EINVAL, "problem is NULL");
  return pdh_assemble_sip_local(ctx, p, 0, p->n_rows, values);
}
extern "C" int pdh_device_values(pdh_ctx *ctx, double **device_ptr, int64_t *n_values)
{
  if (!resident(ctx))
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (device_ptr)
    *device_ptr = ctx->prob.dev.values;
  if (n_values)
    *n_values = ctx->prob.n_values;
  return PDH_OK;
}

extern "C" int pdh_set_profiling(pdh_ctx *ctx, int enabled)
{
  PDH_TRY(need_ctx(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->profiling = enabled != 0;
  ctx->ev_used = 0;
  return PDH_OK;
}

extern "C" int pdh_kernel_times_ms(pdh_ctx *ctx, float *ms, int *n_launches)
{
  if (!ctx || !ms)
    return fail(ctx, PDH_EINVAL, "ctx or ms is NULL");
  const size_t nl = ctx->ev_used / 4;
  if (nl == 0)
    return fail(ctx, PDH_ESTATE, "no profiled launch recorded (pdh_set_profiling(1) then pdh_assemble_device)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  double sum[PDH_N_KERNELS] = {0.0, 0.0};
  for (size_t l = 0; l < nl; ++l)
    for (int k = 0; k < PDH_N_KERNELS; ++k)
      {
        float t = 0.f;
        PDH_HIP(ctx, hipEventElapsedTime(&t, ctx->events[4 * l + 2 * k], ctx->events[4 * l + 2 * k + 1]));
        sum[k] += t;
      }
  for (int k = 0; k < PDH_N_KERNELS; ++k)
    ms[k] = (float)(sum[k] / (double)nl);
  if (n_launches)
    *n_launches = (int)nl;
  return PDH_OK;
}

extern "C" int pdh_kernel_work(pdh_ctx *ctx, int64_t *mfma_instr)
{
  if (!resident(ctx) || !mfma_instr)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  mfma_instr[0] = (ctx->use_moment(0) || ctx->use_rows()) ? 0 : ctx->prob.mfma_diag; // counted for the direct form only
  mfma_instr[1] = (ctx->use_moment(1) || ctx->use_rows()) ? 0 : ctx->prob.mfma_offdiag;
  return PDH_OK;
}

extern "C" int pdh_problem_stats(pdh_ctx *ctx, int64_t *stats)
{
  if (!resident(ctx) || !stats)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  stats[0] = ctx->prob.n_owned;
  stats[1] = ctx->prob.n_items;
  stats[2] = ctx->prob.n_vq;
  stats[3] = ctx->prob.n_ap;
  stats[4] = ctx->prob.n_values;
  stats[5] = ctx->prob.dev.n;
  stats[6] = (int64_t)pdh::lds_bytes_diag(ctx->prob.dev.dim, ctx->prob.dev.n1d, ctx->prob.NT);
  stats[7] = (int64_t)pdh::lds_bytes_offdiag(ctx->prob.dev.dim, ctx->prob.dev.n1d, ctx->prob.NT);
  return PDH_OK;
}
