// pdh_capi.cpp — the device driver of the C ABI declared in include/polydeal_hip.h: contexts, uploads, launches, streams, graphs,
// right-hand side, evaluation, exchange and solve.
//
// Host work of SETUP (what the reference does once per mesh in AgglomerationHandler::distribute_agglomerated_dofs /
// setup_connectivity_of_agglomeration / create_agglomeration_sparsity_pattern, source/agglomeration_handler.cc:326-379, 495-527,
// 910-1022) - validation, repacking of the face tables per owning polytope, block positions inside CSR rows, the choice of the row
// kernel and its tables - is the planner's (pdh_plan.h, host-only); pdh_set_problem uploads what it built.
// The assembly itself (pdh_assemble_device) only launches the HIP kernels.
#include "../../include/polydeal_hip.h"
#include "pdh_basis.h"
#include "pdh_combos.h"
#include "pdh_kernels.h"
#include "pdh_launch.h"
#include "pdh_moment_tables.h"
#include "pdh_plan.h"

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

static pdh_launch_fn g_launch[PDH_N_GROUPS] = {pdh_launch_g0, pdh_launch_g1, pdh_launch_g2, pdh_launch_g3,
                                               pdh_launch_g4, pdh_launch_g5, pdh_launch_g6, pdh_launch_g7};

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

struct pdh_ctx
{
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr; // stream = the one in use (own_stream unless pdh_set_stream)
  std::string err;
  bool has_problem = false;
  std::vector<void *> allocs;
  PdhDev dev;
  int n_owned = 0, n_items = 0, NT = 0, LB = 0, group = -1;
  bool tiled = false; // n > 64 dofs per polytope: pdh_tiled.h instead of the kernels of `group`
  int64_t terms_merge[4] = {0, 0, 0, 0}; // term kernels: cells before / after merging, sub-faces before / after
  size_t lds_diag = 0, lds_off = 0;
  int64_t n_values = 0, n_vq = 0, n_ap = 0;
  // host-side maps from the caller's quadrature arrays to the packed device layout (for pdh_assemble_rhs)
  std::vector<int64_t> vq_src;                       // per owned slot: first volume point in the caller's arrays
  struct FaceRun { int64_t ap_begin, fq_begin; int32_t count; int32_t boundary; int32_t slot; };
  std::vector<FaceRun> face_runs;
  int64_t n_rows_owned = 0;
  int32_t n_agg_total = 0;
  // caller-order maps for the right-hand side (device): first caller volume point of every slot; caller face point of every
  // packed face point (-1: not on the boundary); sizes of the caller's point arrays
  const int64_t *d_vq_src = nullptr, *d_ap_src = nullptr;
  const int64_t *d_bd_rng = nullptr; // [n_owned][2] packed face points of every slot that lie on the boundary (one run)
  int64_t n_vq_caller = 0, n_fq_caller = 0;
  // Cartesian description: local face of every sub-face and points per direction (the generated face points run the lower
  // tangential axis fastest, the caller's g_bdry is in QProjector's order - they differ on faces of axis 1: ensure_ap_src)
  std::vector<int32_t> cart_fq_face;
  int cart_nqf = 0;
  // grow-only device scratch for the host-pointer variants of rhs / evaluate / shape_values (no hipMalloc per call)
  struct Scratch { void *p = nullptr; size_t bytes = 0; };
  Scratch scratch[6];
  void *scratch_get(int i, size_t bytes)
  {
    Scratch &s = scratch[i];
    if (bytes > s.bytes)
      {
        if (s.p)
          (void)hipFree(s.p);
        s.p = nullptr;
        s.bytes = 0;
        const size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&s.p, want) != hipSuccess)
          return nullptr;
        s.bytes = want;
      }
    return s.p;
  }
  // solving with the resident matrix (pdh_solve.hip): first global dof of every block of every owned slot in value order, the longest
  // row, the global row count; a generation of the values (bumped by every set_problem / assemble / exchange_apply) against which
  // the preconditioner is checked; grow-only device buffers of the solver (allocated at first use, freed with the problem) and
  // the pinned word the CG loop reads its residual through
  const int64_t *d_blk_ptr = nullptr;
  const int32_t *d_blk_dof = nullptr;
  int max_row_len = 0;
  int64_t n_rows_total = 0;
  uint64_t values_gen = 0, prec_gen = 0;
  int prec_kind = PDH_PREC_NONE;
  bool prec_ok = true;
  enum { SOL_DINV, SOL_FLAG, SOL_R, SOL_Z, SOL_P, SOL_Q, SOL_PART, SOL_SCAL, SOL_CHEB_D, SOL_CHEB_R, SOL_N };
  Scratch sol[SOL_N];
  double *pinned = nullptr; // [PDH_CG_NSCALARS]
  // PDH_PREC_CHEBYSHEV (pdh_setup_chebyshev): the inner kind whose inverse lies in SOL_DINV and, per step k, the factors of d_(k-1)
  // and of P^-1 r_k in d_k (step 0: unused and 1 / theta)
  int cheb_inner = PDH_PREC_NONE;
  std::vector<double> cheb_c1, cheb_c2;
  template <class T>
  T *sol_get(int i, size_t count)
  {
    Scratch &s = sol[i];
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (bytes > s.bytes)
      {
        if (s.p)
          (void)hipFree(s.p);
        s.p = nullptr;
        s.bytes = 0;
        if (hipMalloc(&s.p, bytes) != hipSuccess)
          return nullptr;
        s.bytes = bytes;
      }
    return static_cast<T *>(s.p);
  }
  void free_solver()
  {
    for (auto &s : sol)
      {
        if (s.p)
          (void)hipFree(s.p);
        s = Scratch{};
      }
  }
  // cached multi-index table of pdh_shape_values (per dim/degree/basis)
  int shape_key = -1;
  int32_t *d_shape_midx = nullptr;
  int64_t mfma_diag = 0, mfma_offdiag = 0; // MFMA instructions per launch
  // ghost-block exchange variant (pdh_set_exchange_mode); n_diag_slots = n_owned + pseudo slots of the outgoing M22 sums
  int exchange_mode = PDH_EXCHANGE_NONE;
  bool problem_ghost = false;
  int n_diag_slots = 0, n_r21 = 0, n_r22 = 0;
  int64_t n_send = 0, n_recv = 0;
  std::vector<int64_t> send_count, recv_count;
  const int64_t *d_r21_src = nullptr, *d_r21_dst = nullptr, *d_r22_ptr = nullptr, *d_r22_src = nullptr;
  const int32_t *d_r21_rlen = nullptr, *d_r22_slot = nullptr;
  // moment form (pdh_moment.h): available for 3-D bases of degree <= 3; `algorithm` = caller's choice
  int algorithm = PDH_ALG_AUTO;
  int basis = 0;
  const double *d_mtab = nullptr;
  // The row kernel of the problem, if any (set_problem builds the device state of that one only): pdh_rows.h where every face
  // of every owned polytope is a union of axis-aligned planes; the term kernel (pdh_terms.h) on agglomerates of Cartesian cells
  // with tensor rules - any number of planes per neighbour - is taken instead wherever its tables fit the LDS budget.
  RowKernel row_kernel = RowKernel::none;
  PdhRows rows;
  PdhTerms terms;
  // AUTO takes the row kernel where it applies (degree 1 since 12 waves per CU are resident: 0.21 vs 0.24-0.30 ms)
  bool use_rows() const
  {
    return row_kernel != RowKernel::none && (algorithm == PDH_ALG_AUTO || algorithm == PDH_ALG_ROWS);
  }
  // which form each of the two launches uses: [0] diagonal blocks, [1] coupling blocks
  bool use_moment(int kind) const
  {
    if (!d_mtab || algorithm == PDH_ALG_DIRECT)
      return false;
    if (algorithm == PDH_ALG_MOMENT)
      return true;
    if (algorithm == PDH_ALG_ROWS)
      return false;
    // auto: where the moment form was measured faster than the MFMA contraction (profiles/README.md): FE_DGQ(3) both
    // kinds (8.5 -> 4.7 ms), FE_DGQ(2) the diagonal blocks only (BASELINE configs[3]: 9.7 -> 5.6 ms; its coupling blocks
    // 4.3 ms direct vs 6.4 ms moment)
    if (basis != PDH_BASIS_DGQ)
      return false;
    return dev.n1d == 4 || (dev.n1d == 3 && kind == 0);
  }
  // The two kernels of a step write disjoint values and have complementary bottlenecks (the diagonal items compute, the
  // coupling items mostly store): on large problems they run concurrently, the coupling kernel on stream2, forked from /
  // joined into `stream` by events so that the caller still sees one ordered stream.  Measured -4 % per step.
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int overlap = 1; // pdh_set_overlap
  // (two streams pay for their fork / join events only when the kernels run for a while: by the size of the matrix)
  static constexpr int64_t small_values = 16 << 20;
  bool overlapped() const { return overlap && stream2 && (int64_t)n_diag_slots + n_items >= 8192 && n_values >= small_values; }
  // Small problems are bound by the launches themselves (two kernels of a few microseconds each): the pair is captured
  // into a hipGraph once per (problem, algorithm, stream) and replayed with ONE launch.  graph_state: 0 none yet, 1 ready,
  // -1 capture failed on this problem (plain launches from then on).
  hipGraphExec_t graph_exec = nullptr;
  int graph_state = 0, graph_alg = -1;
  hipStream_t graph_stream = nullptr;
  void drop_graph()
  {
    if (graph_exec)
      (void)hipGraphExecDestroy(graph_exec);
    graph_exec = nullptr;
    graph_state = 0;
  }
  bool profiling = false;
  std::vector<hipEvent_t> events; // 4 per profiled launch: before / after the diagonal kernel, before / after the coupling kernel
  size_t ev_used = 0;
  hipEvent_t next_event()
  {
    if (ev_used == events.size())
      {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess)
          return nullptr;
        events.push_back(e);
      }
    return events[ev_used++];
  }
};

static int fail(pdh_ctx *ctx, int code, const std::string &msg)
{
  (ctx ? ctx->err : pdh_noctx_error()) = msg;
  return code;
}

#define PDH_HIP(ctx, call)                                                                         \
  do                                                                                               \
    {                                                                                              \
      hipError_t e_ = (call);                                                                      \
      if (e_ != hipSuccess)                                                                        \
        return fail(ctx, PDH_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_));          \
    }                                                                                              \
  while (0)

#define PDH_TRY(call)                                                                              \
  do                                                                                               \
    {                                                                                              \
      const int rc_ = (call);                                                                      \
      if (rc_ != PDH_OK)                                                                           \
        return rc_;                                                                                \
    }                                                                                              \
  while (0)

static void free_problem(pdh_ctx *ctx)
{
  for (void *p : ctx->allocs)
    (void)hipFree(p);
  ctx->allocs.clear();
  ctx->drop_graph();
  ctx->free_solver();
  ctx->has_problem = false;
  ctx->d_blk_ptr = nullptr;
  ctx->d_blk_dof = nullptr;
  ctx->d_ap_src = nullptr;
  ctx->d_bd_rng = nullptr;
  ctx->d_mtab = nullptr;
  ctx->row_kernel = RowKernel::none;
  ctx->rows = PdhRows{};
  ctx->terms = PdhTerms{};
}

// Device memory of set-up: `count` elements (at least one), recorded in `owner` - ctx->allocs for the resident problem (freed
// by free_problem), Staging::bufs for the inputs of one set-up step; PDH_EDEVICE says what failed
template <class T>
static int alloc_in(pdh_ctx *ctx, std::vector<void *> &owner, size_t count, T **dptr, const char *what)
{
  void *d = nullptr;
  const hipError_t e = hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess)
    return fail(ctx, PDH_EDEVICE, std::string("hipMalloc (") + what + "): " + hipGetErrorString(e));
  owner.push_back(d);
  *dptr = static_cast<T *>(d);
  return PDH_OK;
}
template <class T>
static int upload_in(pdh_ctx *ctx, std::vector<void *> &owner, const T *h, size_t count, const T **dptr, const char *what)
{
  T *d = nullptr;
  PDH_TRY(alloc_in(ctx, owner, count, &d, what));
  *dptr = d;
  const hipError_t e = count ? hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  return e == hipSuccess ? PDH_OK : fail(ctx, PDH_EDEVICE, std::string("upload (") + what + "): " + hipGetErrorString(e));
}

// persistent buffers of the resident problem
template <class T>
static int device_buffer(pdh_ctx *ctx, size_t count, T **dptr, const char *what)
{
  return alloc_in(ctx, ctx->allocs, count, dptr, what);
}
template <class T>
static int upload(pdh_ctx *ctx, const T *h, size_t count, const T **dptr, const char *what)
{
  return upload_in(ctx, ctx->allocs, h, count, dptr, what);
}
template <class V>
static int upload(pdh_ctx *ctx, const V &h, const typename V::value_type **dptr, const char *what)
{
  return upload_in(ctx, ctx->allocs, h.data(), h.size(), dptr, what);
}
#define PDH_UP(vec, field) PDH_TRY(upload(ctx, vec, &field, #field))

// temporary buffers of one set-up step (the inputs of a generating / repacking kernel): freed when the step's scope ends
struct Staging
{
  pdh_ctx *ctx;
  std::vector<void *> bufs;
  explicit Staging(pdh_ctx *c) : ctx(c) {}
  Staging(const Staging &) = delete;
  Staging &operator=(const Staging &) = delete;
  ~Staging()
  {
    for (void *d : bufs)
      (void)hipFree(d);
  }
  template <class T>
  int alloc(size_t count, T **dptr, const char *what)
  {
    return alloc_in(ctx, bufs, count, dptr, what);
  }
  template <class T>
  int upload(const T *h, size_t count, const T **dptr, const char *what)
  {
    return upload_in(ctx, bufs, h, count, dptr, what);
  }
};

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
  free_problem(ctx);
  for (auto &sc : ctx->scratch)
    if (sc.p)
      (void)hipFree(sc.p);
  if (ctx->d_shape_midx)
    (void)hipFree(ctx->d_shape_midx);
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
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_terms_merge_stats called before pdh_set_problem");
  for (int i = 0; i < 4; ++i)
    out4[i] = ctx->row_kernel == RowKernel::terms ? ctx->terms_merge[i] : 0;
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
  PdhDev &D = ctx->dev;
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
  PDH_UP(K.blk_ptr, ctx->d_blk_ptr);
  PDH_UP(K.blk_dof, ctx->d_blk_dof);
  if (K.ghost)
    {
      PDH_UP(K.r21_src, ctx->d_r21_src);
      PDH_UP(K.r21_dst, ctx->d_r21_dst);
      PDH_UP(K.r21_rlen, ctx->d_r21_rlen);
      PDH_UP(K.r22_ptr, ctx->d_r22_ptr);
      PDH_UP(K.r22_src, ctx->d_r22_src);
      PDH_UP(K.r22_slot, ctx->d_r22_slot);
    }
  PDH_TRY(device_buffer(ctx, (size_t)(K.n_values + K.n_send), &D.values, "values"));
  // (the per-point map of the packed boundary points to the caller's face points - 8 bytes per packed face point - is needed by
  // the right-hand side only: built and uploaded at its first call, ensure_ap_src)
  PDH_UP(K.vq_src, ctx->d_vq_src);
  if (p->dim == 3 && K.n1d >= 2 && K.n1d <= 4)
    {
      const std::vector<double> mt = pdh::moment_tables(p->degree, p->basis);
      if ((int)mt.size() != pdhm::moment_table_doubles(K.n1d))
        return fail(ctx, PDH_EDEVICE, "moment tables: the host's and the kernels' sizes differ");
      PDH_UP(mt, ctx->d_mtab);
    }
  return PDH_OK;
}

// Host side of the resident problem: sizes, the caller-order maps of the right-hand side, the kernels' launch shapes and work.
static void record_problem(pdh_ctx *ctx, const pdh_problem *p, const Packed &K)
{
  ctx->problem_ghost = K.ghost;
  ctx->n_send = K.n_send;
  ctx->n_recv = K.n_recv;
  ctx->send_count = K.send_count;
  ctx->recv_count = K.recv_count;
  ctx->n_r21 = (int)K.r21_src.size();
  ctx->n_r22 = (int)K.r22_slot.size();
  ctx->n_values = K.n_values;
  ctx->n_owned = K.n_owned;
  ctx->n_diag_slots = (int)K.own_agg.size();
  ctx->n_items = (int)K.it_own.size();
  ctx->n_vq = K.n_vq;
  ctx->n_ap = K.n_ap;
  ctx->NT = K.NT;
  ctx->LB = K.LB;
  ctx->tiled = K.tiled;
  ctx->group = K.tiled ? -1 : combo_group(p->dim, K.n1d, K.NT, K.LB);
  ctx->lds_diag = pdh::lds_bytes_diag(p->dim, K.n1d, K.NT);
  ctx->lds_off = pdh::lds_bytes_offdiag(p->dim, K.n1d, K.NT);
  ctx->basis = p->basis;
  ctx->vq_src = K.vq_src;
  ctx->n_vq_caller = p->vq_ptr[p->n_agg];
  ctx->n_fq_caller = p->n_faces ? p->fq_ptr[p->n_faces] : 0;
  ctx->cart_fq_face.clear();
  ctx->cart_nqf = 0;
  if (K.cart && K.cart->nqf > 0)
    {
      ctx->cart_nqf = K.cart->nqf;
      ctx->cart_fq_face.assign(K.cart->fq_face, K.cart->fq_face + ctx->n_fq_caller / ((int64_t)K.cart->nqf * K.cart->nqf));
    }
  ctx->face_runs.clear();
  ctx->face_runs.reserve(K.run_ap.size());
  for (size_t r = 0; r < K.run_ap.size(); ++r)
    ctx->face_runs.push_back({K.run_ap[r], K.run_fq[r], K.run_cnt[r], K.run_bdry[r], K.run_slot[r]});
  ctx->n_rows_owned = (int64_t)K.n_owned * K.n;
  ctx->n_rows_total = p->n_rows;
  ctx->max_row_len = K.max_row_len;
  ctx->n_agg_total = p->n_agg;
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
  ctx->mfma_diag = kv * (p->dim + (p->reaction_c != 0.0 ? 1 : 0)) * i_sym + kf * 2 * i_sym;
  ctx->mfma_offdiag = ko * 2 * i_full;
  if (K.tiled)
    { // tiles ti < tj of the own block and all tiles of a coupling block are full 64 x 64 products (64 instructions per k-step), the
      // tiles ti == tj symmetric ones (the schedule of a full n = 64 block)
      const int64_t nt = (K.n + 63) / 64, i64 = sched_instr_rt(4, 4, true);
      ctx->mfma_diag = (kv * (p->dim + (p->reaction_c != 0.0 ? 1 : 0)) + kf * 2) * (64 * (nt * (nt - 1) / 2) + i64 * nt);
      ctx->mfma_offdiag = ko * 2 * 64 * nt * nt;
    }
}

// pdh_rows.h: face tables and per-slot records, the work counter of the persistent waves, the stamps of -DPDHR_STAMP builds and,
// for the MULTI instantiation, a scratch row per resident wave
static int upload_rows_state(pdh_ctx *ctx, const Packed &K, const KernelPlan &plan)
{
  const RowsHost &RH = plan.rows;
  PdhRows &R = ctx->rows;
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
      int cus = 256;
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
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
// stamps of -DPDHT_STAMP builds
static int upload_terms_state(pdh_ctx *ctx, const Packed &K, const KernelPlan &plan)
{
  const TermsHost &TH = plan.terms;
  PdhTerms &T = ctx->terms;
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
  PDH_HIP(ctx, pdh_launch_terms_gather(&ctx->dev, &T, tdata, K.n_owned, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t n_stamps = (size_t)std::max(K.n_owned, 1) * 16;
  PDH_TRY(device_buffer(ctx, n_stamps, &T.stamps, "term kernel: stamps"));
  PDH_HIP(ctx, hipMemset(T.stamps, 0, n_stamps * sizeof(long long)));
  ctx->terms_merge[0] = TH.n_cells_in, ctx->terms_merge[1] = TH.n_cells_out;
  ctx->terms_merge[2] = TH.n_sf_in, ctx->terms_merge[3] = TH.n_sf_out;
  return PDH_OK;
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
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (cart && ctx->exchange_mode == PDH_EXCHANGE_GHOST)
    return fail(ctx, PDH_EUNSUPPORTED, "the cartesian description runs owner-computes-rows only (no ghost-block exchange)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_problem(ctx);
  ++ctx->values_gen;
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
  // PDH_TRACE_SETUP=1 (diagnostics): wall time of the phases of this call on stderr
  static const bool trace = getenv("PDH_TRACE_SETUP") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!trace)
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
  auto plan = std::make_unique<KernelPlan>(plan_kernels(p, K, true));
  lap("row kernel plan (host)");
  if (cart && plan->kernel != RowKernel::terms)
    return fail(ctx, PDH_EUNSUPPORTED, "cartesian description: the term kernels do not apply (a polytope's tables exceed their LDS budget, "
                                       "or the element has none): describe the problem with its points (pdh_set_problem)");
  // 2. device: the state every kernel reads
  PDH_TRY(upload_problem(ctx, p, K));
  record_problem(ctx, p, K);
  lap("upload: state of every kernel");
  // 3. device: the state of the row kernel the plan chose, of that one only
  if (plan->kernel == RowKernel::rows)
    {
      PDH_TRY(upload_rows_state(ctx, K, *plan));
      lap("upload: pdh_rows.h state");
    }
  else if (plan->kernel == RowKernel::terms)
    {
      PDH_TRY(upload_terms_state(ctx, K, *plan));
      lap("upload: term kernel state");
    }
  ctx->row_kernel = plan->kernel;
  ctx->has_problem = true;
  ctx->ev_used = 0;
  guard.done = true;
  K_owner.reset();
  plan.reset();
  lap("release host staging");
  return PDH_OK;
}

extern "C" int pdh_set_algorithm(pdh_ctx *ctx, int algorithm)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (algorithm != PDH_ALG_AUTO && algorithm != PDH_ALG_DIRECT && algorithm != PDH_ALG_MOMENT && algorithm != PDH_ALG_ROWS)
    return fail(ctx, PDH_EINVAL, "algorithm must be PDH_ALG_AUTO, PDH_ALG_DIRECT, PDH_ALG_MOMENT or PDH_ALG_ROWS");
  ctx->algorithm = algorithm;
  return PDH_OK;
}

extern "C" int pdh_algorithm_in_use(pdh_ctx *ctx)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (ctx->use_rows())
    return PDH_ALG_ROWS;
  const bool d = ctx->use_moment(0), o = ctx->use_moment(1);
  return d && o ? PDH_ALG_MOMENT : (d || o ? PDH_ALG_MIXED : PDH_ALG_DIRECT);
}

extern "C" int pdh_rows_kernel_in_use(pdh_ctx *ctx)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!ctx->use_rows())
    return PDH_ROWS_NONE;
  if (ctx->row_kernel == RowKernel::terms)
    return PDH_ROWS_TERMS;
  if (ctx->rows.multi)
    return PDH_ROWS_MULTI;
  return ctx->dev.n == 64 ? PDH_ROWS_PIECES : PDH_ROWS_STREAMED;
}

extern "C" int pdh_set_problem(pdh_ctx *ctx, const pdh_problem *p)
{
  if (!p)
    return fail(ctx, PDH_EINVAL, "problem is NULL");
  return pdh_set_problem_local(ctx, p, 0, p->n_rows);
}

extern "C" int pdh_assemble_device(pdh_ctx *ctx)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_assemble_device called before pdh_set_problem");
  ++ctx->values_gen;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  pdh_launch_fn fn = ctx->tiled ? nullptr : g_launch[ctx->group];
  const int dim = ctx->dev.dim, n1d = ctx->dev.n1d, nt = ctx->NT, lb = ctx->LB;
  if (ctx->algorithm == PDH_ALG_MOMENT && !ctx->d_mtab)
    return fail(ctx, PDH_EUNSUPPORTED, "the moment form exists for 3-D bases of degree 1..3 only");
  if (ctx->algorithm == PDH_ALG_ROWS && ctx->row_kernel == RowKernel::none)
    return fail(ctx, PDH_EUNSUPPORTED, "the row kernel does not apply to the resident problem (3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3 on polytopes whose faces are unions of axis-aligned planes, no exchange variant; pdh_check_rows says why)");
  if (ctx->use_rows())
    { // one launch writes everything; reported as kernel 0, kernel 1 takes no time
      hipEvent_t r0 = nullptr, r1 = nullptr, z0 = nullptr, z1 = nullptr;
      if (ctx->profiling)
        {
          r0 = ctx->next_event();
          r1 = ctx->next_event();
          z0 = ctx->next_event();
          z1 = ctx->next_event();
          if (!r0 || !r1 || !z0 || !z1)
            return fail(ctx, PDH_EDEVICE, "hipEventCreate failed");
          PDH_HIP(ctx, hipEventRecord(r0, ctx->stream));
        }
      if (ctx->row_kernel == RowKernel::terms)
        PDH_HIP(ctx, pdh_launch_terms(&ctx->dev, &ctx->terms, ctx->n_owned, ctx->stream));
      else
        PDH_HIP(ctx, pdh_launch_rows(&ctx->dev, &ctx->rows, ctx->d_mtab, ctx->n_owned, ctx->stream));
      if (ctx->profiling)
        {
          PDH_HIP(ctx, hipEventRecord(r1, ctx->stream));
          PDH_HIP(ctx, hipEventRecord(z0, ctx->stream));
          PDH_HIP(ctx, hipEventRecord(z1, ctx->stream));
        }
      return PDH_OK;
    }
  hipEvent_t e0 = nullptr, e1 = nullptr, f0 = nullptr, f1 = nullptr;
  if (ctx->profiling)
    {
      e0 = ctx->next_event();
      e1 = ctx->next_event();
      f0 = ctx->next_event();
      f1 = ctx->next_event();
      if (!e0 || !e1 || !f0 || !f1)
        return fail(ctx, PDH_EDEVICE, "hipEventCreate failed");
    }
  const bool ov = ctx->overlapped();
  hipStream_t sd = ctx->stream, so = ov ? ctx->stream2 : ctx->stream;
  // launch-bound sizes: replay the captured pair (see pdh_ctx::graph_exec)
  const bool graphable = !ctx->profiling && !ov && ctx->n_values < pdh_ctx::small_values;
  if (graphable && ctx->graph_state == 1 && (ctx->graph_alg != ctx->algorithm || ctx->graph_stream != ctx->stream))
    ctx->drop_graph();
  if (graphable && ctx->graph_state == 1)
    {
      PDH_HIP(ctx, hipGraphLaunch(ctx->graph_exec, ctx->stream));
      return PDH_OK;
    }
  bool capturing = false;
  if (graphable && ctx->graph_state == 0)
    {
      if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess)
        capturing = true;
      else
        {
          (void)hipGetLastError();
          ctx->graph_state = -1;
        }
    }
  auto end_capture = [&](bool ok) {
    if (!capturing)
      return;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (ok && e == hipSuccess && g && hipGraphInstantiate(&ctx->graph_exec, g, nullptr, nullptr, 0) == hipSuccess)
      {
        ctx->graph_state = 1;
        ctx->graph_alg = ctx->algorithm;
        ctx->graph_stream = ctx->stream;
      }
    else
      {
        (void)hipGetLastError();
        ctx->graph_exec = nullptr;
        ctx->graph_state = -1;
      }
    if (g)
      (void)hipGraphDestroy(g);
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
    const hipError_t le = ctx->use_moment(0) ? pdh_launch_moment(n1d, 0, &ctx->dev, ctx->d_mtab, ctx->n_diag_slots, sd)
                          : ctx->tiled     ? pdh_launch_tiled(dim, n1d, ctx->dev.reaction_c != 0.0 ? 2 : 0, &ctx->dev, ctx->n_diag_slots, sd)
                                           : fn(dim, n1d, nt, lb, ctx->dev.reaction_c != 0.0 ? 2 : 0, &ctx->dev, ctx->n_diag_slots,
                                                ctx->lds_diag, sd);
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
    const hipError_t le = ctx->use_moment(1) ? pdh_launch_moment(n1d, 1, &ctx->dev, ctx->d_mtab, ctx->n_items, so)
                          : ctx->tiled     ? pdh_launch_tiled(dim, n1d, 1, &ctx->dev, ctx->n_items, so)
                                           : fn(dim, n1d, nt, lb, 1, &ctx->dev, ctx->n_items, ctx->lds_off, so);
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
      if (ctx->graph_state == 1)
        PDH_HIP(ctx, hipGraphLaunch(ctx->graph_exec, ctx->stream));
      else
        return pdh_assemble_device(ctx);
    }
  return PDH_OK;
}


extern "C" int pdh_set_exchange_mode(pdh_ctx *ctx, int mode)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (mode != PDH_EXCHANGE_NONE && mode != PDH_EXCHANGE_GHOST)
    return fail(ctx, PDH_EINVAL, "mode must be PDH_EXCHANGE_NONE or PDH_EXCHANGE_GHOST");
  ctx->exchange_mode = mode; // takes effect at the next pdh_set_problem*
  return PDH_OK;
}

extern "C" int pdh_exchange_layout(pdh_ctx *ctx, int n_ranks, int64_t *send_count, int64_t *recv_count)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!ctx->problem_ghost)
    return fail(ctx, PDH_ESTATE, "the resident problem was not set in PDH_EXCHANGE_GHOST mode");
  if (n_ranks < (int)ctx->send_count.size() || !send_count || !recv_count)
    return fail(ctx, PDH_EINVAL, "n_ranks is smaller than the number of ranks in agg_rank, or an output is NULL");
  for (int r = 0; r < n_ranks; ++r)
    {
      send_count[r] = r < (int)ctx->send_count.size() ? ctx->send_count[r] : 0;
      recv_count[r] = r < (int)ctx->recv_count.size() ? ctx->recv_count[r] : 0;
    }
  return PDH_OK;
}

extern "C" int pdh_exchange_get_send(pdh_ctx *ctx, double *d_send)
{
  if (!ctx || !ctx->has_problem || !ctx->problem_ghost)
    return fail(ctx, PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode");
  if (ctx->n_send == 0)
    return PDH_OK;
  if (!d_send)
    return fail(ctx, PDH_EINVAL, "d_send is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipMemcpyAsync(d_send, ctx->dev.values + ctx->n_values, ctx->n_send * sizeof(double), hipMemcpyDeviceToDevice,
                              ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_exchange_apply(pdh_ctx *ctx, const double *d_recv)
{
  if (!ctx || !ctx->has_problem || !ctx->problem_ghost)
    return fail(ctx, PDH_ESTATE, "no problem resident in PDH_EXCHANGE_GHOST mode");
  ++ctx->values_gen;
  if (ctx->n_recv == 0)
    return PDH_OK;
  if (!d_recv)
    return fail(ctx, PDH_EINVAL, "d_recv is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, pdh_launch_ghost_apply(&ctx->dev, d_recv, ctx->n_r21, ctx->d_r21_src, ctx->d_r21_dst, ctx->d_r21_rlen, ctx->n_r22,
                                      ctx->d_r22_ptr, ctx->d_r22_src, ctx->d_r22_slot, ctx->stream));
  return PDH_OK;
}

// Run the kernels on a stream of the caller (e.g. the framework's current stream, so that collectives issued there are
// ordered with the assembly without host synchronisation).  NULL restores the context's own stream.
extern "C" int pdh_set_stream(pdh_ctx *ctx, void *stream)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = stream ? (hipStream_t)stream : ctx->own_stream;
  return PDH_OK;
}

// Diagnostic (builds with -DPDHR_STAMP only): s_memtime stamps of the row kernel's phase boundaries and in-phase sums, [n_owned][16].
extern "C" int pdh_debug_rows_stamps(pdh_ctx *ctx, long long *out)
{
  const long long *src = !ctx || !ctx->has_problem ? nullptr
                         : ctx->row_kernel == RowKernel::terms ? ctx->terms.stamps
                         : ctx->row_kernel == RowKernel::rows ? ctx->rows.stamps
                                                                : nullptr;
  if (!src || !out)
    return fail(ctx, PDH_ESTATE, "no row-kernel problem resident");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  PDH_HIP(ctx, hipMemcpy(out, src, (size_t)ctx->n_owned * 16 * sizeof(long long), hipMemcpyDeviceToHost));
  return PDH_OK;
}

extern "C" int pdh_set_overlap(pdh_ctx *ctx, int enabled)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  ctx->overlap = enabled != 0;
  return PDH_OK;
}

extern "C" int pdh_synchronize(pdh_ctx *ctx)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
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
  PDH_HIP(ctx, hipMemcpyAsync(values, ctx->dev.values, ctx->n_values * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// Copy of the CSR values as they stand in HBM (after pdh_assemble_device / pdh_exchange_apply), without re-assembling.
extern "C" int pdh_copy_values(pdh_ctx *ctx, double *values)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!values)
    return fail(ctx, PDH_EINVAL, "values is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, hipMemcpyAsync(values, ctx->dev.values, ctx->n_values * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}


// sum, sum of |.|, max |.| and number of non-finite entries of the owned rows' values as they stand in HBM
extern "C" int pdh_values_checksum(pdh_ctx *ctx, double *out4)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (!out4)
    return fail(ctx, PDH_EINVAL, "out4 is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d = nullptr;
  PDH_HIP(ctx, hipMalloc((void **)&d, 4 * sizeof(double)));
  hipError_t e = pdh_launch_checksum(ctx->dev.values, ctx->n_values, d, ctx->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out4, d, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
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

// ---- right-hand side -------------------------------------------------------------------------------------------------
// packed boundary point -> the caller's face point (-1: interior), for the Nitsche datum; once per problem
static int ensure_ap_src(pdh_ctx *ctx)
{
  if (ctx->d_ap_src)
    return PDH_OK;
  std::vector<int64_t> ap_src((size_t)std::max<int64_t>(ctx->n_ap, 1), -1);
  // Cartesian description: the packed points are the generated ones (pdh_cartgen.hip: lower tangential axis fastest); the caller
  // samples g_bdry at the points of the equivalent points description, QProjector's order (y, z), (z, x), (x, y) - on the faces of
  // axis 1 the two tangential indices are swapped
  const int64_t nqf = ctx->cart_nqf, m2 = nqf * nqf;
  auto caller = [&](int64_t q) {
    if (!nqf || (ctx->cart_fq_face[(size_t)(q / m2)] >> 1) != 1)
      return q;
    const int64_t l = q % m2;
    return q - l + (l / nqf) + nqf * (l % nqf);
  };
  host_parallel_for(ctx->face_runs.size(), [&](size_t r) {
    const auto &fr = ctx->face_runs[r];
    if (fr.boundary)
      for (int32_t t = 0; t < fr.count; ++t)
        ap_src[fr.ap_begin + t] = caller(fr.fq_begin + t);
  });
  // the boundary points of a slot are one contiguous run (all boundary sub-faces form ONE polytopal face, reference
  // source/agglomeration_handler.cc:1575-1613): the kernel visits only that range
  std::vector<int64_t> bd((size_t)std::max(ctx->n_owned, 1) * 2, 0);
  for (const auto &fr : ctx->face_runs)
    if (fr.boundary && fr.slot >= 0 && fr.slot < ctx->n_owned)
      {
        int64_t &b = bd[(size_t)fr.slot * 2], &e = bd[(size_t)fr.slot * 2 + 1];
        if (e == b)
          b = fr.ap_begin, e = fr.ap_begin + fr.count;
        else
          b = std::min(b, fr.ap_begin), e = std::max(e, fr.ap_begin + fr.count); // (several runs: their hull; interior points in between carry no datum)
      }
  PDH_TRY(upload(ctx, bd, &ctx->d_bd_rng, "boundary ranges of the right-hand side"));
  return upload(ctx, ap_src, &ctx->d_ap_src, "caller face points of the right-hand side");
}

extern "C" int pdh_assemble_rhs_device(pdh_ctx *ctx, const double *d_f_vol, const double *d_g_bdry, double *d_rhs)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_assemble_rhs called before pdh_set_problem");
  if (!d_rhs)
    return fail(ctx, PDH_EINVAL, "rhs is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int rc_map = ensure_ap_src(ctx);
  if (rc_map != PDH_OK)
    return rc_map;
  PDH_HIP(ctx, pdh_launch_rhs(ctx->dev.dim, ctx->dev.n1d, &ctx->dev, ctx->n_owned, d_f_vol, d_g_bdry, d_rhs, ctx->d_vq_src,
                              ctx->d_ap_src, ctx->d_bd_rng, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_assemble_rhs(pdh_ctx *ctx, const double *f_vol, const double *g_bdry, double *rhs)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_assemble_rhs called before pdh_set_problem");
  if (!rhs)
    return fail(ctx, PDH_EINVAL, "rhs is NULL");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  // the caller's samples go up as they are (caller order; the kernel indexes them through the maps made at set_problem)
  double *d_f = nullptr, *d_g = nullptr;
  double *d_rhs = static_cast<double *>(ctx->scratch_get(2, std::max<int64_t>(ctx->n_rows_owned, 1) * sizeof(double)));
  if (f_vol)
    d_f = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(ctx->n_vq_caller, 1) * sizeof(double)));
  if (g_bdry)
    d_g = static_cast<double *>(ctx->scratch_get(1, std::max<int64_t>(ctx->n_fq_caller, 1) * sizeof(double)));
  if (!d_rhs || (f_vol && !d_f) || (g_bdry && !d_g))
    return fail(ctx, PDH_EDEVICE, "pdh_assemble_rhs: out of device memory");
  if (f_vol)
    PDH_HIP(ctx, hipMemcpyAsync(d_f, f_vol, ctx->n_vq_caller * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (g_bdry)
    PDH_HIP(ctx, hipMemcpyAsync(d_g, g_bdry, ctx->n_fq_caller * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const int rc = pdh_assemble_rhs_device(ctx, d_f, d_g, d_rhs);
  if (rc != PDH_OK)
    return rc;
  PDH_HIP(ctx, hipMemcpyAsync(rhs, d_rhs, ctx->n_rows_owned * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
extern "C" int pdh_evaluate_device(pdh_ctx *ctx, const double *d_solution, const int64_t *d_pt_ptr, const double *d_pts,
                                   int64_t n_points, double *d_u, double *d_grad)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_evaluate called before pdh_set_problem");
  if (!d_solution || !d_pt_ptr || !d_pts || !d_u || n_points < 0)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts and u are required");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  PDH_HIP(ctx, pdh_launch_eval(ctx->dev.dim, ctx->dev.n1d, d_grad ? 1 : 0, &ctx->dev, ctx->n_owned, d_solution, d_pt_ptr, d_pts,
                               n_points, d_u, d_grad, 1, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_evaluate(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, double *u,
                            double *grad)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_evaluate called before pdh_set_problem");
  if (!solution || !pt_ptr || !pts || !u)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts and u are required");
  const int nA = ctx->n_agg_total, dim = ctx->dev.dim;
  if (pt_ptr[0] != 0)
    return fail(ctx, PDH_EINVAL, "pt_ptr[0] must be 0");
  for (int a = 0; a < nA; ++a)
    if (pt_ptr[a + 1] < pt_ptr[a])
      return fail(ctx, PDH_EINVAL, "pt_ptr must be non-decreasing");
  const int64_t N = pt_ptr[nA];
  if (N == 0)
    return PDH_OK;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_sol = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(ctx->n_rows_owned, 1) * sizeof(double)));
  double *d_pts = static_cast<double *>(ctx->scratch_get(1, (size_t)N * dim * sizeof(double)));
  int64_t *d_ptr = static_cast<int64_t *>(ctx->scratch_get(2, ((size_t)nA + 1) * sizeof(int64_t)));
  double *d_u = static_cast<double *>(ctx->scratch_get(3, (size_t)N * sizeof(double)));
  double *d_g = grad ? static_cast<double *>(ctx->scratch_get(4, (size_t)N * dim * sizeof(double))) : nullptr;
  if (!d_sol || !d_pts || !d_ptr || !d_u || (grad && !d_g))
    return fail(ctx, PDH_EDEVICE, "pdh_evaluate: out of device memory");
  PDH_HIP(ctx, hipMemcpyAsync(d_sol, solution, ctx->n_rows_owned * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_pts, pts, (size_t)N * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_ptr, pt_ptr, ((size_t)nA + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  const int rc = pdh_evaluate_device(ctx, d_sol, d_ptr, d_pts, N, d_u, d_g);
  if (rc != PDH_OK)
    return rc;
  // only the points of polytopes owned here are produced; the others are left untouched in the caller's arrays
  std::vector<double> hu((size_t)N), hg(grad ? (size_t)N * dim : 0);
  PDH_HIP(ctx, hipMemcpyAsync(hu.data(), d_u, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (grad)
    PDH_HIP(ctx, hipMemcpyAsync(hg.data(), d_g, (size_t)N * dim * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  std::vector<int32_t> own((size_t)ctx->n_owned);
  PDH_HIP(ctx, hipMemcpyAsync(own.data(), ctx->dev.own_agg, own.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
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
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_global_error called before pdh_set_problem");
  if (!d_solution || !d_pt_ptr || !d_pts || !d_w || !d_exact_u || !d_exact_grad || !sums || n_points < 0)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts, w, exact_u, exact_grad and sums are required");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  sums[0] = sums[1] = 0.0;
  if (ctx->n_owned == 0)
    return PDH_OK;
  double *d_err = static_cast<double *>(ctx->scratch_get(5, (size_t)ctx->n_owned * 2 * sizeof(double)));
  if (!d_err)
    return fail(ctx, PDH_EDEVICE, "pdh_global_error: out of device memory");
  PDH_HIP(ctx, pdh_launch_eval_err(ctx->dev.dim, ctx->dev.n1d, &ctx->dev, ctx->n_owned, d_solution, d_pt_ptr, d_pts, n_points, d_w,
                                   d_exact_u, d_exact_grad, d_err, ctx->stream));
  // 16 bytes per polytope come back; they are added in slot order (the result does not depend on the launch)
  std::vector<double> h((size_t)ctx->n_owned * 2);
  PDH_HIP(ctx, hipMemcpyAsync(h.data(), d_err, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int sl = 0; sl < ctx->n_owned; ++sl)
    {
      sums[0] += h[2 * (size_t)sl];
      sums[1] += h[2 * (size_t)sl + 1];
    }
  return PDH_OK;
}

extern "C" int pdh_global_error(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, const double *w,
                                const double *exact_u, const double *exact_grad, double *sums)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_global_error called before pdh_set_problem");
  if (!solution || !pt_ptr || !pts || !w || !exact_u || !exact_grad || !sums)
    return fail(ctx, PDH_EINVAL, "solution, pt_ptr, pts, w, exact_u, exact_grad and sums are required");
  const int nA = ctx->n_agg_total, dim = ctx->dev.dim;
  if (pt_ptr[0] != 0)
    return fail(ctx, PDH_EINVAL, "pt_ptr[0] must be 0");
  for (int a = 0; a < nA; ++a)
    if (pt_ptr[a + 1] < pt_ptr[a])
      return fail(ctx, PDH_EINVAL, "pt_ptr must be non-decreasing");
  const int64_t N = pt_ptr[nA];
  sums[0] = sums[1] = 0.0;
  if (N == 0)
    return PDH_OK;
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_sol = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(ctx->n_rows_owned, 1) * sizeof(double)));
  double *d_pts = static_cast<double *>(ctx->scratch_get(1, (size_t)N * dim * sizeof(double)));
  int64_t *d_ptr = static_cast<int64_t *>(ctx->scratch_get(2, ((size_t)nA + 1) * sizeof(int64_t)));
  double *d_eu = static_cast<double *>(ctx->scratch_get(3, (size_t)N * 2 * sizeof(double))); // exact_u | w
  double *d_eg = static_cast<double *>(ctx->scratch_get(4, (size_t)N * dim * sizeof(double)));
  if (!d_sol || !d_pts || !d_ptr || !d_eu || !d_eg)
    return fail(ctx, PDH_EDEVICE, "pdh_global_error: out of device memory");
  PDH_HIP(ctx, hipMemcpyAsync(d_sol, solution, ctx->n_rows_owned * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_pts, pts, (size_t)N * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_ptr, pt_ptr, ((size_t)nA + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_eu, exact_u, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_eu + N, w, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_eg, exact_grad, (size_t)N * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  return pdh_global_error_device(ctx, d_sol, d_ptr, d_pts, N, d_eu + N, d_eu, d_eg, sums);
}

// ---- basis values on boxes (injection matrices) -----------------------------------------------------------------------
extern "C" int pdh_shape_values_device(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *d_bbox,
                                       const int64_t *d_pt_ptr, const double *d_pts, int64_t n_points, double *d_values)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
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
      if (!ctx->d_shape_midx)
        PDH_HIP(ctx, hipMalloc((void **)&ctx->d_shape_midx, 512 * sizeof(int32_t)));
      PDH_HIP(ctx, hipMemcpy(ctx->d_shape_midx, midx.data(), 512 * sizeof(int32_t), hipMemcpyHostToDevice));
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
  D.midx = ctx->d_shape_midx;
  PDH_HIP(ctx, pdh_launch_shape(dim, n1d, &D, n_boxes, d_pt_ptr, d_pts, n_points, d_values, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_shape_values(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *bbox,
                                const int64_t *pt_ptr, const double *pts, double *values)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
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
  double *d_bbox = static_cast<double *>(ctx->scratch_get(0, (size_t)n_boxes * 2 * dim * sizeof(double)));
  double *d_pts = static_cast<double *>(ctx->scratch_get(1, (size_t)N * dim * sizeof(double)));
  int64_t *d_ptr = static_cast<int64_t *>(ctx->scratch_get(2, ((size_t)n_boxes + 1) * sizeof(int64_t)));
  double *d_out = static_cast<double *>(ctx->scratch_get(3, (size_t)N * n * sizeof(double)));
  if (!d_bbox || !d_pts || !d_ptr || !d_out)
    return fail(ctx, PDH_EDEVICE, "pdh_shape_values: out of device memory");
  PDH_HIP(ctx, hipMemcpyAsync(d_bbox, bbox, (size_t)n_boxes * 2 * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_pts, pts, (size_t)N * dim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_ptr, pt_ptr, ((size_t)n_boxes + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  const int rc = pdh_shape_values_device(ctx, dim, degree, basis, n_boxes, d_bbox, d_ptr, d_pts, N, d_out);
  if (rc != PDH_OK)
    return rc;
  PDH_HIP(ctx, hipMemcpyAsync(values, d_out, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_device_values(pdh_ctx *ctx, double **device_ptr, int64_t *n_values)
{
  if (!ctx || !ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  if (device_ptr)
    *device_ptr = ctx->dev.values;
  if (n_values)
    *n_values = ctx->n_values;
  return PDH_OK;
}

extern "C" int pdh_set_profiling(pdh_ctx *ctx, int enabled)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
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
  if (!ctx || !ctx->has_problem || !mfma_instr)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  mfma_instr[0] = (ctx->use_moment(0) || ctx->use_rows()) ? 0 : ctx->mfma_diag; // counted for the direct form only
  mfma_instr[1] = (ctx->use_moment(1) || ctx->use_rows()) ? 0 : ctx->mfma_offdiag;
  return PDH_OK;
}

extern "C" int pdh_problem_stats(pdh_ctx *ctx, int64_t *stats)
{
  if (!ctx || !ctx->has_problem || !stats)
    return fail(ctx, PDH_ESTATE, "no problem resident");
  stats[0] = ctx->n_owned;
  stats[1] = ctx->n_items;
  stats[2] = ctx->n_vq;
  stats[3] = ctx->n_ap;
  stats[4] = ctx->n_values;
  stats[5] = ctx->dev.n;
  stats[6] = (int64_t)ctx->lds_diag;
  stats[7] = (int64_t)ctx->lds_off;
  return PDH_OK;
}

// ---- solving with the resident matrix (pdh_solve.hip) -----------------------------------------------------------------
static PdhSolveArgs solve_args(const pdh_ctx *ctx)
{
  PdhSolveArgs A;
  A.values = ctx->dev.values;
  A.row_base = ctx->dev.row_base;
  A.row_len = ctx->dev.row_len;
  A.diag_L = ctx->dev.diag_L;
  A.own_row = ctx->dev.own_row;
  A.blk_ptr = ctx->d_blk_ptr;
  A.blk_dof = ctx->d_blk_dof;
  A.n = ctx->dev.n;
  A.diag_first = ctx->dev.diag_first;
  A.n_owned = ctx->n_owned;
  A.max_row_len = ctx->max_row_len;
  return A;
}

static bool overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
  const char *pa = static_cast<const char *>(a), *pb = static_cast<const char *>(b);
  return pa < pb + nb * (int64_t)sizeof(double) && pb < pa + na * (int64_t)sizeof(double);
}

static constexpr int PDH_VMULT_LDS_CAP = 64 * 1024; // column set of one polytope in LDS (8192 columns)

static int vmult_checks(pdh_ctx *ctx, const void *x, const void *y)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_vmult called before pdh_set_problem");
  if (!x || !y)
    return fail(ctx, PDH_EINVAL, "x and y are required");
  if (overlap(x, ctx->n_rows_total, y, ctx->n_rows_owned))
    return fail(ctx, PDH_EINVAL, "x and y overlap");
  if ((int64_t)ctx->max_row_len * (int64_t)sizeof(double) > PDH_VMULT_LDS_CAP)
    return fail(ctx, PDH_EUNSUPPORTED, "a row has more than 8192 entries (the column set of a polytope must fit 64 KB of LDS)");
  return PDH_OK;
}

extern "C" int pdh_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y)
{
  PDH_TRY(vmult_checks(ctx, d_x, d_y));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = solve_args(ctx);
  PDH_HIP(ctx, pdh_launch_vmult(&A, d_x, d_y, nullptr, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_vmult(pdh_ctx *ctx, const double *x, double *y)
{
  PDH_TRY(vmult_checks(ctx, x, y));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double *d_x = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(ctx->n_rows_total, 1) * sizeof(double)));
  double *d_y = static_cast<double *>(ctx->scratch_get(1, std::max<int64_t>(ctx->n_rows_owned, 1) * sizeof(double)));
  if (!d_x || !d_y)
    return fail(ctx, PDH_EDEVICE, "pdh_vmult: out of device memory");
  PDH_HIP(ctx, hipMemcpyAsync(d_x, x, ctx->n_rows_total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_TRY(pdh_vmult_device(ctx, d_x, d_y));
  PDH_HIP(ctx, hipMemcpyAsync(y, d_y, ctx->n_rows_owned * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_setup_preconditioner(pdh_ctx *ctx, int kind)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_setup_preconditioner called before pdh_set_problem");
  if (kind != PDH_PREC_NONE && kind != PDH_PREC_JACOBI && kind != PDH_PREC_BLOCK_JACOBI)
    return fail(ctx, PDH_EINVAL, "kind must be PDH_PREC_NONE, PDH_PREC_JACOBI or PDH_PREC_BLOCK_JACOBI");
  if (kind == PDH_PREC_BLOCK_JACOBI && ctx->dev.n > 64)
    return fail(ctx, PDH_EUNSUPPORTED, "block Jacobi needs at most 64 dofs per polytope (use PDH_PREC_JACOBI)");
  ctx->prec_kind = kind;
  ctx->prec_gen = ctx->values_gen;
  ctx->prec_ok = false; // until the set-up below has succeeded
  if (kind == PDH_PREC_NONE)
    {
      ctx->prec_ok = true;
      return PDH_OK;
    }
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = ctx->dev.n;
  double *dinv = ctx->sol_get<double>(pdh_ctx::SOL_DINV, kind == PDH_PREC_BLOCK_JACOBI ? ctx->n_owned * n * n : ctx->n_rows_owned);
  int32_t *flag = ctx->sol_get<int32_t>(pdh_ctx::SOL_FLAG, ctx->n_owned);
  if (!dinv || !flag)
    return fail(ctx, PDH_EDEVICE, "pdh_setup_preconditioner: out of device memory");
  const PdhSolveArgs A = solve_args(ctx);
  PDH_HIP(ctx, kind == PDH_PREC_BLOCK_JACOBI ? pdh_launch_block_inverse(&A, dinv, flag, ctx->stream)
                                             : pdh_launch_diag_inverse(&A, dinv, flag, ctx->stream));
  std::vector<int32_t> h_flag((size_t)ctx->n_owned);
  if (ctx->n_owned)
    PDH_HIP(ctx, hipMemcpyAsync(h_flag.data(), flag, h_flag.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  PDH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < ctx->n_owned; ++s)
    if (h_flag[s])
      { // slots are in polytope order: the first flagged slot is the lowest polytope number
        int32_t agg = -1;
        PDH_HIP(ctx, hipMemcpy(&agg, ctx->dev.own_agg + s, sizeof(int32_t), hipMemcpyDeviceToHost));
        return fail(ctx, PDH_EINVAL,
                    kind == PDH_PREC_BLOCK_JACOBI
                      ? "block Jacobi: the diagonal block of polytope " + std::to_string(agg) + " is not positive definite"
                      : "Jacobi: a diagonal entry of polytope " + std::to_string(agg) + " is zero or not finite");
      }
  ctx->prec_ok = true;
  return PDH_OK;
}

static int prec_checks(pdh_ctx *ctx)
{
  if (ctx->prec_kind != PDH_PREC_NONE && (!ctx->prec_ok || ctx->prec_gen != ctx->values_gen))
    return fail(ctx, PDH_ESTATE, ctx->prec_ok ? "the values changed since pdh_setup_preconditioner: set it up again"
                                              : "the last pdh_setup_preconditioner failed");
  return PDH_OK;
}

// One application of the Chebyshev polynomial to b, queued on the stream: x <- x + p(P^-1 A) P^-1 (b - A x) (zero: x <- p(..) P^-1 b,
// x not read).  d, r and q are the context's own vectors - never CG's residual.  rcg / part: see pdh_launch_cheb_update.
static int cheb_apply(pdh_ctx *ctx, const PdhSolveArgs &A, const double *b, double *x, bool zero, const double *rcg, double *part)
{
  double *d = static_cast<double *>(ctx->sol[pdh_ctx::SOL_CHEB_D].p), *r = static_cast<double *>(ctx->sol[pdh_ctx::SOL_CHEB_R].p);
  double *q = static_cast<double *>(ctx->sol[pdh_ctx::SOL_Q].p);
  const double *dinv = static_cast<const double *>(ctx->sol[pdh_ctx::SOL_DINV].p);
  const int m = (int)ctx->cheb_c2.size();
  if (!d || !r || !q || !dinv || m < 1)
    return fail(ctx, PDH_ESTATE, "the Chebyshev preconditioner is not set up");
  if (!zero)
    PDH_HIP(ctx, pdh_launch_vmult(&A, x, q, nullptr, ctx->stream));
  for (int k = 0; k < m; ++k)
    {
      if (k > 0)
        PDH_HIP(ctx, pdh_launch_vmult(&A, d, q, nullptr, ctx->stream));
      PDH_HIP(ctx, pdh_launch_cheb_update(&A, k == 0, ctx->cheb_inner, dinv, b, (k == 0 && zero) ? nullptr : q, d, r, x, ctx->cheb_c1[k],
                                          ctx->cheb_c2[k], k == 0 && zero, k == m - 1 ? rcg : nullptr, part, ctx->stream));
    }
  return PDH_OK;
}

extern "C" int pdh_precondition_device(pdh_ctx *ctx, const double *d_r, double *d_z)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_precondition_device called before pdh_set_problem");
  if (!d_r || !d_z)
    return fail(ctx, PDH_EINVAL, "r and z are required");
  PDH_TRY(prec_checks(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const PdhSolveArgs A = solve_args(ctx);
  if (ctx->prec_kind == PDH_PREC_CHEBYSHEV)
    return cheb_apply(ctx, A, d_r, d_z, true, nullptr, nullptr);
  PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_APPLY, ctx->prec_kind, static_cast<const double *>(ctx->sol[pdh_ctx::SOL_DINV].p),
                                    nullptr, nullptr, nullptr, nullptr, const_cast<double *>(d_r), d_z, nullptr, nullptr, ctx->stream));
  return PDH_OK;
}

extern "C" int pdh_solve_cg_device(pdh_ctx *ctx, const pdh_cg_control *c, const double *d_b, double *d_x, pdh_cg_result *res)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_solve_cg called before pdh_set_problem");
  if (!c || !d_b || !d_x || !res)
    return fail(ctx, PDH_EINVAL, "control, b, x and result are required");
  if (c->max_iter < 0 || !(c->rel_tol >= 0.0) || !(c->abs_tol >= 0.0))
    return fail(ctx, PDH_EINVAL, "max_iter, rel_tol and abs_tol must be non-negative");
  if (ctx->problem_ghost)
    return fail(ctx, PDH_EUNSUPPORTED, "pdh_solve_cg: the problem was set in PDH_EXCHANGE_GHOST mode; the solver runs on a context that "
                                       "owns all rows with PDH_EXCHANGE_NONE (no distributed Krylov solver)");
  if (ctx->n_rows_owned != ctx->n_rows_total)
    return fail(ctx, PDH_EUNSUPPORTED, "pdh_solve_cg: the context owns rows " + std::to_string(ctx->n_rows_owned) + " of " +
                                         std::to_string(ctx->n_rows_total) + "; the solver needs all rows in one context (no distributed "
                                                                             "Krylov solver)");
  if (overlap(d_b, ctx->n_rows_total, d_x, ctx->n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  PDH_TRY(prec_checks(ctx));
  if ((int64_t)ctx->max_row_len * (int64_t)sizeof(double) > PDH_VMULT_LDS_CAP)
    return fail(ctx, PDH_EUNSUPPORTED, "a row has more than 8192 entries (the column set of a polytope must fit 64 KB of LDS)");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = ctx->n_rows_owned;
  double *r = ctx->sol_get<double>(pdh_ctx::SOL_R, N), *z = ctx->sol_get<double>(pdh_ctx::SOL_Z, N);
  double *p = ctx->sol_get<double>(pdh_ctx::SOL_P, N), *q = ctx->sol_get<double>(pdh_ctx::SOL_Q, N);
  double *part = ctx->sol_get<double>(pdh_ctx::SOL_PART, (size_t)PDH_CG_NPART * ctx->n_owned);
  double *scal = ctx->sol_get<double>(pdh_ctx::SOL_SCAL, PDH_CG_NSCALARS);
  if (!ctx->pinned && hipHostMalloc((void **)&ctx->pinned, PDH_CG_NSCALARS * sizeof(double), hipHostMallocDefault) != hipSuccess)
    ctx->pinned = nullptr;
  if (!r || !z || !p || !q || !part || !scal || !ctx->pinned)
    return fail(ctx, PDH_EDEVICE, "pdh_solve_cg: out of device memory");
  const double *dinv = static_cast<const double *>(ctx->sol[pdh_ctx::SOL_DINV].p);
  // Chebyshev: the fused update leaves z alone (kind none) and the chain z = p(P^-1 A) P^-1 r follows it; its last step writes the
  // partials of r^T z
  const bool cheb = ctx->prec_kind == PDH_PREC_CHEBYSHEV;
  const int kind = cheb ? PDH_PREC_NONE : ctx->prec_kind;
  const PdhSolveArgs A = solve_args(ctx);
  hipStream_t st = ctx->stream;
  // r = b - A x0, z = P^-1 r, p = z
  PDH_HIP(ctx, pdh_launch_vmult(&A, d_x, q, nullptr, st));
  PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_INIT, kind, dinv, d_b, q, nullptr, nullptr, r, z, scal, part, st));
  if (cheb)
    PDH_TRY(cheb_apply(ctx, A, r, z, true, r, part));
  PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 0, scal, st));
  PDH_HIP(ctx, pdh_launch_cg_direction(N, 1, z, p, scal, st));
  PDH_HIP(ctx, hipMemcpyAsync(ctx->pinned, scal + PDH_CG_RR, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  PDH_HIP(ctx, hipStreamSynchronize(st));
  double rr = ctx->pinned[0];
  const double bnorm = std::sqrt(ctx->pinned[1]);
  const double stop = std::max(c->abs_tol, c->rel_tol * bnorm);
  res->residual0 = std::sqrt(rr);
  int it = 0;
  // the loop of examples/host_solver.h: test, then q = A p, alpha, x and r, z, beta, p.  Only ||r||^2 crosses PCIe (8 bytes, pinned).
  for (; it < c->max_iter && std::sqrt(rr) > stop; ++it)
    {
      PDH_HIP(ctx, pdh_launch_vmult(&A, p, q, part + (size_t)PDH_PART_PQ * ctx->n_owned, st));
      PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 1, scal, st));
      PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_STEP, kind, dinv, nullptr, q, p, d_x, r, z, scal, part, st));
      if (cheb)
        PDH_TRY(cheb_apply(ctx, A, r, z, true, r, part));
      PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 2, scal, st));
      PDH_HIP(ctx, pdh_launch_cg_direction(N, 0, z, p, scal, st));
      PDH_HIP(ctx, hipMemcpyAsync(ctx->pinned, scal + PDH_CG_RR, sizeof(double), hipMemcpyDeviceToHost, st));
      PDH_HIP(ctx, hipStreamSynchronize(st));
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
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_solve_cg called before pdh_set_problem");
  if (!b || !x)
    return fail(ctx, PDH_EINVAL, "b and x are required");
  if (overlap(b, ctx->n_rows_total, x, ctx->n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t N = ctx->n_rows_total;
  double *d_b = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(N, 1) * sizeof(double)));
  double *d_x = static_cast<double *>(ctx->scratch_get(1, std::max<int64_t>(N, 1) * sizeof(double)));
  if (!d_b || !d_x)
    return fail(ctx, PDH_EDEVICE, "pdh_solve_cg: out of device memory");
  PDH_HIP(ctx, hipMemcpyAsync(d_b, b, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PDH_HIP(ctx, hipMemcpyAsync(d_x, x, N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
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
static int all_rows_checks(pdh_ctx *ctx, const char *who)
{
  if (ctx->problem_ghost)
    return fail(ctx, PDH_EUNSUPPORTED, std::string(who) + ": the problem was set in PDH_EXCHANGE_GHOST mode; it needs a context that owns "
                                                          "all rows with PDH_EXCHANGE_NONE");
  if (ctx->n_rows_owned != ctx->n_rows_total)
    return fail(ctx, PDH_EUNSUPPORTED, std::string(who) + ": the context owns rows " + std::to_string(ctx->n_rows_owned) + " of " +
                                         std::to_string(ctx->n_rows_total) + "; it needs all rows in one context");
  if ((int64_t)ctx->max_row_len * (int64_t)sizeof(double) > PDH_VMULT_LDS_CAP)
    return fail(ctx, PDH_EUNSUPPORTED, "a row has more than 8192 entries (the column set of a polytope must fit 64 KB of LDS)");
  return PDH_OK;
}

// Largest Ritz value of P^-1 A after k steps of P-preconditioned CG on A x = b0 from x = 0 (P = the inner preconditioner, set up and
// current): the launches of pdh_solve_cg_device, but alpha_j, beta_j and ||r||^2 come back every step - a path of its own, the
// solver's loop keeps reading 8 bytes.  steps: CG steps that entered the Lanczos matrix.
static int cheb_estimate(pdh_ctx *ctx, int kind, int k, double *est, int *steps)
{
  const int64_t N = ctx->n_rows_owned;
  double *r = ctx->sol_get<double>(pdh_ctx::SOL_R, N), *z = ctx->sol_get<double>(pdh_ctx::SOL_Z, N);
  double *p = ctx->sol_get<double>(pdh_ctx::SOL_P, N), *q = ctx->sol_get<double>(pdh_ctx::SOL_Q, N);
  double *part = ctx->sol_get<double>(pdh_ctx::SOL_PART, (size_t)PDH_CG_NPART * ctx->n_owned);
  double *scal = ctx->sol_get<double>(pdh_ctx::SOL_SCAL, PDH_CG_NSCALARS);
  double *d_b = static_cast<double *>(ctx->scratch_get(0, std::max<int64_t>(N, 1) * sizeof(double)));
  double *d_x = static_cast<double *>(ctx->scratch_get(1, std::max<int64_t>(N, 1) * sizeof(double)));
  if (!ctx->pinned && hipHostMalloc((void **)&ctx->pinned, PDH_CG_NSCALARS * sizeof(double), hipHostMallocDefault) != hipSuccess)
    ctx->pinned = nullptr;
  if (!r || !z || !p || !q || !part || !scal || !d_b || !d_x || !ctx->pinned)
    return fail(ctx, PDH_EDEVICE, "pdh_setup_chebyshev: out of device memory");
  std::vector<double> b0((size_t)N);
  for (int64_t i = 0; i < N; ++i)
    b0[(size_t)i] = (double)(uint32_t)(2654435761ull * (uint64_t)i) / 4294967296.0 - 0.5;
  hipStream_t st = ctx->stream;
  const double *dinv = static_cast<const double *>(ctx->sol[pdh_ctx::SOL_DINV].p);
  const PdhSolveArgs A = solve_args(ctx);
  PDH_HIP(ctx, hipMemcpyAsync(d_b, b0.data(), N * sizeof(double), hipMemcpyHostToDevice, st));
  PDH_HIP(ctx, hipMemsetAsync(d_x, 0, N * sizeof(double), st));
  PDH_HIP(ctx, pdh_launch_vmult(&A, d_x, q, nullptr, st));
  PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_INIT, kind, dinv, d_b, q, nullptr, nullptr, r, z, scal, part, st));
  PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 0, scal, st));
  PDH_HIP(ctx, pdh_launch_cg_direction(N, 1, z, p, scal, st));
  PDH_HIP(ctx, hipMemcpyAsync(ctx->pinned, scal, PDH_CG_NSCALARS * sizeof(double), hipMemcpyDeviceToHost, st));
  PDH_HIP(ctx, hipStreamSynchronize(st));
  double rr = ctx->pinned[PDH_CG_RR];
  std::vector<double> alpha, beta;
  for (int it = 0; it < k && rr > 0.0; ++it)
    {
      PDH_HIP(ctx, pdh_launch_vmult(&A, p, q, part + (size_t)PDH_PART_PQ * ctx->n_owned, st));
      PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 1, scal, st));
      PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_STEP, kind, dinv, nullptr, q, p, d_x, r, z, scal, part, st));
      PDH_HIP(ctx, pdh_launch_cg_finalise(part, ctx->n_owned, 2, scal, st));
      PDH_HIP(ctx, pdh_launch_cg_direction(N, 0, z, p, scal, st));
      PDH_HIP(ctx, hipMemcpyAsync(ctx->pinned, scal, PDH_CG_NSCALARS * sizeof(double), hipMemcpyDeviceToHost, st));
      PDH_HIP(ctx, hipStreamSynchronize(st));
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
  std::vector<double> dg((size_t)m), od((size_t)std::max(m - 1, 1));
  for (int j = 0; j < m; ++j)
    {
      dg[j] = j == 0 ? 1.0 / alpha[j] : 1.0 / alpha[j] + beta[j - 1] / alpha[j - 1];
      if (j + 1 < m)
        od[j] = std::sqrt(beta[j]) / alpha[j];
    }
  double lo = 0.0, hi = 0.0;
  if (pdh_tridiagonal_eigenvalues(m, dg.data(), od.data(), &lo, &hi) != PDH_OK)
    return fail(ctx, PDH_EINVAL, std::string("pdh_setup_chebyshev: ") + pdh_last_error(nullptr));
  *est = hi;
  *steps = m;
  return PDH_OK;
}

extern "C" int pdh_setup_chebyshev(pdh_ctx *ctx, const pdh_chebyshev_control *c, pdh_chebyshev_info *info)
{
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_setup_chebyshev called before pdh_set_problem");
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
  PDH_TRY(all_rows_checks(ctx, "pdh_setup_chebyshev"));
  PDH_TRY(pdh_setup_preconditioner(ctx, c->inner)); // the inner inverse; prec_kind = inner for the estimate
  ctx->prec_ok = false;                             // until the whole set-up has succeeded
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  double est = c->max_eigenvalue;
  int steps = 0;
  if (!given)
    PDH_TRY(cheb_estimate(ctx, c->inner, c->eig_cg_n_iterations, &est, &steps));
  if (!(est > 0.0) || !std::isfinite(est))
    return fail(ctx, PDH_EINVAL, "pdh_setup_chebyshev: the eigenvalue estimate " + std::to_string(est) + " is not positive");
  const int64_t N = ctx->n_rows_owned;
  if (!ctx->sol_get<double>(pdh_ctx::SOL_CHEB_D, N) || !ctx->sol_get<double>(pdh_ctx::SOL_CHEB_R, N) ||
      !ctx->sol_get<double>(pdh_ctx::SOL_Q, N))
    return fail(ctx, PDH_EDEVICE, "pdh_setup_chebyshev: out of device memory");
  const double hi = 1.2 * est, lo = hi / c->smoothing_range;
  const double theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta;
  ctx->cheb_c1.assign((size_t)c->degree, 0.0);
  ctx->cheb_c2.assign((size_t)c->degree, 0.0);
  ctx->cheb_c2[0] = 1 / theta;
  double rho_old = 1 / sigma;
  for (int k = 1; k < c->degree; ++k)
    {
      const double rho = 1 / (2 * sigma - rho_old);
      ctx->cheb_c1[k] = rho * rho_old;
      ctx->cheb_c2[k] = 2 * rho / delta;
      rho_old = rho;
    }
  ctx->cheb_inner = c->inner;
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
  if (!ctx)
    return fail(nullptr, PDH_EINVAL, "ctx is NULL");
  if (!ctx->has_problem)
    return fail(ctx, PDH_ESTATE, "pdh_chebyshev_step_device called before pdh_set_problem");
  if (!d_b || !d_x)
    return fail(ctx, PDH_EINVAL, "b and x are required");
  if (overlap(d_b, ctx->n_rows_total, d_x, ctx->n_rows_total))
    return fail(ctx, PDH_EINVAL, "b and x overlap");
  if (ctx->prec_kind != PDH_PREC_CHEBYSHEV)
    return fail(ctx, PDH_ESTATE, "pdh_chebyshev_step_device: the preconditioner set up last is not PDH_PREC_CHEBYSHEV");
  PDH_TRY(prec_checks(ctx));
  PDH_HIP(ctx, hipSetDevice(ctx->device));
  return cheb_apply(ctx, solve_args(ctx), d_b, d_x, zero_initial_guess != 0, nullptr, nullptr);
}
