// pdh_ctx.h — internal to the device driver (pdh_capi.cpp, pdh_capi_vectors.cpp, pdh_capi_solve.cpp, pdh_capi_dist.cpp, pdh_capi_matfree.cpp, pdh_capi_transfer.cpp,
// pdh_capi_mg.cpp), not
// installed: the context
// behind the opaque pdh_ctx of include/polydeal_hip.h, error reporting, the one device-buffer type, the alloc / upload helpers of
// set-up and the entry guards.  No kernel header here: pdh_launch.h brings the kernels' argument structs and the launch records.
#pragma once
#include "../../include/polydeal_hip.h"
#include "pdh_launch.h"
#include "pdh_plan.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

// Grow-only device memory, freed with its owner.  Two policies, fixed per buffer: `exact` takes the size asked for (the solver's
// vectors, sized once per problem), `slack` a quarter more (the staging copies of the host-pointer entry points, whose sizes
// creep from call to call - no hipMalloc per call).  get() returns NULL when the device has no memory left.
class DevBuf
{
public:
  enum Policy { exact, slack };
  DevBuf() = default;
  explicit DevBuf(Policy p) : policy(p) {}
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    release();
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevBuf() { release(); }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T *get(size_t count) // at least `count` elements (at least one); the contents do not survive growth
  {
    const size_t need = std::max<size_t>(count, 1) * sizeof(T);
    if (need > bytes)
      {
        release();
        const size_t want = policy == slack ? need + need / 4 + 256 : need;
        if (hipMalloc(&p, want) != hipSuccess)
          {
            p = nullptr;
            return nullptr;
          }
        bytes = want;
      }
    return static_cast<T *>(p);
  }
  template <class T>
  T *ptr() const // as it stands (NULL: never sized)
  {
    return static_cast<T *>(p);
  }

private:
  Policy policy = exact;
  void *p = nullptr;
  size_t bytes = 0;
};

struct pdh_ctx
{
  // ---- what lives as long as the context ----
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr; // stream = the one in use (own_stream unless pdh_set_stream)
  std::string err;
  // The two kernels of a step write disjoint values and have complementary bottlenecks (the diagonal items compute, the
  // coupling items mostly store): on large problems they run concurrently, the coupling kernel on stream2, forked from /
  // joined into `stream` by events so that the caller still sees one ordered stream.  Measured -4 % per step.
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int overlap = 1;                           // pdh_set_overlap
  int algorithm = PDH_ALG_AUTO;              // pdh_set_algorithm: the caller's choice (moment form: 3-D bases of degree <= 3)
  int exchange_mode = PDH_EXCHANGE_NONE;     // pdh_set_exchange_mode: takes effect at the next pdh_set_problem*
  bool profiling = false;
  std::vector<hipEvent_t> events; // 4 per profiled launch: before / after the diagonal kernel, before / after the coupling kernel
  size_t ev_used = 0;
  // a generation of the values (bumped by every set_problem / assemble / exchange_apply, across problems) against which the
  // preconditioner set up last is checked; the caller's choice of it outlives a problem so that solving after a new
  // pdh_set_problem answers "set it up again" (its data - Problem::Solver - does not)
  uint64_t values_gen = 0, prec_gen = 0;
  uint64_t problem_epoch = 0; // counts the pdh_set_problem* calls: what a cached plan of two contexts' problems is checked against
  int prec_kind = PDH_PREC_NONE;
  bool prec_ok = true;
  // prec_epoch counts the set-up calls (a pdh_mg records it per level: the same kind set up again on the same values is a change too);
  // mg: the V-cycle attached as PDH_PREC_MULTIGRID (pdh_capi_mg.cpp), mg_gone: it was destroyed and nothing was set up since
  uint64_t prec_epoch = 0;
  struct pdh_mg *mg = nullptr;
  bool mg_gone = false;
  // staging copies of the host-pointer entry points, shared by all of them: in0 f_vol / solution / bbox / x / b, in1 g_bdry / pts /
  // y / x, ptr pt_ptr (pdh_assemble_rhs: the rhs), out u / exact_u | w / shape values, grad grad / exact_grad, err the error sums
  struct Io
  {
    DevBuf in0{DevBuf::slack}, in1{DevBuf::slack}, ptr{DevBuf::slack}, out{DevBuf::slack}, grad{DevBuf::slack}, err{DevBuf::slack};
  } io;
  int shape_key = -1; // cached multi-index table of pdh_shape_values (per dim / degree / basis)
  DevBuf shape_midx;
  DevBuf checksum;          // the four doubles of pdh_values_checksum, then its workgroups' partials
  double *pinned = nullptr; // [PDH_CG_NSCALARS] the word the CG loop reads its residual through

  // ---- what lives as long as the resident problem: free_problem() assigns a fresh one ----
  struct Problem
  {
    bool resident = false;
    std::vector<void *> allocs; // every hipMalloc of set-up (upload / device_buffer); the pointers below point into these
    PdhDev dev{};
    int n_owned = 0, n_items = 0, NT = 0;
    bool tiled = false; // n > 64 dofs per polytope: pdh_tiled.h instead of the kernels of pdh_inst.hip
    // The launches of every form pdh_set_algorithm can ask of this problem, resolved once at set-up (pdh_launch.h): the direct form
    // ([0] own blocks, [1] coupling blocks, tiled: [2] the tile pairs of the own blocks), the moment form where d_mtab exists, the row
    // kernel of row_kernel.  pdh_assemble_device selects among them (use_rows, use_moment) and launches.
    PdhLaunch direct[3] = {}, moment[2] = {}, row = {};
    bool row_zero_sched = false; // pdh_rows.h, FE_DGQ(3) kind: its work counter is zeroed in front of every launch
    int64_t terms_merge[4] = {0, 0, 0, 0}; // term kernels: cells before / after merging, sub-faces before / after
    int64_t n_values = 0, n_vq = 0, n_ap = 0;
    int64_t mfma_diag = 0, mfma_offdiag = 0; // MFMA instructions per launch
    int basis = 0;
    const double *d_mtab = nullptr; // moment tables (pdh_moment.h)
    int64_t n_rows_owned = 0, n_rows_total = 0;
    int32_t n_agg_total = 0;
    // right-hand side: host-side runs of the packed face points and, on the device, the first caller volume point of every slot,
    // the caller face point of every packed face point (-1: not on the boundary; built at the first call, ensure_ap_src), the
    // packed boundary points [n_owned][2] of every slot; sizes of the caller's point arrays
    struct FaceRun { int64_t ap_begin, fq_begin; int32_t count; int32_t boundary; int32_t slot; };
    std::vector<FaceRun> face_runs;
    const int64_t *d_vq_src = nullptr, *d_ap_src = nullptr, *d_bd_rng = nullptr;
    int64_t n_vq_caller = 0, n_fq_caller = 0;
    // Cartesian description: local face of every sub-face and points per direction (the generated face points run the lower
    // tangential axis fastest, the caller's g_bdry is in QProjector's order - they differ on faces of axis 1: ensure_ap_src)
    std::vector<int32_t> cart_fq_face;
    int cart_nqf = 0;
    // ghost-block exchange variant; n_diag_slots = n_owned + pseudo slots of the outgoing M22 sums
    bool ghost = false;
    int n_diag_slots = 0, n_r21 = 0, n_r22 = 0;
    int64_t n_send = 0, n_recv = 0;
    std::vector<int64_t> send_count, recv_count;
    const int64_t *d_r21_src = nullptr, *d_r21_dst = nullptr, *d_r22_ptr = nullptr, *d_r22_src = nullptr;
    const int32_t *d_r21_rlen = nullptr, *d_r22_slot = nullptr;
    // The row kernel of the problem, if any (set_problem builds the device state of that one only): pdh_rows.h where every face
    // of every owned polytope is a union of axis-aligned planes; the term kernel (pdh_terms.h) on agglomerates of Cartesian cells
    // with tensor rules - any number of planes per neighbour - is taken instead wherever its tables fit the LDS budget.
    RowKernel row_kernel = RowKernel::none;
    PdhRows rows{};
    PdhTerms terms{};
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
    // solving with the resident matrix (pdh_solve.hip): first global dof of every block of every owned slot in value order, the
    // longest row; the solver's vectors, sized at first use; PDH_PREC_CHEBYSHEV: the inner kind whose inverse lies in dinv and,
    // per step k, the factors of d_(k-1) and of P^-1 r_k in d_k (step 0: unused and 1 / theta)
    const int64_t *d_blk_ptr = nullptr;
    const int32_t *d_blk_dof = nullptr;
    int max_row_len = 0;
    // host copies of the block lists and of the first dof of every owned slot's polytope, for the planner of the Galerkin product
    // (pdh_galerkin.h); has_values: the values were written at least once (pdh_assemble_device, pdh_galerkin_device)
    std::vector<int64_t> h_blk_ptr;
    std::vector<int32_t> h_blk_dof, h_slot_dof;
    bool has_values = false;
    bool galerkin_values = false; // ... last by pdh_galerkin_device: they are not the SIP assembly of this description
    // pdh_setup_matrix_free (pdh_matfree.h): the finished 1-D tables of every owned polytope (in `allocs`), valid for the life of the
    // problem; why_terms: what the planner said where it built no term tables
    const double *d_mf_tables = nullptr;
    int64_t mf_table_bytes = 0;
    std::string why_terms;
    struct Solver
    {
      DevBuf dinv, flag, r, z, p, q, part, scal, cheb_d, cheb_r;
      int cheb_inner = PDH_PREC_NONE;
      std::vector<double> cheb_c1, cheb_c2;
      // PDH_PREC_DIRECT (pdh_dense.h): the inverse G [dense_ld][dense_ld] of the dense_n rows; dense_tmp: the copy of r of the in-place
      // apply
      DevBuf dense_g, dense_tmp;
      int dense_ld = 0, dense_n = 0;
      // pdh_set_smoother_precision (pdh_shadow.h): the float32 rows, their per-slot bases (they follow the pattern: computed once per
      // problem) and the float32 block inverses, grow-only; f32: the smoother and the V-cycle residual of this context read them
      DevBuf sh_values, sh_base, sh_dinv;
      int64_t sh_count = 0; // entries of sh_values once sh_base is filled, 0 before
      bool f32 = false;
      bool matrix_free = false; // pdh_set_smoother_operator: the same products apply the operator from d_mf_tables
    } sol;
    // pdh_halo_setup (pdh_dist.h): the plan of the local vector's halo on the device - the block lists with local positions, the
    // sources of the send buffer's blocks, the three slot lists one after the other (all, interior, boundary) - and the send buffer
    // of pdh_dcg_*; dcg: the open run of pdh_dcg_begin (pdh_capi_dist.cpp).  All of it goes with the problem.
    struct Halo
    {
      bool ready = false;
      int n_ranks = 0, n_interior = 0, n_boundary = 0;
      int64_t n_owned_rows = 0, n_ghost_rows = 0, n_send = 0, n_recv = 0;
      DevBuf blk_loc, pack_src, slots, send, red;
    } halo;
    std::shared_ptr<struct PdhDcgRun> dcg;
  } prob;

  // AUTO takes the row kernel where it applies (degree 1 since 12 waves per CU are resident: 0.21 vs 0.24-0.30 ms)
  bool use_rows() const
  {
    return prob.row_kernel != RowKernel::none && (algorithm == PDH_ALG_AUTO || algorithm == PDH_ALG_ROWS);
  }
  // which form each of the two launches uses: [0] diagonal blocks, [1] coupling blocks
  bool use_moment(int kind) const
  {
    if (!prob.d_mtab || algorithm == PDH_ALG_DIRECT)
      return false;
    if (algorithm == PDH_ALG_MOMENT)
      return true;
    if (algorithm == PDH_ALG_ROWS)
      return false;
    // auto: where the moment form was measured faster than the MFMA contraction (profiles/README.md): FE_DGQ(3) both
    // kinds (8.5 -> 4.7 ms), FE_DGQ(2) the diagonal blocks only (BASELINE configs[3]: 9.7 -> 5.6 ms; its coupling blocks
    // 4.3 ms direct vs 6.4 ms moment)
    if (prob.basis != PDH_BASIS_DGQ)
      return false;
    return prob.dev.n1d == 4 || (prob.dev.n1d == 3 && kind == 0);
  }
  // (two streams pay for their fork / join events only when the kernels run for a while: by the size of the matrix)
  static constexpr int64_t small_values = 16 << 20;
  bool overlapped() const
  {
    return overlap && stream2 && (int64_t)prob.n_diag_slots + prob.n_items >= 8192 && prob.n_values >= small_values;
  }
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

static inline int fail(pdh_ctx *ctx, int code, const std::string &msg)
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

// ---- entry guards: `name` is what the entry point prints (the *_device variants print their host-pointer sibling's) ----
static inline int need_ctx(pdh_ctx *ctx) { return ctx ? PDH_OK : fail(nullptr, PDH_EINVAL, "ctx is NULL"); }
static inline int need_problem(pdh_ctx *ctx, const char *name)
{
  PDH_TRY(need_ctx(ctx));
  return ctx->prob.resident ? PDH_OK : fail(ctx, PDH_ESTATE, std::string(name) + " called before pdh_set_problem");
}
// the entry points that answer a NULL context and a missing problem alike
static inline bool resident(const pdh_ctx *ctx) { return ctx && ctx->prob.resident; }

// ---- staging of the host-pointer entry points: `who` names the entry point in "<who>: out of device memory" ----
template <class T>
static int stage(pdh_ctx *ctx, const char *who, DevBuf &buf, size_t count, T **d)
{
  *d = buf.get<T>(count);
  return *d ? PDH_OK : fail(ctx, PDH_EDEVICE, std::string(who) + ": out of device memory");
}
// ... and the copy of `count` elements of the caller's into it, queued on the context's stream (room: elements to make room for)
template <class T>
static int stage_in(pdh_ctx *ctx, const char *who, DevBuf &buf, const T *host, size_t count, T **d, size_t room = 0)
{
  PDH_TRY(stage(ctx, who, buf, std::max(count, room), d));
  const hipError_t e = hipMemcpyAsync(*d, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
  return e == hipSuccess ? PDH_OK : fail(ctx, PDH_EDEVICE, std::string(who) + ": copy to the device: " + hipGetErrorString(e));
}

// ---- device memory of set-up ----
// `count` elements (at least one), recorded in `owner` - Problem::allocs for the resident problem (freed by free_problem),
// Staging::bufs for the inputs of one set-up step; PDH_EDEVICE says what failed
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
  return alloc_in(ctx, ctx->prob.allocs, count, dptr, what);
}
template <class T>
static int upload(pdh_ctx *ctx, const T *h, size_t count, const T **dptr, const char *what)
{
  return upload_in(ctx, ctx->prob.allocs, h, count, dptr, what);
}
template <class V>
static int upload(pdh_ctx *ctx, const V &h, const typename V::value_type **dptr, const char *what)
{
  return upload_in(ctx, ctx->prob.allocs, h.data(), h.size(), dptr, what);
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

// ---- what the driver units call of each other ----
// pdh_capi_solve.cpp.  The launch helpers take the stream they queue on: the context's own for its entry points, the finest level's
// for every level of a V-cycle.
PdhSolveArgs pdh_solve_args(const pdh_ctx *ctx);
// the guard of the products: a problem resident (`name` in the message), x [n_rows_total] and y [owned rows] given and disjoint
int pdh_vmult_vectors_check(pdh_ctx *ctx, const char *name, const void *x, const void *y);
// PDH_ESTATE on `ctx` unless the preconditioner set up last is current for the values as they stand (what pdh_solve_cg* asks first)
int pdh_prec_checks(pdh_ctx *ctx);
int pdh_row_fits_lds(pdh_ctx *ctx); // PDH_EUNSUPPORTED on `ctx`: a row of more than 8192 entries (k_vmult keeps a column set in LDS)
// One application of the Chebyshev polynomial of `ctx` to b: x <- x + p(P^-1 A) P^-1 (b - A x) (zero: x <- p(..) P^-1 b, x not read).
// rcg / part: see pdh_launch_cheb_update.  Errors are reported on `report`.
int pdh_cheb_apply(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *b, double *x, bool zero, const double *rcg, double *part,
                   hipStream_t stream);
// y = A x as the smoother of `ctx` sees A: from the term tables while PDH_SMOOTHER_OP_MATRIX_FREE is in force, else the float32 shadow
// while PDH_SMOOTHER_F32 is, else pdh_launch_vmult
int pdh_smoother_vmult(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *x, double *y, hipStream_t stream);
// z = P^-1 r with the preconditioner of `ctx` as set up - any kind but PDH_PREC_MULTIGRID, r and z disjoint - without the state checks
int pdh_prec_apply(pdh_ctx *ctx, pdh_ctx *report, const PdhSolveArgs &A, const double *r, double *z, const double *rcg, double *part,
                   hipStream_t stream);
// pdh_capi_transfer.cpp
void pdh_transfer_info(const pdh_transfer *t, pdh_ctx **ctx, int64_t *n_fine_rows, int64_t *n_coarse_rows);
hipError_t pdh_transfer_launch(const pdh_transfer *t, bool restriction, int add, const double *src, double *dst, hipStream_t stream);
// pdh_capi_mg.cpp: the V-cycle attached to a finest context.  pdh_mg_checks: PDH_ESTATE naming the level whose values or
// preconditioner changed since pdh_mg_create; pdh_mg_cycle: one cycle queued on the finest context's stream, no checks (rcg / part: the
// last post-smoothing update on the finest level writes the partials of rcg^T x); pdh_mg_detach: the context's set-up calls and
// pdh_destroy let go of an attached mg.
int pdh_mg_checks(pdh_mg *mg);
int pdh_mg_cycle(pdh_mg *mg, const double *b, double *x, bool zero, const double *rcg, double *part);
void pdh_mg_detach(pdh_ctx *ctx);
