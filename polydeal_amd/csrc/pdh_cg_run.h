// pdh_cg_run.h — the ONE preconditioned CG recurrence of the driver, shared by pdh_solve_cg* and the eigenvalue estimate of the Chebyshev
// set-up (pdh_capi_solve.cpp) and by CG over several ranks (pdh_capi_dist.cpp).  Internal to the driver like pdh_ctx.h.
#pragma once
#include "pdh_ctx.h"

// The recurrence on the resident matrix, queued on the context's stream: the loop of examples/host_solver.h (q = A p, alpha, x and r,
// z, beta, p) with every scalar kept on the device.  After each of start() / step() `n_scalars` doubles from scal[first_scalar] are in
// ctx->pinned and the stream is idle - what they are and what follows from them is the caller's.
// kind: the preconditioner of the fused update; chain: an application z = M r queued after it instead (kind none leaves z alone) -
// the Chebyshev chain p(P^-1 A) P^-1, the dense inverse or the V-cycle attached to the context - whose last kernel writes the partials
// of r^T z.
// start() and step() are made of the pieces below them.  A run over several ranks queues the same pieces with its own products
// (on the local vector p, n_ghost entries longer than the owned rows) and, where one rank turns partials into scalars in one kernel
// (finalise), puts the caller's all-reduce between the two halves of that kernel: local_sum into `red`, finish from `red`.
struct CgRun
{
  pdh_ctx *ctx;
  const PdhSolveArgs A;
  const int kind;
  const int chain; // PDH_PREC_NONE (no chain) | PDH_PREC_CHEBYSHEV | PDH_PREC_DIRECT | PDH_PREC_MULTIGRID
  const int64_t N;
  const int n_owned;
  hipStream_t st;
  double *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *part = nullptr, *scal = nullptr;
  const double *dinv = nullptr;

  CgRun(pdh_ctx *c, int kind_, int chain_, int64_t n_ghost = 0)
    : ctx(c), A(pdh_solve_args(c)), kind(kind_), chain(chain_), N(c->prob.n_rows_owned), n_owned(c->prob.n_owned), st(c->stream)
  {
    pdh_ctx::Problem::Solver &S = c->prob.sol;
    r = S.r.get<double>(N), z = S.z.get<double>(N), p = S.p.get<double>(N + n_ghost), q = S.q.get<double>(N);
    part = S.part.get<double>((size_t)PDH_CG_NPART * n_owned);
    scal = S.scal.get<double>(PDH_CG_NSCALARS);
    if (!c->pinned && hipHostMalloc((void **)&c->pinned, PDH_CG_NSCALARS * sizeof(double), hipHostMallocDefault) != hipSuccess)
      c->pinned = nullptr;
    dinv = S.dinv.ptr<double>();
  }
  bool ok() const { return r && z && p && q && part && scal && ctx->pinned; }
  int apply_chain()
  {
    if (chain == PDH_PREC_MULTIGRID)
      return pdh_mg_cycle(ctx->mg, r, z, true, r, part);
    return chain == PDH_PREC_NONE ? PDH_OK : pdh_prec_apply(ctx, ctx, A, r, z, r, part, st);
  }
  int read_back(int first_scalar, int n_scalars)
  {
    PDH_HIP(ctx, hipMemcpyAsync(ctx->pinned, scal + first_scalar, n_scalars * sizeof(double), hipMemcpyDeviceToHost, st));
    PDH_HIP(ctx, hipStreamSynchronize(st));
    return PDH_OK;
  }
  // ---- the pieces ----
  double *pq_part() const { return part + (size_t)PDH_PART_PQ * n_owned; }
  // q = A x is in place: r = b - q, z = M r; partials of r^T z, r^T r, b^T b
  int first_residual(const double *b)
  {
    PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_INIT, kind, dinv, b, q, nullptr, nullptr, r, z, scal, part, st));
    return apply_chain();
  }
  // q = A p and alpha are in place: x += alpha p, r -= alpha q, z = M r; partials of r^T z, r^T r
  int update(double *x)
  {
    PDH_HIP(ctx, pdh_launch_cg_update(&A, PDH_UPD_STEP, kind, dinv, nullptr, q, p, x, r, z, scal, part, st));
    return apply_chain();
  }
  // p = z (init) or z + beta p, over the owned rows
  int direction(int init)
  {
    PDH_HIP(ctx, pdh_launch_cg_direction(N, init, z, p, scal, st));
    return PDH_OK;
  }
  // partials -> scalars of a stage (0: rz, rr, bb; 1: pq, alpha; 2: rz, rr, beta), in one kernel ...
  int finalise(int stage)
  {
    PDH_HIP(ctx, pdh_launch_cg_finalise(part, n_owned, stage, scal, st));
    return PDH_OK;
  }
  // ... or in its two halves around a sum over the ranks
  int local_sum(int stage, double *red)
  {
    PDH_HIP(ctx, pdh_launch_cg_local_sum(part, n_owned, stage, red, st));
    return PDH_OK;
  }
  int finish(int stage, const double *red)
  {
    PDH_HIP(ctx, pdh_launch_cg_finish(stage, red, scal, st));
    return PDH_OK;
  }
  // ---- one rank that owns all rows ----
  // r = b - A x, z = P^-1 r, p = z
  int start(const double *b, const double *x, int first_scalar, int n_scalars)
  {
    PDH_HIP(ctx, pdh_launch_vmult(&A, x, q, nullptr, st));
    PDH_TRY(first_residual(b));
    PDH_TRY(finalise(0));
    PDH_TRY(direction(1));
    return read_back(first_scalar, n_scalars);
  }
  int step(double *x, int first_scalar, int n_scalars)
  {
    PDH_HIP(ctx, pdh_launch_vmult(&A, p, q, pq_part(), st));
    PDH_TRY(finalise(1));
    PDH_TRY(update(x));
    PDH_TRY(finalise(2));
    PDH_TRY(direction(0));
    return read_back(first_scalar, n_scalars);
  }
};
