// pdh_launch.h — the one declaration of every kernel launcher of the library.  Included by the driver units, which call them, and by
// every .hip file that defines one: extern "C" links a mismatch silently, this way a changed signature does not compile.
// The assembly kernels are launched in two steps.  pdh_set_problem* RESOLVES every form the resident problem can be asked for - each
// instantiating unit runs its family's ladder once, takes the address of the instantiation and sizes the grid - into PdhLaunch records;
// pdh_assemble_device LAUNCHES the records it selects through the unit's typed launch function.  Neither step keeps state of its own:
// what a resolver needs beyond the problem (the diagnostic switches, the device's CU count) set-up hands to it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pdh_dev.h"
#include "pdh_rows_tables.h"
#include "pdh_solve.h"
#include "pdh_terms_tables.h"

struct PdhTransferArgs;  // pdh_transfer.h
struct PdhPTransferArgs; // pdh_ptransfer.h
struct PdhGalerkinArgs; // pdh_galerkin.h

// One resolved launch (host only).  kernel: host stub of the instantiation, NULL where nothing could be resolved (no such instantiation,
// a grid beyond 2^31 - 1 blocks) - launching that answers hipErrorInvalidValue; grid 0: nothing to do, a successful no-op.
struct PdhLaunch
{
  const void *kernel;
  unsigned grid, block;
  size_t lds; // dynamic LDS, bytes
};

// The parameter list of every instantiation of a family.  A resolver converts each kernel it offers to its family's type and a launch
// function builds the arguments from that type, so a kernel whose signature changed compiles in neither.
typedef void (*PdhDirectKernel)(PdhDev, int);                             // pdh_kernels.h: k_diag, k_offdiag
typedef void (*PdhTiledKernel)(PdhDev, int, int);                         // pdh_tiled.h: k_tdiag, k_toffdiag
typedef void (*PdhMomentKernel)(PdhDev, const double *, int);             // pdh_moment.h: k_mdiag, k_moffdiag
typedef void (*PdhRowsKernel)(PdhDev, PdhRows, const double *, int);      // pdh_rows.h: k_rows
typedef void (*PdhTermsKernel)(PdhDev, PdhTerms, int);                    // pdh_terms.h: k_terms, pdh_terms_wg.h: k_terms_wg

template <class... A>
inline PdhLaunch pdh_record(void (*kernel)(A...), long long grid, unsigned block, size_t lds)
{
  return grid > 0x7fffffffLL ? PdhLaunch{} : PdhLaunch{(const void *)kernel, (unsigned)(grid > 0 ? grid : 0), block, lds};
}
template <class... A>
inline hipError_t pdh_launch_as(void (*)(A...), const PdhLaunch &L, hipStream_t stream, A... a)
{
  if (!L.kernel)
    return hipErrorInvalidValue;
  if (!L.grid)
    return hipSuccess;
  void *args[] = {&a...};
  (void)hipLaunchKernel(L.kernel, dim3(L.grid), dim3(L.block), args, L.lds, stream);
  return hipGetLastError();
}
// f(std::bool_constant<b>{}...) for run-time bools: a family's ladder over its bool template arguments, written once
template <class F>
inline void pdh_for_bools(F &&f)
{
  f();
}
template <class F, class... B>
inline void pdh_for_bools(F &&f, bool b, B... rest)
{
  if (b)
    pdh_for_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else
    pdh_for_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

extern "C" {
// pdh_inst.hip, one translation unit per group of pdh_combos.h: L[0] own blocks (reaction: with reaction term), L[1] coupling blocks; the
// launch function is the same for every group (pdh_tiled.hip, next to that of the tiled form)
typedef void (*pdh_resolve_fn)(int dim, int n1d, int nt, int lb, bool reaction, int n_own, int n_items, PdhLaunch *L);
#define PDH_DECL(g) void pdh_resolve_g##g(int, int, int, int, bool, int, int, PdhLaunch *);
PDH_DECL(0) PDH_DECL(1) PDH_DECL(2) PDH_DECL(3) PDH_DECL(4) PDH_DECL(5) PDH_DECL(6) PDH_DECL(7)
#undef PDH_DECL
hipError_t pdh_launch_direct(const PdhLaunch *L, const PdhDev *P, int count, hipStream_t stream);

// pdh_rhs.hip
hipError_t pdh_launch_rhs(int dim, int n1d, const PdhDev *P, int count, const double *f_vol, const double *g_face, double *rhs,
                          const int64_t *vq_src, const int64_t *ap_src, const int64_t *bd_rng, hipStream_t stream);

// pdh_eval.hip
hipError_t pdh_launch_eval(int dim, int n1d, int grad, const PdhDev *P, int count, const double *coef, const int64_t *pt_ptr,
                           const double *pts, int64_t pts_stride, double *out_u, double *out_g, int by_agg, hipStream_t stream);
hipError_t pdh_launch_shape(int dim, int n1d, const PdhDev *P, int n_boxes, const int64_t *pt_ptr, const double *pts,
                            int64_t pts_stride, double *out, hipStream_t stream);
hipError_t pdh_launch_eval_err(int dim, int n1d, const PdhDev *P, int count, const double *coef, const int64_t *pt_ptr,
                               const double *pts, int64_t pts_stride, const double *w, const double *exact_u, const double *exact_g,
                               double *err, hipStream_t stream);

// pdh_moment.hip: the moment form (L[0] diagonal, L[1] coupling blocks) and the kinds of pdh_rows.h.  The row kernel's grid
// is min(count, cus x waves per CU), the waves per CU the smaller of what fits by LDS and the occupancy query unless waves_per_cu > 0
// says otherwise; lds_pad: extra dynamic LDS, bytes (PlanSwitches); verbose: one line on stderr
void pdh_resolve_moment(int n1d, int n, int n_own, int n_items, PdhLaunch *L);
hipError_t pdh_launch_moment(const PdhLaunch *L, const PdhDev *P, const double *mtab, int count, hipStream_t stream);
// zero_sched (resolved with the kind): PdhRows::sched is zeroed, stream-ordered, in front of every launch
PdhLaunch pdh_resolve_rows(const PdhDev *P, const PdhRows *R, int count, int cus, int waves_per_cu, size_t lds_pad, bool verbose,
                           bool *zero_sched);
hipError_t pdh_launch_rows(const PdhLaunch *L, bool zero_sched, const PdhDev *P, const PdhRows *R, const double *mtab, int count,
                           hipStream_t stream);

// pdh_terms.hip; FE_DGQ(3) kernel: wg_waves: writer waves of a workgroup, 4 | 8; its grid is min(count, cus), or, wg_batch > 0,
// ceil(count / wg_batch) workgroups (PlanSwitches).  Nothing is resolved (kernel NULL) where that kernel would not be alone on its CU:
// *why (never NULL) names the reason, and set-up fails with it.  Launches of one problem share its work counter: one stream, in order.
// store_aux, drain: how that kernel's writers store (pdh_terms_tables.h: WG_STORE_AUX, WG_DRAIN are what set-up asks for and all the
// library instantiates; -DPDHT_VARIANTS builds resolve the other policies for pdh_debug_terms_wg_variant)
PdhLaunch pdh_resolve_terms(const PdhDev *P, const PdhTerms *T, int count, int cus, int wg_waves, int wg_batch, int store_aux, int drain,
                            const char **why);
hipError_t pdh_launch_terms(const PdhLaunch *L, const PdhDev *P, const PdhTerms *T, int count, hipStream_t stream);
hipError_t pdh_launch_terms_gather(const PdhDev *P, const PdhTerms *T, double *out, int count, hipStream_t stream);

// pdh_matfree.hip (3-D, n1d 2 .. 4, a problem whose plan built the term tables).  tables: the finished 1-D tables of every owned polytope,
// count * pdht::matfree_rec_doubles doubles; hipErrorInvalidValue: no such kind
hipError_t pdh_launch_mf_tables(const PdhDev *P, const PdhTerms *T, double *tables, int count, hipStream_t stream);
// y[own rows] = A x from the tables, with the vectors and the partial of pdh_launch_vmult
hipError_t pdh_launch_mf_vmult(const PdhSolveArgs *A, int n1d, const PdhTerms *T, const double *tables, const double *x, double *y,
                               double *part, hipStream_t stream);

// pdh_tiled.hip: L[0] own blocks, symmetric tiles ti == tj, L[1] coupling blocks, L[2] own blocks, pairs ti < tj (none of the own
// blocks resolves if one of the two grids is too large)
void pdh_resolve_tiled(int dim, int n1d, int n, bool reaction, int n_own, int n_items, PdhLaunch *L);
hipError_t pdh_launch_tiled(const PdhLaunch *L, const PdhDev *P, int count, hipStream_t stream);

// pdh_cartgen.hip
hipError_t pdh_launch_gen_volume(int nq, const double *nodes, const double *weights, const double *d_box, const int32_t *d_gcell,
                                 int64_t n_points, double *vq_x, int64_t stride, double *vq_w, hipStream_t stream);
hipError_t pdh_launch_gen_faces(int nqf, const double *nodes, const double *weights, const double *d_box, const int32_t *d_cell,
                                const int32_t *d_face, int64_t n_points, double *fq_x, double *fq_n, double *fq_w, hipStream_t stream);

// pdh_exchange.hip
hipError_t pdh_launch_pack_faces(int dim, int64_t nqf, const double *fq_x, const double *fq_n, const double *fq_w,
                                 const double *fq_w_out, int64_t n_runs, const int64_t *pk_at, const int64_t *pk_fq,
                                 const int32_t *pk_cnt, const int32_t *pk_flags, const double *pk_sig, int64_t nap, double *ap_x,
                                 double *ap_n, double *ap_wself, double *ap_wcross, double *ap_sig, hipStream_t stream);
hipError_t pdh_launch_ghost_apply(const PdhDev *P, const double *recv, int n_r21, const int64_t *r21_src, const int64_t *r21_dst,
                                  const int32_t *r21_rlen, int n_r22, const int64_t *r22_ptr, const int64_t *r22_src,
                                  const int32_t *r22_slot, hipStream_t stream);
// d_out [pdh_checksum_doubles()]: the four results, then scratch for the workgroups' partials (summed in a fixed order: reproducible bits)
size_t pdh_checksum_doubles();
hipError_t pdh_launch_checksum(const double *values, int64_t n, double *d_out, hipStream_t stream);

// pdh_solve.hip
// y[own rows] = A x (x in the global dof numbering).  part (may be NULL): per slot, sum_i y_i x_i over the slot's own rows.
hipError_t pdh_launch_vmult(const PdhSolveArgs *A, const double *x, double *y, double *part, hipStream_t stream);
// inverses of the n x n diagonal blocks (n <= 64) into dinv [n_owned][n][n]; flag[s] = 1 where the block is not positive definite
hipError_t pdh_launch_block_inverse(const PdhSolveArgs *A, double *dinv, int32_t *flag, hipStream_t stream);
// inverse of the diagonal into dinv [n_owned * n]; flag[s] = 1 where a diagonal entry of the slot is zero or not finite
hipError_t pdh_launch_diag_inverse(const PdhSolveArgs *A, double *dinv, int32_t *flag, hipStream_t stream);
// the fused vector kernel (PdhCgMode; kind = PDH_PREC_*); vectors indexed by owned row
hipError_t pdh_launch_cg_update(const PdhSolveArgs *A, int mode, int kind, const double *dinv, const double *b, const double *q,
                                const double *p, double *x, double *r, double *z, const double *scal, double *part, hipStream_t stream);
// one step of the Chebyshev chain (pdh_setup_chebyshev; kind = PDH_PREC_JACOBI | PDH_PREC_BLOCK_JACOBI): r = first ? b (- q if q) : r - q,
// d = first ? c2 P^-1 r : c1 d + c2 P^-1 r, x = (first && zero_start) ? d : x + d; rcg (may be NULL): partial of rcg^T x to PDH_PART_RZ
hipError_t pdh_launch_cheb_update(const PdhSolveArgs *A, int first, int kind, const double *dinv, const double *b, const double *q,
                                  double *d, double *r, double *x, double c1, double c2, int zero_start, const double *rcg, double *part,
                                  hipStream_t stream);
// p = z + beta p (init: p = z) over n_rows entries
hipError_t pdh_launch_cg_direction(int64_t n_rows, int init, const double *z, double *p, const double *scal, hipStream_t stream);
// one workgroup: partials -> scalars.  stage 0: rz, rr, bb;  1: pq, alpha;  2: rz, rr, beta
hipError_t pdh_launch_cg_finalise(const double *part, int n_owned, int stage, double *scal, hipStream_t stream);
// its two halves, for sums that are added over several ranks in between: partials -> sums [3] of this rank (the stage's, the rest 0);
// the reduced sums -> scalars
hipError_t pdh_launch_cg_local_sum(const double *part, int n_owned, int stage, double *sums, hipStream_t stream);
hipError_t pdh_launch_cg_finish(int stage, const double *sums, double *scal, hipStream_t stream);

// pdh_dist.hip
// send [n_blocks][n] = the blocks of n doubles at v + src[b]: whole blocks, contiguous within a block
hipError_t pdh_launch_halo_pack(int n, int64_t n_blocks, const int64_t *src, const double *v, double *send, hipStream_t stream);
// y = A v for the rows of the slots listed (k_vmult's arithmetic).  A->blk_dof holds LOCAL positions: v is a rank's local vector.
// part (may be NULL): per slot LISTED, sum_i y_i v_i over the slot's own rows, at part[slot]
hipError_t pdh_launch_vmult_local(const PdhSolveArgs *A, const int32_t *slots, int n_slots, const double *v, double *y, double *part,
                                  hipStream_t stream);

// pdh_dense.hip (pdh_dense.h: ld = pdh_dense_ld(n_rows), 1 <= n_rows <= PDH_DENSE_MAX_ROWS, else hipErrorInvalidValue)
// D [ld][ld] (zeroed by the caller) = the resident rows, dense
hipError_t pdh_launch_dense_gather(const PdhSolveArgs *A, double *D, int ld, int n_rows, hipStream_t stream);
// Cholesky in the upper triangle of U = D, diagonal of L to dg [ld]; piv [2]: smallest / largest pivot, flag [1]: 0 or 1 + the row whose
// pivot is <= 0 or not finite
hipError_t pdh_launch_dense_cholesky(double *U, int ld, int n_rows, double *dg, double *piv, int32_t *flag, hipStream_t stream);
// Wd [ld][ld] = L^-1, then G [ld][ld] = Wd^T Wd, exactly symmetric
hipError_t pdh_launch_dense_inverse(const double *U, const double *dg, int ld, int n_rows, double *Wd, double *G, hipStream_t stream);
// z = G r over the owned rows (r and z disjoint); rcg (may be NULL): partial of rcg^T z to PDH_PART_RZ
hipError_t pdh_launch_dense_symv(const PdhSolveArgs *A, const double *G, int ld, int n_rows, const double *r, double *z,
                                 const double *rcg, double *part, hipStream_t stream);

// pdh_transfer.hip (dim 2 | 3, n1d 2 .. 8; add: accumulate into the destination)
// fine (+)= P coarse: one wave per max(1, 64 / n) fine polytopes
hipError_t pdh_launch_prolongate(int dim, int n1d, int add, const PdhTransferArgs *A, const double *coarse, double *fine, hipStream_t stream);
// coarse (+)= P^T fine: one wave per max(1, 64 / n) coarse polytopes, children in CSR order
hipError_t pdh_launch_restrict(int dim, int n1d, int add, const PdhTransferArgs *A, const double *fine, double *coarse, hipStream_t stream);
// r = b - r over n_rows entries (r holds A x)
hipError_t pdh_launch_residual_sub(int64_t n_rows, const double *b, double *r, hipStream_t stream);

// pdh_ptransfer.hip (dim 2 | 3; dgq: FE_DGQ by sum factorisation with A->nf1d 3 .. 8 > A->nc1d >= 2, else FE_AggloDGP by A->map / A->inv;
// restriction: dst = coarse (+)= P^T src, else dst = fine (+)= P src; add: accumulate): one wave per max(1, 64 / n_f) polytopes
hipError_t pdh_launch_ptransfer(int dim, int dgq, int restriction, int add, const PdhPTransferArgs *A, const double *src, double *dst,
                                hipStream_t stream);

// pdh_galerkin.hip (dim 2, n1d 2 .. 8 | dim 3, n1d 2 .. 4: at most 64 dofs per polytope)
// coarse values = P^T (fine values) P: one wave per coarse block, its fine blocks in plan order
hipError_t pdh_launch_galerkin(int dim, int n1d, const PdhGalerkinArgs *A, hipStream_t stream);
}
