// pdh_launch.h — the one declaration of every kernel launcher of the library.  Included by pdh_capi.cpp, which calls them,
// and by every .hip file that defines one: extern "C" links a mismatch silently, this way a changed signature does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pdh_dev.h"
#include "pdh_rows_tables.h"
#include "pdh_solve.h"
#include "pdh_terms_tables.h"

extern "C" {
// pdh_inst.hip, one translation unit per group of pdh_combos.h: which = 0 diagonal blocks, 1 coupling blocks, 2 diagonal blocks
// with reaction term
typedef hipError_t (*pdh_launch_fn)(int dim, int n1d, int nt, int lb, int which, const PdhDev *P, int count, size_t lds,
                                    hipStream_t stream);
#define PDH_DECL(g) hipError_t pdh_launch_g##g(int, int, int, int, int, const PdhDev *, int, size_t, hipStream_t);
PDH_DECL(0) PDH_DECL(1) PDH_DECL(2) PDH_DECL(3) PDH_DECL(4) PDH_DECL(5) PDH_DECL(6) PDH_DECL(7)
#undef PDH_DECL

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

// pdh_moment.hip: the moment form (which = 0 diagonal blocks, 1 coupling blocks) and the kinds of pdh_rows.h
hipError_t pdh_launch_moment(int n1d, int which, const PdhDev *P, const double *mtab, int count, hipStream_t stream);
hipError_t pdh_launch_rows(const PdhDev *P, const PdhRows *R, const double *mtab, int count, hipStream_t stream);

// pdh_terms.hip
hipError_t pdh_launch_terms(const PdhDev *P, const PdhTerms *T, int count, hipStream_t stream);
hipError_t pdh_launch_terms_gather(const PdhDev *P, const PdhTerms *T, double *out, int count, hipStream_t stream);

// pdh_tiled.hip: which = 0 own blocks, 2 own blocks with reaction term, 1 coupling blocks
hipError_t pdh_launch_tiled(int dim, int n1d, int which, const PdhDev *P, int count, hipStream_t stream);

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
hipError_t pdh_launch_checksum(const double *values, int64_t n, double *d_out4, hipStream_t stream);

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
}
