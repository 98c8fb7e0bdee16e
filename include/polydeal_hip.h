/* polydeal_hip.h — C ABI of the MI355X (gfx950) SIP assembly path.
 *
 * This is the drop-in boundary for ONE hot path of polyDEAL: the DG/SIP system-matrix assembly
 * over agglomerated polytopal elements, i.e. what
 *
 *   PolyUtils::assemble_dg_matrix(MatrixType&, const FiniteElement<dim>&, const AgglomerationHandler<dim>&)
 *       reference include/poly_utils.h:2000-2195
 *   and the hand-written loops of examples/poisson.cc:694-988, examples/minimal_SIP.cc:143-365,
 *   examples/diffusion_reaction.cc:420-696
 *
 * do on the CPU through AgglomerationHandler::reinit / reinit_interface
 * (reference source/agglomeration_handler.cc:729-906, 1103-1243), MappingBox
 * (source/mapping_box.cc:393-531) and FE_DGQ / FE_AggloDGP (source/fe_agglodgp.cc:27-55).
 *
 * The reference has no FFI layer (it is a set of C++ templates over deal.II types); the entry
 * points below are what a deal.II-side adapter binds (INTEGRATION.md shows it).  Plain pointers and
 * sizes only, no exceptions cross the boundary: every function returns 0 on success or a negative
 * PDH_E* code, and pdh_last_error() gives the message.  One pdh_ctx per device and per host thread
 * (not re-entrant, like the reference's handler: include/agglomeration_handler.h:834-851).
 *
 * All arithmetic is fp64.  Indices are 32-bit except CSR row pointers / point offsets (64-bit).
 */
#ifndef POLYDEAL_HIP_H
#define POLYDEAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDH_BASIS_DGQ 0      /* FE_DGQ<dim>(p): tensor Lagrange on Gauss-Lobatto nodes, (p+1)^dim dofs   */
#define PDH_BASIS_AGGLODGP 1 /* FE_AggloDGP<dim>(p): Legendre P_p, C(p+dim,dim) dofs (fe_agglodgp.cc:27) */

#define PDH_OK 0
#define PDH_EINVAL -1     /* malformed problem description                */
#define PDH_EUNSUPPORTED -2 /* valid but outside what the kernels implement */
#define PDH_EDEVICE -3    /* HIP runtime error (no GPU, OOM, launch failure) */
#define PDH_ESTATE -4     /* call order (e.g. assemble before set_problem)  */
#define PDH_ENOCONV -5    /* iterative solver hit max_iter; x holds the last iterate */

typedef struct pdh_ctx pdh_ctx; /* opaque; owns all device memory */

/* Flattened description of one agglomerated mesh + SIP variant.  All pointers are caller-owned host
 * memory, read-only, and need to stay valid only for the duration of the call they are passed to.
 * Letters in brackets refer to SURVEY.md section 8(a).                                            */
typedef struct pdh_problem
{
  int32_t dim;     /* 2 or 3                                                                       */
  int32_t degree;  /* polynomial degree p, 0 .. 7.  Polytopes of up to 64 dofs run one wavefront per
                      block; more (3-D only: FE_DGQ(4..7), FE_AggloDGP(6, 7)) in 64 x 64 tiles
                      (pdh_tiled.h; owner-computes-rows only, no ghost-block exchange)             */
  int32_t basis;   /* PDH_BASIS_*                                                                  */
  int32_t n_agg;   /* number of polytopes (agglomerates) in this description                       */
  int32_t n_faces; /* polytopal faces; each interior face stored ONCE (in/out), boundary: out = -1 */
  int32_t n_rows;  /* GLOBAL number of dofs (= n_dofs_per_cell * n_agg for a global description)   */
  int32_t diag_first; /* 1: deal.II SparsityPattern row layout (diagonal first, then ascending);
                         0: plain ascending columns (Epetra local CSR)                       [A4] */
  int32_t local;   /* 0: GLOBAL description - all polytopes, rowptr [n_rows+1] over all rows.
                      1: RANK-LOCAL description, what an MPI rank of the reference holds
                         (source/agglomeration_handler.cc:1026-1091: locally owned polytopes + the ghost
                         polytopes across its partition boundary, with their bounding boxes and GLOBAL dof
                         indices).  Polytopes are numbered locally 0..n_agg-1: the owned ones - exactly those
                         whose dof_offset lies in [row_begin,row_end) - and at least every neighbour of an owned
                         one.  dof_offset holds GLOBAL dof numbers; ghosts need bbox and dof_offset only (their
                         volume range may be empty); every face with an owned side must be listed, with the
                         quadrature data of side 0 as always; faces between two ghosts are ignored.
                         rowptr has row_end - row_begin + 1 entries (owned rows only, rowptr[0] = 0), colind
                         - if given - global column numbers of those rows.                              */
  double reaction_c; /* adds c * phi_i phi_j to the volume term (diffusion_reaction.cc:495-501)    */

  const double  *bbox;       /* [n_agg][2][dim] lower, upper corner of the bounding box      [A1] */
  const int32_t *dof_offset; /* [n_agg] first global dof of each polytope                    [A2] */

  const int64_t *vq_ptr; /* [n_agg+1] CSR offsets into the volume quadrature arrays           [A5] */
  const double  *vq_x;   /* [dim][Nq_tot] REAL quadrature points (structure of arrays)             */
  const double  *vq_w;   /* [Nq_tot] JxW of the sub-cell rules (agglomeration_handler.cc:639-653)  */

  const int32_t *face_in;  /* [n_faces] polytope on side 0                                    [A3] */
  const int32_t *face_out; /* [n_faces] polytope on side 1, or -1 on the domain boundary           */
  const int64_t *fq_ptr;   /* [n_faces+1] CSR offsets into the face quadrature arrays         [A8] */
  const double  *fq_x;     /* [dim][Nqf_tot] REAL points                                           */
  const double  *fq_n;     /* [dim][Nqf_tot] outward unit normal of side 0 (poly_utils.h:1881)     */
  const double  *fq_w;     /* [Nqf_tot] JxW seen from side 0                                       */
  const double  *fq_w_out; /* [Nqf_tot] JxW seen from side 1, or NULL if identical     */
  const double  *face_sigma; /* [n_faces] penalty sigma = C / h_f, resolved per caller variant     */

  const int64_t *rowptr; /* [n_rows+1] (local: [row_end-row_begin+1]) target CSR row pointers    [A4] */
  const int32_t *colind; /* [nnz] target CSR columns, or NULL: canonical DG block pattern assumed  */

  /* Optional (NULL = dof_offset): column number of the first dof of every polytope in the numbering that ORDERS the
   * entries of a row.  An Epetra_CrsMatrix row is sorted by LOCAL column id, and the column map lists the owned
   * columns first and the ghost columns after them, so on rank > 0 a ghost block with a smaller global number sits
   * BEHIND the owned blocks of the row (TrilinosWrappers::SparseMatrix, reference examples/diffusion_reaction.cc:
   * 448-466).  With col_offset = local column ids the values come out in exactly that order (colind, if given, is
   * then checked against these numbers).  Requires diag_first = 0.                                              */
  const int32_t *col_offset;
  /* Optional: owning rank of every polytope (the calling rank's own number for the owned ones).  Needed only by the
   * ghost-block exchange variant (pdh_set_exchange_mode), which ships the M21/M22 blocks of the faces cut by the
   * partition to the rank that owns their rows (reference include/poly_utils.h:1930-1992, 2134-2194).             */
  const int32_t *agg_rank;
  /* Structure of the volume rules.  The volume points of every polytope may come in consecutive groups of
   * vq_tensor_n^dim points, each group a tensor-product rule on an axis-aligned box, first index fastest:
   *   x_(i,j,k) = (X_i, Y_j, Z_k),  JxW_(i,j,k) = a_i b_j c_k        (QGauss<dim>(n) on Cartesian sub-cells,
   *   source/agglomeration_handler.cc:639-653 with MappingCartesian-like cells).
   * > 0: a claim, which pdh_set_problem VERIFIES on the points (a few ulp); 0: pdh_set_problem finds out by itself
   * (n = 8 .. 2 are tried; a candidate that does not hold fails on the first group); < 0: do not look.  Where the
   * structure holds for all owned polytopes the row kernel integrates the volume moments cell by cell in factorised form
   * (3 n sums instead of n^3 points).  A wrong claim is harmless: the check fails and the general path is taken.   */
  int32_t vq_tensor_n;
  /* The same for the face points: groups of fq_tensor_n^(dim-1) points, each a tensor rule on an axis-aligned rectangle
   * (either tangential direction may run fastest).  Verified on the points like vq_tensor_n.                        */
  int32_t fq_tensor_n;
} pdh_problem;

/* Lifetime -------------------------------------------------------------------------------------- */
int pdh_create(pdh_ctx **out, int device_id);
void pdh_destroy(pdh_ctx *ctx);
const char *pdh_last_error(const pdh_ctx *ctx); /* valid until the next call on ctx; ctx may be NULL */

/* Setup: validates the description, derives the per-polytope block positions inside the CSR rows and
 * uploads the repacked tables to HBM.  Plays the role of the caches AgglomerationHandler builds in
 * distribute_agglomerated_dofs / initialize_fe_values (agglomeration_handler.cc:210-236, 326-379).
 * [row_begin,row_end) selects the dof rows this context owns (multi-GPU: one contiguous range per
 * rank, whole polytopes only, like the reference asserts at agglomeration_handler.cc:83-87).     */
/* With problem->local = 1 the description itself is rank-local (owned + ghost polytopes, global dof numbers): a
 * rank never needs the global mesh.  With local = 0 every rank passes the same global description and its range. */
int pdh_set_problem(pdh_ctx *ctx, const pdh_problem *problem);
int pdh_set_problem_local(pdh_ctx *ctx, const pdh_problem *problem, int32_t row_begin, int32_t row_end);

/* Set-up from a COMPACT description of agglomerates of CARTESIAN cells: the quadrature data of the problem are generated ON THE
 * DEVICE instead of being gathered on the host and uploaded.  The reference gathers them per polytope inside the span it times
 * (source/agglomeration_handler.cc:622-707 agglomerated_quadrature, :1103-1243 reinit_master; examples/poisson.cc:1099-1106); for
 * sub-cells that are axis-aligned boxes with QGauss rules - every BASELINE configuration but the piston mesh - a group of nq^3
 * volume points is a function of its cell's box, a group of nqf^2 face points of its cell's box and local face number.
 *   problem : as for pdh_set_problem_local (global or rank-local), with vq_x, vq_w, fq_x, fq_n, fq_w, fq_w_out = NULL; dim = 3;
 *             vq_ptr / fq_ptr count points as always (nq^3 per sub-cell, nqf^2 per sub-face); vq_tensor_n / fq_tensor_n ignored
 *   points  : where the points come from.  Volume group g (the g-th group of nq^3 points in the order of vq_ptr) is QGauss<3>(nq)
 *             on cell vq_cell[g] (x fastest); face group s (order of fq_ptr) is QGauss<2>(nqf) on local face fq_face[s] (deal.II
 *             numbering 2 * axis + side) of cell fq_cell[s] - the sub-cell on side 0 of the polytopal face, whose outward normal
 *             is the face's normal (reference include/poly_utils.h:1881) - lower tangential axis fastest.  g_bdry of
 *             pdh_assemble_rhs is sampled as for the equivalent points description: QProjector's order, tangential axes
 *             (y, z), (z, x), (x, y) for faces of axis 0, 1, 2, the first fastest.
 * The generated arrays are exactly what the caller would have passed (to rounding of lo + h * xi), so everything downstream is
 * unchanged; the assembly runs through the term kernels (PDH_ROWS_TERMS: a problem whose polytopes are too large for them is
 * refused with PDH_EUNSUPPORTED - describe it with points then).                                                              */
typedef struct pdh_cartesian_points
{
  int32_t n_cells;          /* cells of the background grid referred to below                                   */
  const double *cell_box;   /* [n_cells][2][3] lower, upper corner                                              */
  const int32_t *vq_cell;   /* [vq_ptr[n_agg] / nq^3] cell of every group of volume points                      */
  const int32_t *fq_cell;   /* [fq_ptr[n_faces] / nqf^2] side-0 cell of every sub-face                          */
  const int32_t *fq_face;   /* [same] its local face number 0 .. 5                                              */
  int32_t nq, nqf;          /* points per direction of the cell / face rule (1 .. 8)                            */
} pdh_cartesian_points;
int pdh_set_problem_cartesian(pdh_ctx *ctx, const pdh_problem *problem, const pdh_cartesian_points *points, int32_t row_begin,
                              int32_t row_end);

/* The hot path.  Replaces the body of assemble_dg_matrix (poly_utils.h:2034-2193): volume term,
 * boundary (Nitsche) term and the four interface blocks, written straight into CSR value order.
 *   pdh_assemble_device : values stay in HBM (pointer from pdh_device_values); asynchronous on the
 *                         context's stream; nothing crosses PCIe.
 *   pdh_assemble        : same + copy of the owned rows' values into `values`
 *                         (length rowptr[row_end]-rowptr[row_begin]); overwrites, does not add.
 *   pdh_assemble_sip    : set_problem + assemble in one call (all rows).                           */
int pdh_assemble_device(pdh_ctx *ctx);
int pdh_assemble(pdh_ctx *ctx, double *values);
int pdh_assemble_sip(pdh_ctx *ctx, const pdh_problem *problem, double *values);
int pdh_assemble_sip_local(pdh_ctx *ctx, const pdh_problem *problem, int32_t row_begin, int32_t row_end,
                           double *values);

/* Right-hand side of the SIP Poisson problem for the resident problem, i.e. what the
 * callers assemble in the same loops as the matrix (examples/poisson.cc:745-759, 788-828):
 *   rhs_i(P) = sum_q phi_i f(x_q) JxW  +  sum_{q on boundary faces} (sigma g phi_i - grad phi_i . n g) JxW
 * f_vol : [Nq_tot]  f sampled at the volume quadrature points, in the order of vq_x; NULL = no volume term
 * g_bdry: [Nqf_tot] Dirichlet datum sampled at the face quadrature points, in the order of fq_x (only the
 *         entries of boundary faces are read); NULL = homogeneous
 * rhs   : [row_end-row_begin] host output for the owned rows, overwritten.  Rows are in dof order.      */
int pdh_assemble_rhs(pdh_ctx *ctx, const double *f_vol, const double *g_bdry, double *rhs);

/* Evaluation of a polytopal DG function at caller-given points: the device part of
 * PolyUtils::interpolate_to_fine_grid (include/poly_utils.h:1145-1274: points = support points of the sub-cells)
 * and PolyUtils::compute_global_error (:1686-1731: points = quadrature points; the JxW-weighted sums stay with the
 * caller).  solution: coefficients of the owned rows [row_end-row_begin]; pt_ptr [n_agg+1]: CSR offsets of the
 * points of every polytope; pts [dim][N] real coordinates; u [N] (required) and grad [dim][N] (may be NULL) receive
 * u_h and grad u_h at the points of the polytopes owned by this context (others are left untouched).        */
int pdh_evaluate(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, double *u, double *grad);

/* Values of all basis functions of a set of bounding boxes at caller-given points - the local matrices of
 * Utils::fill_injection_matrix (include/utils.h:219-229: local_matrix(i,j) = fe.shape_value(j,
 * coarse_bbox.real_to_unit(real_qpoints[i]))); needs no resident problem.  bbox [n_boxes][2][dim] (lower corner,
 * upper corner); pt_ptr [n_boxes+1] CSR offsets of the points of every box; pts [dim][N] real coordinates;
 * values [N][n] row-major, n = dofs per cell of (dim, degree, basis).                                         */
int pdh_shape_values(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *bbox,
                     const int64_t *pt_ptr, const double *pts, double *values);

/* Device-resident variants of the three calls above: every pointer is DEVICE memory, nothing is allocated or copied,
 * the kernels are queued on pdh_stream() and the call returns (pdh_synchronize waits).  Arrays are in the CALLER's order,
 * exactly as for the host variants: d_f_vol [Nq_tot] / d_g_bdry [Nqf_tot] sampled at vq_x / fq_x of the resident
 * description (NULL = absent), d_rhs [row_end-row_begin]; d_pt_ptr [n_agg+1], d_pts [dim][n_points] (component stride
 * n_points), d_u [n_points], d_grad [dim][n_points] or NULL - only the points of polytopes owned by the context are written.
 * The host variants are these plus the transfers through grow-only scratch buffers of the context.              */
int pdh_assemble_rhs_device(pdh_ctx *ctx, const double *d_f_vol, const double *d_g_bdry, double *d_rhs);
int pdh_evaluate_device(pdh_ctx *ctx, const double *d_solution, const int64_t *d_pt_ptr, const double *d_pts, int64_t n_points,
                        double *d_u, double *d_grad);
int pdh_shape_values_device(pdh_ctx *ctx, int dim, int degree, int basis, int n_boxes, const double *d_bbox,
                            const int64_t *d_pt_ptr, const double *d_pts, int64_t n_points, double *d_values);

/* PolyUtils::compute_global_error (reference include/poly_utils.h:1647-1750) with the weighted sums formed ON THE DEVICE:
 *   sums[0] = sum_q JxW_q (u(x_q) - u_h(x_q))^2,   sums[1] = sum_q JxW_q |grad u(x_q) - grad u_h(x_q)|^2
 * over the points of the polytopes owned by the context (the SQUARES: ranks add them before the root, like the reference's
 * Utilities::MPI::sum, :1736-1745).  pt_ptr / pts as for pdh_evaluate; w [N] the JxW of the points; exact_u [N] and
 * exact_grad [dim][N] the analytical solution and its gradient sampled by the caller at the same points (the library has no
 * callbacks into host code).  One kernel evaluates u_h, grad u_h and the two sums per polytope (fixed summation order:
 * the result is reproducible); 16 bytes per polytope cross PCIe instead of 8 (dim + 1) per point.  sums is HOST memory in
 * both variants; the _device variant takes every array in device memory and synchronises the stream before it returns. */
int pdh_global_error(pdh_ctx *ctx, const double *solution, const int64_t *pt_ptr, const double *pts, const double *w,
                     const double *exact_u, const double *exact_grad, double *sums /* [2] */);
int pdh_global_error_device(pdh_ctx *ctx, const double *d_solution, const int64_t *d_pt_ptr, const double *d_pts, int64_t n_points,
                            const double *d_w, const double *d_exact_u, const double *d_exact_grad, double *sums /* [2], host */);

/* Access to device-resident results and synchronisation. */
int pdh_device_values(pdh_ctx *ctx, double **device_ptr, int64_t *n_values);
int pdh_synchronize(pdh_ctx *ctx);
void *pdh_stream(pdh_ctx *ctx); /* hipStream_t the kernels are launched on */

/* Multi-GPU, two realisations of the one exchange step of the path:
 *   PDH_EXCHANGE_NONE  (default) owner-computes-rows: a face cut by the partition is contracted on BOTH ranks, each writing
 *                      only its own rows - no matrix traffic at all (the reference's compress(VectorOperation::add),
 *                      include/poly_utils.h:2194, disappears).
 *   PDH_EXCHANGE_GHOST the reference's scheme (include/poly_utils.h:1930-1992, 2134-2194; examples/diffusion_reaction.cc:
 *                      615-692): the rank owning side 0 of a cut face assembles all four blocks, keeps M11/M12 and ships
 *                      M21 (one n x n block per face) and M22 (summed per remote polytope) to the owner of those rows.
 *                      Needs problem->agg_rank.  A step is then
 *                         pdh_assemble_device(ctx);                 owned rows minus the foreign faces + outgoing blocks
 *                         pdh_exchange_get_send(ctx, d_send);       [sum send_count] doubles, peer by peer in rank order
 *                         <caller moves them: grouped ncclSend/ncclRecv or all-to-all-v over RCCL/xGMI, d_send -> peers' d_recv>
 *                         pdh_exchange_apply(ctx, d_recv);          stores the M21 blocks, adds the M22 sums
 *                      The library stays transport-free (no RCCL/MPI dependency in the C ABI); bench.py drives it with
 *                      torch.distributed (RCCL).  Both ranks derive the block order of a peer buffer from the global dof
 *                      numbers of the cut faces, so no index lists are exchanged.  Results equal PDH_EXCHANGE_NONE up to
 *                      rounding (1e-14 relative).  Mode changes take effect at the next pdh_set_problem*.
 *                      The wire format (n = dofs per polytope, blocks of n * n doubles): d_send holds one segment per peer
 *                      in rank order, send_count[peer] doubles each (0 for the rank itself and for peers without a common
 *                      face); d_recv likewise, recv_count[peer] doubles from every peer.  A segment carries
 *                        1. the M21 blocks of the cut faces towards that peer, ascending by (first dof of the side-0
 *                           polytope P, first dof of the side-1 polytope Q): plain [row of Q][column of P] - A[Q, P];
 *                        2. one M22 block per distinct side-1 polytope Q of those faces, ascending by its first dof: the
 *                           sum over the sender's cut faces into Q of their contribution to A[Q, Q], in the layout of
 *                           Q's diagonal block - plain [row][column] with diag_first = 0; with diag_first = 1 row R holds
 *                           column R first, then the columns 0 .. R-1, then R+1 .. n-1.
 *                      A polytope cut off from several peers receives one M22 block from each; pdh_exchange_apply adds
 *                      them to the diagonal block in peer order and STORES the M21 blocks (the assembly writes nothing
 *                      there: between pdh_assemble_device and pdh_exchange_apply those entries hold what stood there
 *                      before).                                                                                        */
#define PDH_EXCHANGE_NONE 0
#define PDH_EXCHANGE_GHOST 1
int pdh_set_exchange_mode(pdh_ctx *ctx, int mode);
int pdh_exchange_layout(pdh_ctx *ctx, int n_ranks, int64_t *send_count /* [n_ranks] doubles */, int64_t *recv_count);
int pdh_exchange_get_send(pdh_ctx *ctx, double *d_send /* device memory */);
int pdh_exchange_apply(pdh_ctx *ctx, const double *d_recv /* device memory */);
/* Launch everything on a stream of the caller (hipStream_t; NULL = the context's own): collectives issued on that
 * stream are then ordered with the kernels without host synchronisation.                                       */
int pdh_set_stream(pdh_ctx *ctx, void *stream);
/* Host-only (no GPU): the per-peer sizes pdh_exchange_layout would report for this description and row range. */
int pdh_check_exchange(const pdh_problem *problem, int32_t row_begin, int32_t row_end, int n_ranks, int64_t *send_count,
                       int64_t *recv_count);
/* Copy of the owned rows' values as they stand in HBM (after pdh_assemble_device / pdh_exchange_apply). */
int pdh_copy_values(pdh_ctx *ctx, double *values);
/* One pass over the values in HBM: out4 = { sum, sum of |.|, max |.|, number of non-finite entries } of the owned rows -
 * a validity signal for matrices too large to copy back (for FE_DGQ the sum is 1^T A 1, known in closed form).        */
int pdh_values_checksum(pdh_ctx *ctx, double *out4);

/* Two algebraically identical forms of the same sums exist (results differ by rounding only, both are tested against
 * the oracle): DIRECT contracts basis values over the quadrature points for all n^2 pairs (f64 MFMA, pdh_kernels.h;
 * pdh_tiled.h for more than 64 dofs per polytope);
 * MOMENT first reduces the quadrature to (2p+1)^3 Legendre moments per polytope / face and obtains the blocks by sum
 * factorisation (pdh_moment.h; 3-D, degree 1..3).  AUTO picks the faster one for the resident problem.          */
#define PDH_ALG_AUTO 0
#define PDH_ALG_DIRECT 1
#define PDH_ALG_MOMENT 2
#define PDH_ALG_MIXED 3 /* reported only: AUTO chose MOMENT for the diagonal blocks and DIRECT for the coupling blocks */
/* ROWS: the owner of a polytope writes ALL blocks of its rows as whole 128-byte lines (owner computes rows).  Exists in 3-D for
 * FE_DGQ / FE_AggloDGP of degree 1 .. 3 when every face of every owned polytope lies in axis-aligned planes (agglomerates of
 * Cartesian cells; a neighbour may be met along several planes - METIS-like "staircase" agglomerates - for every element).  Every
 * element but FE_DGQ(3) additionally needs tensor-product rules on the sub-cells and sub-faces (vq_tensor_n / fq_tensor_n).
 * Several kernels serve it (pdh_rows_kernel_in_use below).  AUTO takes it whenever the resident problem qualifies (tested on the
 * quadrature points at pdh_set_problem - or known by construction after pdh_set_problem_cartesian - no mesh flag needed).   */
#define PDH_ALG_ROWS 4
/* Host-only: 1 if PDH_ALG_ROWS applies to this description / row range, 0 if not (pdh_last_error(NULL) says why). */
int pdh_check_rows(const pdh_problem *problem, int32_t row_begin, int32_t row_end);
/* Host-only: 1 if the term kernels (PDH_ROWS_TERMS) apply to this description / row range, 0 if not (pdh_last_error(NULL) says
 * why).  stats5 (may be NULL): most runs (polytopal faces), sub-faces, interior sub-faces and cells of one owned polytope, and
 * the LDS bytes a workgroup needs for them (the kernels apply while that stays within their budget).                          */
int pdh_check_terms(const pdh_problem *problem, int32_t row_begin, int32_t row_end, int64_t *stats5);
/* Term kernels sum over the cells and sub-faces of a polytope; where those form tensor grids (block agglomerates: the R-tree levels of a
 * structured grid; the sub-faces shared with one neighbour in one plane) a sub-grid of them is ONE cell / sub-face with composite 1-D
 * rules - found on the data at pdh_set_problem.  out4 = { cells, cells after merging, sub-faces, sub-faces after merging } of the
 * resident problem's owned polytopes (zeros if another kernel serves it).                                                          */
int pdh_terms_merge_stats(pdh_ctx *ctx, int64_t *out4);
int pdh_set_algorithm(pdh_ctx *ctx, int algorithm);
/* Which row kernel serves the resident problem (PDH_ALG_ROWS has several; all write whole rows, owner computes rows):
 *   TERMS    every element of degree 1 .. 3 on agglomerates of Cartesian cells with tensor-product rules, while a polytope's 1-D tables
 *            fit the kernels' LDS budget: every entry a short sum of products of three 1-D matrix entries per sub-cell / sub-face, any
 *            number of planes per neighbour; cells / sub-faces that form tensor grids summed over as one with composite rules
 *            (pdh_terms.h, one wave per polytope; FE_DGQ(3): pdh_terms_wg.h, a workgroup per polytope - PDH_TERMS_DGQ3=0 in the
 *            environment keeps pdh_rows.h for that element; reference examples/poisson.cc:413, 543-566 - FE_AggloDGP on METIS
 *            agglomerates - is this case)
 *   PIECES   FE_DGQ(3), one plane per neighbour: moments + Kronecker form, rows in aligned 512-byte pieces (pdh_rows.h) - also
 *            for rules without tensor structure
 *   MULTI    FE_DGQ(3), several planes per neighbour (METIS-like agglomerates of Cartesian cells; pdh_rows.h)
 *   STREAMED FE_DGQ(1,2) / FE_AggloDGP(1..3), moment form, one plane per neighbour (pdh_rows.h): polytopes beyond the LDS budget of
 *            TERMS                                                                                                              */
#define PDH_ROWS_NONE 0
#define PDH_ROWS_PIECES 1
#define PDH_ROWS_MULTI 2
#define PDH_ROWS_STREAMED 3
#define PDH_ROWS_TERMS 4
int pdh_rows_kernel_in_use(pdh_ctx *ctx);
int pdh_algorithm_in_use(pdh_ctx *ctx); /* PDH_ALG_DIRECT, PDH_ALG_MOMENT, PDH_ALG_MIXED or PDH_ALG_ROWS for the resident problem, < 0 on error */

/* On large problems the two kernels of a step (diagonal blocks / coupling blocks: disjoint values, complementary
 * bottlenecks) run concurrently, the second on an internal stream forked from and joined into pdh_stream() - callers
 * still see one ordered stream.  pdh_set_overlap(ctx, 0) serialises them (cleaner per-kernel timings, ~4 % slower).   */
int pdh_set_overlap(pdh_ctx *ctx, int enabled);

/* Measurement helpers (HIP events on the context's stream).  kernel 0 = diagonal-block kernel
 * (volume + own-side face terms), kernel 1 = off-diagonal (interface coupling) kernel.            */
#define PDH_N_KERNELS 2
int pdh_set_profiling(pdh_ctx *ctx, int enabled); /* enabling (re)starts the accumulation */
int pdh_kernel_times_ms(pdh_ctx *ctx, float *ms /* [PDH_N_KERNELS] average per launch */,
                        int *n_launches /* launches averaged over, may be NULL */);
int pdh_problem_stats(pdh_ctx *ctx, int64_t *stats /* [8]: n_owned_agg, n_offdiag_items, n_vq_points,
                        n_face_side_points, n_values, dofs_per_cell, lds_bytes_diag, lds_bytes_offdiag */);

/* Executed work of one pdh_assemble_device launch: v_mfma_f64_4x4x4_4b_f64 instructions issued by k_diag and
 * k_offdiag (512 flop each).  Smaller than the algorithmic count of SURVEY.md 8(d): only the upper tile
 * pairs of the symmetric diagonal blocks are computed and A[Q,P] is written as A[P,Q]^T.             */
int pdh_kernel_work(pdh_ctx *ctx, int64_t *mfma_instr /* [PDH_N_KERNELS] */);

/* Host-only validation of a problem description: runs every check of pdh_set_problem_local without
 * touching a GPU (usable on a build machine).  stats as in pdh_problem_stats, may be NULL.          */
int pdh_check_problem(const pdh_problem *problem, int32_t row_begin, int32_t row_end, int64_t *stats);

/* Solving with the resident matrix (pdh_solve.hip).  The values are used as they stand in HBM: after pdh_assemble* or
 * pdh_exchange_apply.  Every call needs a resident problem (else PDH_ESTATE).  Every sum (dot products, norms) is formed in a fixed
 * order - per-polytope partials, then one fixed-order pass - so the same call on the same data gives the same bits.
 *
 * y = A x for the owned rows.  x [n_rows] is in the GLOBAL dof numbering (dof_offset): a rank-local context reads its ghost columns
 * from it; y [row_end-row_begin] is overwritten.  Every resident problem (global, row range, rank-local, Cartesian, more than 64 dofs
 * per polytope; both layouts, col_offset included).  x and y must not overlap (PDH_EINVAL).  The _device variant takes device
 * pointers and is asynchronous on pdh_stream().                                                                                    */
int pdh_vmult(pdh_ctx *ctx, const double *x, double *y);
int pdh_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y);

/* Preconditioners, built from the values as they stand (like deal.II's precondition.initialize(A)).  A diagonal block that is not
 * positive definite (a Cholesky pivot <= 0 or not finite) - for point Jacobi a zero or non-finite diagonal entry - makes the set-up
 * fail with PDH_EINVAL naming the first such polytope.  PDH_PREC_BLOCK_JACOBI needs n <= 64 dofs per polytope (PDH_EUNSUPPORTED).
 * pdh_precondition_device (z = P^-1 r over the owned rows, device pointers, asynchronous) and pdh_solve_cg* return PDH_ESTATE when
 * the values changed (pdh_set_problem*, pdh_assemble*, pdh_exchange_apply) since the set-up.  PDH_PREC_NONE needs no set-up call.
 * d_r and d_z of pdh_precondition_device are either the same array (in place, every kind) or disjoint: a partial overlap is
 * PDH_EINVAL.                                                                                                                        */
#define PDH_PREC_NONE 0
#define PDH_PREC_JACOBI 1       /* inverse of the diagonal                                */
#define PDH_PREC_BLOCK_JACOBI 2 /* inverses of the n x n diagonal blocks, one per polytope */
int pdh_setup_preconditioner(pdh_ctx *ctx, int kind);
int pdh_precondition_device(pdh_ctx *ctx, const double *d_r, double *d_z);

/* Conjugate gradients preconditioned with the preconditioner set up last (none if there was no set-up).  x: initial guess in,
 * solution out.  Stops when ||r||_2 <= max(abs_tol, rel_tol * ||b||_2), tested before every iteration.  Needs a context that owns
 * ALL rows with PDH_EXCHANGE_NONE (else PDH_EUNSUPPORTED).  At max_iter it returns PDH_ENOCONV with res and x filled.  b and x must
 * not overlap.  The _device variant takes device pointers and synchronises before it returns.  Scratch vectors and the inverse
 * blocks are grow-only buffers of the context, allocated at first use, freed with the problem.                                     */
typedef struct pdh_cg_control
{
  int32_t max_iter;
  double rel_tol;
  double abs_tol;
} pdh_cg_control;
typedef struct pdh_cg_result
{
  int32_t iterations;
  double residual0; /* ||b - A x0||_2 */
  double residual;  /* ||r||_2 at the end */
} pdh_cg_result;
int pdh_solve_cg(pdh_ctx *ctx, const pdh_cg_control *control, const double *b, double *x, pdh_cg_result *result);
int pdh_solve_cg_device(pdh_ctx *ctx, const pdh_cg_control *control, const double *d_b, double *d_x, pdh_cg_result *result);

/* Chebyshev smoother / preconditioner over point or block Jacobi (reference: PreconditionChebyshev as the multigrid smoother of
 * examples/simplex_agglomerated_multigrid.cc:410-470 - degree 5, smoothing range 20, 20 CG steps for the eigenvalue estimate).  With P
 * the inner preconditioner and `est` the largest Ritz value of P^-1 A:
 *   lambda_hi = 1.2 est, lambda_lo = lambda_hi / smoothing_range, theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta,
 *   rho_0 = 1 / sigma;   r_0 = b - A x_0,  d_0 = (1 / theta) P^-1 r_0,  x_1 = x_0 + d_0;   for k = 1 .. degree - 1:
 *   r_k = r_(k-1) - A d_(k-1),  rho_k = 1 / (2 sigma - rho_(k-1)),  d_k = rho_k rho_(k-1) d_(k-1) + (2 rho_k / delta) P^-1 r_k,
 *   x_(k+1) = x_k + d_k.
 * One application is degree - 1 products with A (one more from a non-zero start) and degree fused updates queued back to back: the
 * coefficients are computed on the host at the set-up, nothing is synchronised inside.  est comes from eig_cg_n_iterations steps of
 * P-preconditioned CG on A x = b0 from x = 0 on the device, b0[i] = ((2654435761 i) mod 2^32) / 2^32 - 1/2: the largest eigenvalue
 * of the Lanczos tridiagonal of its alpha_j, beta_j (T_jj = 1 / alpha_j + beta_(j-1) / alpha_(j-1), T_(j,j+1) = sqrt(beta_j) /
 * alpha_j; fewer steps if the residual reaches zero).  max_eigenvalue > 0 is taken as est instead and no CG runs.
 * pdh_setup_chebyshev builds the inner preconditioner (failures as for pdh_setup_preconditioner), estimates, and makes
 * PDH_PREC_CHEBYSHEV the preconditioner of pdh_precondition_device (z = the application to r from a zero start) and pdh_solve_cg*.
 * PDH_EINVAL: degree < 1, smoothing_range <= 1, inner not one of the two, eig_cg_n_iterations outside 1 .. 256 while it is needed.
 * Needs a context that owns all rows with PDH_EXCHANGE_NONE (PDH_EUNSUPPORTED), like pdh_solve_cg.  pdh_setup_preconditioner does
 * not take PDH_PREC_CHEBYSHEV (PDH_EINVAL).  pdh_chebyshev_step_device is the smoother: one application to b from the x given
 * (zero_initial_guess != 0: x is not read), device pointers [n_rows], asynchronous on pdh_stream(); b and x must not overlap.    */
#define PDH_PREC_CHEBYSHEV 3
typedef struct pdh_chebyshev_control
{
  int32_t inner;               /* PDH_PREC_JACOBI | PDH_PREC_BLOCK_JACOBI */
  int32_t degree;              /* >= 1 */
  double smoothing_range;      /* > 1 */
  int32_t eig_cg_n_iterations; /* 1..256, unused when max_eigenvalue > 0 */
  double max_eigenvalue;       /* > 0: used as `est` */
} pdh_chebyshev_control;
typedef struct pdh_chebyshev_info
{
  double estimate, lambda_lo, lambda_hi;
  int32_t cg_iterations, degree, inner;
} pdh_chebyshev_info;
int pdh_setup_chebyshev(pdh_ctx *ctx, const pdh_chebyshev_control *control, pdh_chebyshev_info *info /* may be NULL */);
int pdh_chebyshev_step_device(pdh_ctx *ctx, const double *d_b, double *d_x, int zero_initial_guess);
/* Host-only: smallest and largest eigenvalue of the symmetric tridiagonal matrix with diagonal diag [k] and off-diagonal
 * offdiag [k-1] (not read for k = 1), 1 <= k <= 256, by bisection on Sturm counts (a few ulp of the largest |eigenvalue|). */
int pdh_tridiagonal_eigenvalues(int k, const double *diag, const double *offdiag, double *lo, double *hi);

/* r = b - A x on the resident values: the one vector operation of a multigrid cycle next to the smoother, the transfers below and the
 * coarse solve.  Device pointers, asynchronous on pdh_stream(); x [n_rows] in the global numbering like pdh_vmult_device, b and r
 * [row_end-row_begin].  r must overlap neither x nor b (PDH_EINVAL); PDH_ESTATE without a resident problem.                      */
int pdh_residual_device(pdh_ctx *ctx, const double *d_b, const double *d_x, double *d_r);

/* Level transfer between two NESTED polytopal FE_DGQ spaces (pdh_transfer.hip): the reference's MGTransferAgglomeration
 * (include/multigrid_amg.h:439-490 prolongate, prolongate_and_add, restrict_and_add) over the injection of Utils::fill_injection_matrix
 * (include/utils.h:95-270), without its matrix.  The basis lives on the bounding box and the support points of a fine polytope are a
 * tensor grid in its box, so every injection block (fine polytope F, parent C) is the Kronecker product of `dim` 1-D matrices
 *   B_c[i][j] = l_j((lo_F[c] + node_i h_F[c] - lo_C[c]) / h_C[c])
 * (l_j: Lagrange polynomials on the p + 1 Gauss-Lobatto nodes; first axis fastest in the dof index): dim (p+1)^2 doubles per fine
 * polytope, applied by sum factorisation.  All pointers of the description are caller-owned host memory, read during the call only. */
typedef struct pdh_transfer_desc
{
  int32_t dim, degree, basis;          /* 2|3, 1..7, PDH_BASIS_DGQ                                     */
  int32_t n_fine, n_coarse;            /* polytopes                                                    */
  int32_t n_fine_rows, n_coarse_rows;  /* lengths of the level vectors                                 */
  const double  *fine_bbox, *coarse_bbox;              /* [n][2][dim] as pdh_problem.bbox              */
  const int32_t *fine_dof_offset, *coarse_dof_offset;  /* [n] as pdh_problem.dof_offset                */
  const int32_t *parent;                               /* [n_fine] coarse polytope of every fine one   */
} pdh_transfer_desc;
/* Host-only.  PDH_EUNSUPPORTED: FE_AggloDGP (no support points; the reference refuses it too, include/fe_agglodgp.h:63), degree 0 or
 * above 7, 2-D with more than 64 dofs per polytope.  PDH_EINVAL: a parent out of range, a coarse polytope without children, a
 * degenerate box, a fine box not inside its parent's (slack: 1e-12 of the parent's extent per axis), dof ranges [off, off + n) that
 * overlap or leave [0, n_rows) on either level, n_coarse >= n_fine (include/utils.h:120).  pdh_last_error(NULL) says which.      */
int pdh_check_transfer(const pdh_transfer_desc *d);
/* Host-only: the 1-D matrices, out [n_fine][dim][p+1][p+1] (B_c[i][j] as above), from the tables of the kernels' basis. */
int pdh_transfer_matrices_1d(const pdh_transfer_desc *d, double *out);
/* Host-only: the children of every coarse polytope as a CSR, child_ptr [n_coarse+1], child_idx [n_fine], ascending fine index per
 * parent - the order in which the restriction adds the children's contributions.                                           */
int pdh_transfer_children(const pdh_transfer_desc *d, int32_t *child_ptr, int32_t *child_idx);

/* A transfer lives on the device and stream of the context it was created on and needs NO resident problem there (the levels live in
 * different contexts); destroy it before its context.  pdh_transfer_create runs pdh_check_transfer, builds the tables and the children
 * CSR on the host and uploads them - there is no set-up kernel.  Errors of a transfer are reported on its context (pdh_last_error).
 *   prolongate          fine    = P coarse        prolongate_and_add    fine   += P coarse
 *   restrict            coarse  = P^T fine        restrict_and_add      coarse += P^T fine
 * The _device entries take device pointers (coarse [n_coarse_rows], fine [n_fine_rows]) and are asynchronous on pdh_stream() of the
 * context; pdh_prolongate / pdh_restrict take host pointers, staged like pdh_vmult, and give the same bits.  NULL or overlapping vectors:
 * PDH_EINVAL.  The restriction adds the children of a coarse polytope in ascending fine index, no atomics: the same call on the same
 * data gives the same bits.  Global descriptions only (one context per level, like pdh_solve_cg).                                */
typedef struct pdh_transfer pdh_transfer;
int  pdh_transfer_create(pdh_ctx *ctx, const pdh_transfer_desc *d, pdh_transfer **out);
void pdh_transfer_destroy(pdh_transfer *t);
int pdh_prolongate_device        (pdh_transfer *t, const double *d_coarse, double *d_fine);
int pdh_prolongate_and_add_device(pdh_transfer *t, const double *d_coarse, double *d_fine);
int pdh_restrict_device          (pdh_transfer *t, const double *d_fine,   double *d_coarse);
int pdh_restrict_and_add_device  (pdh_transfer *t, const double *d_fine,   double *d_coarse);
int pdh_prolongate(pdh_transfer *t, const double *coarse, double *fine);
int pdh_restrict  (pdh_transfer *t, const double *fine,   double *coarse);

/* p-transfer: the SAME polytopes at two polynomial degrees q = coarse_degree < p = fine_degree (pdh_ptransfer.hip) - the hierarchy
 * every mesh has, nested or not.  Both bases live in the unit coordinates of the polytope's bounding box, so no box enters and every
 * polytope has the same injection block:
 *   FE_DGQ       the Kronecker power (first axis fastest) of ONE (p+1) x (q+1) matrix B[i][j] = l^q_j(node^p_i): the degree-q Lagrange
 *                basis on its Gauss-Lobatto nodes at the degree-p Gauss-Lobatto nodes; applied by rectangular sum factorisation.
 *   FE_AggloDGP  the basis is the orthonormal Legendre product basis of the box frame, a coarse function IS a fine one: the injection
 *                is the index map between the two multi-index lists (2-D 1 -> 2: [0, 1, 3]), exact to the bit.
 * All pointers of the description are caller-owned host memory, read during the call only.                                          */
typedef struct pdh_ptransfer_desc
{
  int32_t dim, fine_degree, coarse_degree, basis;      /* 2|3; 1 <= coarse < fine <= 7; PDH_BASIS_DGQ | PDH_BASIS_AGGLODGP */
  int32_t n_polytopes;                                 /* the same polytopes on both levels                              */
  int32_t n_fine_rows, n_coarse_rows;                  /* lengths of the level vectors                                   */
  const int32_t *fine_dof_offset, *coarse_dof_offset;  /* [n_polytopes] as pdh_problem.dof_offset                        */
} pdh_ptransfer_desc;
/* Host-only.  The refusals, in this order: PDH_EINVAL for a NULL description, dim other than 2 or 3, an unknown basis;
 * PDH_EUNSUPPORTED for degrees outside 1 <= coarse_degree < fine_degree <= 7 (in 2-D this is also the h-transfer's bound of 64 fine dofs
 * per polytope); PDH_EINVAL for n_polytopes <= 0, NULL offsets, dof ranges [off, off + n) that overlap or leave [0, n_rows) on either
 * level.  pdh_last_error(NULL) says which.                                                                                           */
int pdh_check_ptransfer(const pdh_ptransfer_desc *d);
/* Host-only, FE_DGQ (FE_AggloDGP: PDH_EINVAL): out [p+1][q+1], B[i][j] as above, from the 1-D basis behind the kernels' tables. */
int pdh_ptransfer_matrix_1d(const pdh_ptransfer_desc *d, double *out);
/* Host-only, FE_AggloDGP (FE_DGQ: PDH_EINVAL): out [n coarse dofs per polytope], the fine dof that IS coarse dof j. */
int pdh_ptransfer_index_map(const pdh_ptransfer_desc *d, int32_t *out);
/* The same opaque pdh_transfer as pdh_transfer_create gives, on the device and stream of `ctx` (no resident problem needed): everything
 * above that takes one - pdh_prolongate*, pdh_restrict*, pdh_transfer_destroy - and pdh_mg_create serve it.  Runs pdh_check_ptransfer;
 * uploads the two offset lists (and the index map); the 1-D matrix travels with every launch.  Every sum has a fixed order, no atomics:
 * the same call on the same data gives the same bits; FE_AggloDGP transfers copy values and are exact.  Rows that belong to no polytope
 * are not touched by the _device entries; prolongate_and_add leaves the fine FE_AggloDGP dofs outside the image untouched.
 * pdh_galerkin_device on such a transfer is PDH_EUNSUPPORTED: coarse degrees are re-assembled on their own description.              */
int pdh_ptransfer_create(pdh_ctx *ctx, const pdh_ptransfer_desc *d, pdh_transfer **out);

/* Coarse level matrix as the Galerkin product A_c = P^T A_f P (pdh_galerkin.hip): the reference's AmgProjector::compute_level_matrices
 * (include/multigrid_amg.h:267-305) over the injection of the transfer, without the injection matrix.  With par() the parent map and B_X
 * the Kronecker injection block of fine polytope X,
 *   A_c[C, C'] = sum over the fine blocks (F, F') with par(F) = C, par(F') = C' of  B_F^T A_f[F, F'] B_F'.
 * If fine polytopes share a face their parents are equal or share a face, so on nested levels every fine block lands in ONE block of the
 * coarse level's own face-neighbour pattern: the product is written into the rows the coarse context already has, and everything that
 * reads them (pdh_vmult*, every pdh_setup_*, pdh_copy_values) works as after pdh_assemble_device.  At most 64 dofs per polytope.
 *
 * pdh_galerkin_plan, host-only: which fine blocks every coarse block receives, and in which order they are added.  A level is given by
 * the block lists of its resident rows - slot s is the s-th polytope, blk_dof[blk_ptr[s] + t] the first global dof of the t-th block of
 * its rows in value order (ascending col_offset or dof_offset, whichever orders the pattern) - and what the refusals read.  Output: a
 * CSR over the coarse blocks, block b = coarse->blk_ptr[slot] + t; plan_ptr [coarse->blk_ptr[n] + 1], plan_slot / plan_pos
 * [fine->blk_ptr[n]]: fine slot and block position of every entry, ascending (slot, position) inside a coarse block - the summation
 * order.  Runs pdh_check_transfer first.  PDH_EINVAL: a level's slot count, row count or dof offsets differ from the transfer's; a block
 * dof that is not the first dof of a polytope; a fine block whose pair of parents is no block of the coarse pattern (levels not nested,
 * or patterns that are not face-neighbour patterns); a coarse block that receives nothing.  PDH_EUNSUPPORTED: more than 64 dofs per
 * polytope (3-D FE_DGQ(4..7), which the transfers themselves accept); a level that does not own all its rows or was set in
 * PDH_EXCHANGE_GHOST mode; levels on different devices.  pdh_last_error(NULL) says which.                                        */
typedef struct pdh_galerkin_level
{
  int32_t n_slots;             /* owned polytopes                                                     */
  int32_t n_rows_owned, n_rows;/* rows of the owned polytopes, rows of the level                      */
  int32_t exchange_mode;       /* PDH_EXCHANGE_* the problem was set in                               */
  int32_t device;
  const int64_t *blk_ptr;      /* [n_slots + 1]                                                       */
  const int32_t *blk_dof;      /* [blk_ptr[n_slots]]                                                  */
  const int32_t *dof_offset;   /* [n_slots] first dof of every slot's polytope                        */
} pdh_galerkin_level;
int pdh_galerkin_plan(const pdh_transfer_desc *d, const pdh_galerkin_level *fine, const pdh_galerkin_level *coarse, int64_t *plan_ptr,
                      int32_t *plan_slot, int32_t *plan_pos);
/* Host-only: the 1-D matrices the product applies, out [n_fine][dim][p+1][p+1]: those of pdh_transfer_matrices_1d with every row that lies
 * within 64 ulp of a unit vector made that unit vector.  Such a row belongs to a fine support point that IS a coarse one (the corners and
 * faces of nested boxes), where the injection is exactly 0 and 1; the rounded Horner form leaves 1e-19 .. 1e-17 in the zeros, which is
 * nothing to a transfer but the whole of an entry of P^T A P that is structurally zero.  The factors of the product and of pdh_prolongate* / pdh_restrict* thus differ
 * by those 1e-19 .. 1e-17 (64 ulp at the very most), inside the 1e-13 of the sum of absolute products every row of either is held to. */
int pdh_galerkin_matrices_1d(const pdh_transfer_desc *d, double *out);
/* coarse's values = P^T A_f P, A_f the values of the context `t` was created on as they stand.  PDH_ESTATE: that context has no resident
 * problem or its values were never assembled (pdh_assemble*, or a pdh_galerkin_device into it), or `coarse` has no resident problem -
 * `coarse` needs its pattern only, its values are overwritten.  The refusals of pdh_galerkin_plan apply.  The plan is built at the first
 * call and kept on the transfer until a pdh_set_problem* on either context.  One kernel on the fine context's stream, one wave per coarse
 * block, every sum in a fixed order and no atomics: the same call on the same data gives the same bits.  A set-up call: it synchronises
 * both streams before it starts and the fine one before it returns.  Afterwards `coarse`'s values count as assembled and CHANGED - a
 * preconditioner set up before and a pdh_mg that holds `coarse` turn stale as after pdh_assemble_device, which may also overwrite them
 * again later.  A later change of the fine values does not refresh the coarse ones.  Errors are reported on the fine context.        */
int pdh_galerkin_device(pdh_transfer *t, pdh_ctx *coarse);

/* Dense direct solve on the resident matrix (pdh_dense.hip): the coarse solver of a multigrid hierarchy, the reference's MGCoarseDirect
 * (examples/simplex_agglomerated_multigrid.cc:71-100, used at :476).  For a context that owns all rows with PDH_EXCHANGE_NONE (else PDH_EUNSUPPORTED,
 * like pdh_setup_chebyshev) and has at most 1024 rows (more: PDH_EUNSUPPORTED; 1024 rows are 16 polytopes of 64 dofs).  The set-up runs on
 * the device without reading the matrix back: the resident rows are gathered into a dense array (the diagonal-first shift undone,
 * dof_offset honoured), factored A = L L^T, and the explicit inverse G = L^-T L^-1 is stored EXACTLY symmetric; every sum has a fixed
 * order.  A Cholesky pivot (the diagonal entry at its elimination step) <= 0 or not finite is PDH_EINVAL naming the row.  After a
 * successful set-up PDH_PREC_DIRECT is the preconditioner of the context: pdh_precondition_device gives z = G r by one kernel queued on
 * pdh_stream() (in place or disjoint, like every other kind; the same call on the same data gives the same bits), pdh_solve_cg* uses
 * it, and the staleness rules of the other kinds apply (PDH_ESTATE once the values changed).  pdh_setup_preconditioner does not take
 * PDH_PREC_DIRECT (PDH_EINVAL).                                                                                                       */
#define PDH_PREC_DIRECT 4
typedef struct pdh_direct_info
{
  int32_t n_rows;
  double pivot_min, pivot_max; /* smallest / largest Cholesky pivot */
} pdh_direct_info;
int pdh_setup_direct(pdh_ctx *ctx, pdh_direct_info *info /* may be NULL */);

/* Multigrid V-cycle over resident level matrices (pdh_capi_mg.cpp; no kernel of its own: the smoother, the residual, the transfers and
 * the coarse solver above), the reference's Multigrid / PreconditionMG of examples/simplex_agglomerated_multigrid.cc:378-515.
 * pdh_mg_create takes 2 <= n_levels <= 16 contexts, COARSE TO FINE, on one device, each owning all rows of an assembled problem; every
 * level above the coarsest with PDH_PREC_CHEBYSHEV set up and current (its smoother), the coarsest with ANY preconditioner set up and
 * current as its solver - PDH_PREC_DIRECT, or Chebyshev / block Jacobi / Jacobi beyond 1024 rows; PDH_PREC_NONE is refused.  Every kind
 * is a fixed symmetric positive operator, so the cycle is one too.  transfers[l] connects level l and l + 1, was created on levels[l + 1]
 * and has their row counts.  A violation is PDH_EINVAL or PDH_ESTATE with a message naming the level, reported on the FINEST context
 * (pdh_last_error(levels[n_levels - 1])), as every later error of the mg is.  The mg owns the level vectors b_l, x_l, r_l; it
 * synchronises every level's stream once and makes PDH_PREC_MULTIGRID the preconditioner of the finest context:
 * pdh_precondition_device(finest, r, z) is one V-cycle from zero and pdh_solve_cg* on the finest context is V-cycle-preconditioned CG
 * (the same solve gives the same bits).
 *   One cycle, every launch of every level on pdh_stream(finest) as it stands at the call - no events, no second stream, no graph, no
 *   host synchronisation, no read-back.  From the finest level l down: x_l <- Chebyshev on b_l (from zero; on the finest level from
 *   the caller's x if zero_initial_guess == 0), r_l = b_l - A_l x_l, b_(l-1) = P^T r_l; x_0 = the coarsest preconditioner applied to
 *   b_0; on the way up x_l += P x_(l-1), then Chebyshev from x_l.
 * pdh_mg_vcycle_device: device pointers [n_rows of the finest level], b and x must not overlap (PDH_EINVAL).  A later
 * pdh_setup_preconditioner / pdh_setup_chebyshev / pdh_setup_direct on the finest context replaces the preconditioner and detaches the
 * mg; pdh_mg_destroy detaches it too - the context falls back to PDH_PREC_NONE and says so (PDH_ESTATE) when it is asked to
 * precondition or solve before something is set up again.  Once the values or the preconditioner of ANY level changed since
 * pdh_mg_create, every entry of the mg and pdh_precondition_device / pdh_solve_cg* on the finest context return PDH_ESTATE naming the
 * level.  Destroy the mg before its transfers and contexts.                                                                          */
#define PDH_PREC_MULTIGRID 5
typedef struct pdh_mg pdh_mg;
int  pdh_mg_create(int n_levels, pdh_ctx *const *levels /* coarse to fine */,
                   pdh_transfer *const *transfers /* [n_levels-1]; transfers[l]: level l <-> l+1, created on levels[l+1] */,
                   pdh_mg **out);
void pdh_mg_destroy(pdh_mg *mg);
int  pdh_mg_vcycle_device(pdh_mg *mg, const double *d_b, double *d_x, int zero_initial_guess);

/* Single-precision smoother matrices (pdh_shadow.hip).  A preconditioner does not need double-precision matrix entries, and the product
 * with the resident matrix is a pure read stream: pdh_set_smoother_precision(ctx, PDH_SMOOTHER_F32) builds a float32 copy - the SHADOW - of
 * the values as they stand (rows in ascending column order, zero-padded to 8 bytes) and of the block inverses pdh_setup_chebyshev just
 * built (rounded entry by entry: exactly symmetric still; the point-Jacobi inverse, one vector, stays double), on the device, without
 * reading anything back.  While F32 is in force the shadow serves the Chebyshev application wherever it runs - pdh_chebyshev_step_device,
 * PDH_PREC_CHEBYSHEV inside pdh_precondition_device and pdh_solve_cg*, the smoother of this level inside a V-cycle - and the residual of
 * this level inside a V-cycle.  Every vector, every product ((double)a * x) and every sum stays double, in the fixed orders of the double
 * kernels (no atomics: the same call on the same data gives the same bits), so the preconditioner is EXACTLY the Chebyshev polynomial /
 * V-cycle of the rounded matrices, a fixed symmetric positive operator, and CG converges to double accuracy as before.  The double matrix
 * keeps serving pdh_vmult*, pdh_residual_device, CG's own A p and b - A x, the eigenvalue estimate and the coarsest level's solver
 * (PDH_PREC_DIRECT inverts the unrounded matrix).  Levels of one hierarchy may mix precisions.
 *   Needs PDH_PREC_CHEBYSHEV set up and current on the context (else PDH_ESTATE; a context with PDH_PREC_MULTIGRID attached is PDH_ESTATE
 * too: choose the precision of every level BEFORE pdh_mg_create); any other precision value is PDH_EINVAL.  It counts as a set-up call:
 * a pdh_mg that already holds the context as a level turns stale (PDH_ESTATE naming the level).  It detaches nothing and does NOT repeat the
 * eigenvalue estimate: lambda_lo, lambda_hi and the coefficients stay those of the double set-up - rounding perturbs every entry by at most
 * 2^-24 = 6e-8 relative, and so the spectrum of P^-1 A by about as much, which the 1.2 safety factor of lambda_hi covers a million times
 * over.  PDH_SMOOTHER_F64 switches back and keeps the buffers (grow-only).  Every pdh_setup_preconditioner, pdh_setup_chebyshev and
 * pdh_setup_direct resets the precision to F64; once the values changed the staleness rules of the set-up apply (PDH_ESTATE).  Out of device
 * memory: PDH_EDEVICE, F64 stays in force and the Chebyshev set-up valid.  The shadow takes half the bytes of the values (plus half those of
 * the block inverses).
 *   What it is for: levels whose diagonal blocks are well conditioned (cond_2 far below 2^24, as on block agglomerates).  The inverse of a
 * block with cond_2 ~ 1e9 (FE_DGQ on the bounding box of a very irregular agglomerate) does not survive rounding to float32 - the call
 * succeeds, the smoother it gives is a different and possibly indefinite operator.  Point Jacobi has no such limit.
 *   pdh_smoother_precision: the one in force (< 0 on error).  pdh_smoother_vmult_device: y = A~ x, the product with the shadow on its own,
 * with the rules of pdh_vmult_device; PDH_ESTATE unless F32 is in force and current.                                                      */
#define PDH_SMOOTHER_F64 0
#define PDH_SMOOTHER_F32 1
int pdh_set_smoother_precision(pdh_ctx *ctx, int precision);
int pdh_smoother_precision(pdh_ctx *ctx);
int pdh_smoother_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y);

/* Matrix-free SIP operator (pdh_matfree.h).  On agglomerates of Cartesian cells every block of the matrix is a short sum of Kronecker
 * products of three 1-D matrices per (merged) cell or sub-face, so y = A x can be formed by sum factorisation from those 1-D matrices
 * alone - a few hundred doubles per polytope where its rows are tens of thousands - in double precision, reading no stored value.
 *   pdh_setup_matrix_free builds the tables of every owned polytope on the device, once per resident problem (a second call only fills
 * `info`); they live and die with the problem and do not depend on the values, assembled or not.  It needs a problem whose plan chose
 * the term kernels (pdh_rows_kernel_in_use == PDH_ROWS_TERMS under PDH_ALG_AUTO: 3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3, axis-aligned
 * cells with tensor rules, no PDH_EXCHANGE_GHOST, PDH_TERMS not 0); anything else is PDH_EUNSUPPORTED naming the reason.
 *   pdh_matrix_free_vmult / _device: y = A x with the vectors and rules of pdh_vmult / pdh_vmult_device (x in the global numbering, ghost
 * columns read from it; x and y disjoint, else PDH_EINVAL); PDH_ESTATE before pdh_setup_matrix_free.  A is the SIP operator of the
 * resident description as pdh_assemble_device would write it, up to rounding (another order of summation; a sub-face plane that lies on
 * a box face is taken from the box, not from a face point, which far from the origin is the more exact).  Fixed order, no atomics:
 * the same call gives the same bits.
 *   pdh_set_smoother_operator(PDH_SMOOTHER_OP_MATRIX_FREE): every product of the Chebyshev application of this context - on its own,
 * inside CG, as the smoother of this level inside a V-cycle - and the residual of this level inside a V-cycle come from the tables.
 * pdh_vmult*, pdh_residual_device, CG's own A p, the eigenvalue estimate, the block inverses and the dense gather keep reading the stored
 * values: the split pdh_set_smoother_precision makes, and orthogonal to it - with MATRIX_FREE the products ignore the shadow rows, the
 * precision still decides which block inverses the update reads.  State rules as for the precision: PDH_PREC_CHEBYSHEV set up and
 * current (else PDH_ESTATE), the tables set up (else PDH_ESTATE), no PDH_PREC_MULTIGRID attached (PDH_ESTATE: choose per level BEFORE
 * pdh_mg_create); it counts as a set-up call for a pdh_mg that holds the context; every pdh_setup_preconditioner / _chebyshev / _direct
 * goes back to STORED.  The tables are the operator of the DESCRIPTION: while the values were last written by pdh_galerkin_device, or
 * never assembled, MATRIX_FREE is PDH_ESTATE, and a later pdh_galerkin_device into the context puts it back to STORED.
 *   pdh_smoother_operator: the one in force (< 0 on error).                                                                            */
typedef struct pdh_matrix_free_info
{
  int64_t table_bytes;          /* device memory of the tables */
  int32_t doubles_per_polytope; /* stride of a polytope's record */
  int32_t max_cells, max_subfaces, max_interior_subfaces; /* of one owned polytope, after merging */
} pdh_matrix_free_info;
int pdh_setup_matrix_free(pdh_ctx *ctx, pdh_matrix_free_info *info /* may be NULL */);
int pdh_matrix_free_vmult(pdh_ctx *ctx, const double *x, double *y);             /* host pointers */
int pdh_matrix_free_vmult_device(pdh_ctx *ctx, const double *d_x, double *d_y);  /* queued on the context's stream */
#define PDH_SMOOTHER_OP_STORED 0
#define PDH_SMOOTHER_OP_MATRIX_FREE 1
int pdh_set_smoother_operator(pdh_ctx *ctx, int op);
int pdh_smoother_operator(pdh_ctx *ctx);

/* Solving on N ranks: local vectors, their halo, y = A x on them and CG by reverse communication (pdh_dist.hip, pdh_capi_dist.cpp; the
 * plan: pdh_halo_plan.cpp).  The counterpart of the reference's solve on its MPI ranks (examples/diffusion_reaction.cc:699-735).  Like the
 * exchange above the library stays transport-free: it says WHAT has to move, the caller moves it (RCCL, MPI, a copy).
 *   A rank owns the contiguous rows [row_begin, row_end) of its resident problem; row_splits [n_ranks + 1] are the first rows of all
 * ranks, ascending, row_splits[r] .. row_splits[r + 1] the range of rank r.  Ownership of a ghost comes from row_splits alone (agg_rank
 * is not read), so every description pdh_vmult serves is served: global with a row range, rank-local, col_offset, Cartesian, more than
 * 64 dofs per polytope, both layouts.  PDH_EXCHANGE_NONE only (a problem set in PDH_EXCHANGE_GHOST mode: PDH_EUNSUPPORTED).
 *   The LOCAL VECTOR of a rank has n_owned_rows + n_ghost_rows doubles: its owned rows in order, then one block of n doubles (n = dofs
 * per polytope) for every distinct ghost polytope - one whose block appears in an owned row and whose rows another rank owns -
 * ascending by first global dof.  Ranges are contiguous, so this ghost tail is grouped by owning rank in rank order: the tail IS the
 * receive buffer, recv_count[peer] doubles from every peer one after the other, and a transport receives straight into
 * d_v + n_owned_rows; nothing is unpacked.
 *   The SEND BUFFER holds one segment per peer in rank order, send_count[peer] doubles (0 for the rank itself and for peers without a
 * common face).  The segment for peer d holds the owned polytopes that have a coupled block in d's range, ascending by first global
 * dof, n doubles each, in dof order; a polytope needed by several peers appears once per peer.
 *   REQUIREMENT: the block pattern is structurally symmetric - if the rows of P hold a block of Q, the rows of Q hold a block of P (the
 * DG face-neighbour pattern is).  Then the segment rank s sends to d is exactly the part of d's ghost tail that s owns, both derived by
 * each side from its own description and row_splits: no index lists travel, as for pdh_exchange_layout.
 *   pdh_check_halo    host-only, no GPU: the per-peer sizes in doubles and pdh_halo_info for a description and its row range.  The halo
 *                     follows from the block pattern, so only the sizes, dof_offset and the face list are read and checked: a
 *                     description without its point arrays (the view pdh_set_problem_cartesian takes) is served too.
 *   pdh_halo_setup    the same for the resident problem, and builds the plan on the device (it is NOT built by pdh_set_problem*; a
 *                     second call replaces it; it is freed with the problem).
 * Both refuse with PDH_EINVAL: n_ranks < 1 or a NULL argument; row_splits that are not ascending; row_splits none of whose ranges is
 * [row_begin, row_end); row_splits that cut a polytope (a split strictly inside the n dofs of an owned or ghost polytope); a ghost
 * block outside [row_splits[0], row_splits[n_ranks]).
 *   pdh_halo_pack_device   gathers the send buffer from the owned part of d_v: whole blocks, contiguous loads and stores, no atomics;
 *                          d_send [sum send_count], asynchronous on the context's stream.  PDH_ESTATE before pdh_halo_setup.
 *   pdh_vmult_local_device y = A v for owned rows, v a local vector, y [n_owned_rows]: the arithmetic of pdh_vmult_device - per row the
 *                          same terms in the same order - with the columns found through a second block table of LOCAL positions, so
 *                          the result equals pdh_vmult_device on the same context and the same numbers TO THE BIT.  `which` selects
 *                          the polytopes whose rows are written (the others are not touched): all, the INTERIOR ones - every block
 *                          owned, no ghost value read: the work a transport overlaps with the move - or the BOUNDARY ones.
 *                          v and y must not overlap (PDH_EINVAL); PDH_ESTATE before pdh_halo_setup.                                  */
typedef struct pdh_halo_info
{
  int64_t n_owned_rows, n_ghost_rows;
  int32_t n_interior, n_boundary; /* owned polytopes */
} pdh_halo_info;
int pdh_check_halo(const pdh_problem *problem, int32_t row_begin, int32_t row_end, int n_ranks, const int32_t *row_splits,
                   int64_t *send_count /* [n_ranks] doubles */, int64_t *recv_count, pdh_halo_info *info);
int pdh_halo_setup(pdh_ctx *ctx, int n_ranks, const int32_t *row_splits, int64_t *send_count, int64_t *recv_count, pdh_halo_info *info);
int pdh_halo_pack_device(pdh_ctx *ctx, const double *d_v /* local vector */, double *d_send);
#define PDH_ROWS_ALL 0
#define PDH_ROWS_INTERIOR 1 /* owned polytopes all of whose blocks are owned: need no ghost value */
#define PDH_ROWS_BOUNDARY 2 /* the others                                                         */
int pdh_vmult_local_device(pdh_ctx *ctx, const double *d_v, double *d_y /* [n_owned_rows] */, int which);

/* Conjugate gradients over the ranks, by reverse communication: the recurrence, the stop rule and the fixed-order sums of pdh_solve_cg,
 * with the halo moves and the global sums handed to the caller.  The library never calls a transport: pdh_dcg_begin and every
 * pdh_dcg_resume return with a REQUEST in *next; the caller carries it out and calls pdh_dcg_resume, until the kind is PDH_DCG_DONE.
 * Every rank makes the same calls in the same order.
 *   HALO_BEGIN  start moving d_send (segments send_count of pdh_halo_setup) into the peers' ghost tails, this rank's being d_recv
 *               (segments recv_count); the kernels that wrote d_send are queued on the context's stream.  May return before the data
 *               has arrived: the library queues the INTERIOR product meanwhile.
 *   HALO_END    make the context's stream see the completed receive (a synchronous transport did everything at HALO_BEGIN); the
 *               library then queues the BOUNDARY product.
 *   ALLREDUCE   sum the n_scalars doubles at d_scalars (device memory, written by kernels queued on the context's stream) over all
 *               ranks, in place, with the SAME bits on every rank (e.g. added in rank order).
 * One iteration is one halo (of p), one all-reduce of p^T A p and one of (r^T z, r^T r); the start moves the halo of x0 and reduces
 * (r^T z, r^T r, b^T b).  Every rank reads the reduced ||r||^2 back, so all ranks stop in the same iteration - when ||r||_2 <=
 * max(abs_tol, rel_tol ||b||_2) over ALL rows, tested before every iteration - and at max_iter every rank gets PDH_ENOCONV (with
 * next->kind = PDH_DCG_DONE, result and x filled).  With ONE rank the sequence is the same with zero counts, and the iterates are those
 * of pdh_solve_cg_device.  d_b and d_x [n_owned_rows] are device memory, disjoint, and stay the caller's until DONE: x0 in, solution out.
 *   Preconditioners: the rank-local kinds PDH_PREC_NONE, PDH_PREC_JACOBI, PDH_PREC_BLOCK_JACOBI of pdh_setup_preconditioner (which works
 * on any row range).  PDH_PREC_CHEBYSHEV (with or without the float32 smoother or the matrix-free smoother operator), PDH_PREC_DIRECT and
 * PDH_PREC_MULTIGRID are PDH_EUNSUPPORTED naming the kind: each of their inner products would need a halo of its own.
 *   PDH_ESTATE: pdh_dcg_resume without a run (no pdh_dcg_begin, or the run ended); pdh_dcg_begin while a run is open; the halo not set
 * up; the values changed since the preconditioner was set up, or the values or the preconditioner changed during a run.  A run ends at
 * PDH_DCG_DONE, at any error return, and with the problem.                                                                             */
#define PDH_DCG_DONE 0
#define PDH_DCG_HALO_BEGIN 1
#define PDH_DCG_HALO_END 2
#define PDH_DCG_ALLREDUCE 3
typedef struct pdh_dcg_request
{
  int32_t kind;         /* PDH_DCG_*                                         */
  const double *d_send; /* HALO_BEGIN: [sum send_count]                      */
  double *d_recv;       /* HALO_BEGIN, HALO_END: the ghost tail [sum recv_count] */
  double *d_scalars;    /* ALLREDUCE                                         */
  int32_t n_scalars;    /* ALLREDUCE: 1 .. 3                                 */
} pdh_dcg_request;
int pdh_dcg_begin(pdh_ctx *ctx, const pdh_cg_control *control, const double *d_b, double *d_x, pdh_dcg_request *next);
int pdh_dcg_resume(pdh_ctx *ctx, pdh_dcg_request *next, pdh_cg_result *result /* filled at PDH_DCG_DONE */);

/* Version / build info: "polydeal_hip <version> gfx950". */
const char *pdh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* POLYDEAL_HIP_H */
