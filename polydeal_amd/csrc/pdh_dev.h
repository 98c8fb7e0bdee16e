// pdh_dev.h — what the host (pdh_plan.cpp, pdh_capi.cpp) and the kernels (pdh_kernels.h) must agree on, as plain data and
// integer arithmetic: compiles with and without HIP.  The layout headers of the kernel families (pdh_rows_tables.h,
// pdh_terms_tables.h, pdh_moment_tables.h) build on it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define PDH_MAX_N1D 8
#define PDH_WAVE 64

// functions the host and the kernels both evaluate
#if defined(__HIPCC__)
#define PDH_HD __host__ __device__
#else
#define PDH_HD
#endif

struct PdhBasisTab
{
  double coef[PDH_MAX_N1D][PDH_MAX_N1D]; // coef[k][m]: monomial coefficients of 1-D basis function k
};

struct PdhDev
{
  int32_t dim, n, n1d, diag_first;
  double reaction_c;
  const double *bbox;   // [n_agg][2][dim]
  const int32_t *midx;  // [16*NT] packed multi-index (k0 | k1<<8 | k2<<16), 0xffffffff = dead
  // volume quadrature of the owned polytopes (SoA), indexed by owned slot
  const int64_t *vq_ptr;
  const double *vq_x;
  int64_t vq_stride;
  const double *vq_w;
  // own-side face points, packed per owned polytope
  const int64_t *ap_ptr; // [n_owned+1]
  const double *ap_x;    // [dim][P]
  const double *ap_n;    // [dim][P] outward normal of the owning polytope
  int64_t ap_stride;
  const double *ap_wself;  // [P] JxW used by the diagonal block (2 JxW on the boundary)
  const double *ap_wcross; // [P] JxW used by the coupling block (JxW of side 1)
  const double *ap_sig;    // [P] sigma (sigma/2 on the boundary)
  // diagonal-block items
  const int32_t *own_agg;  // [n_owned]
  const int64_t *row_base; // [n_owned] value offset of the polytope's first row
  const int32_t *row_len;  // [n_owned] entries per row
  const int32_t *diag_L;   // [n_owned] ascending column position of the own block inside the row
  const int32_t *own_row;  // [n_owned] first dof row of the polytope, relative to the owned row range
  // coupling-block items: one per interior face with at least one owned side
  const int32_t *it_own;  // owned slot of P (the side whose packed points are used)
  const int32_t *it_nbr;  // neighbour polytope id Q
  const int64_t *it_pbeg; // first packed point
  const int32_t *it_pcnt; // number of points
  const int32_t *it_pos;  // position of Q's block inside P's rows (diag-first shift included)
  const int32_t *it_nbr_slot; // owned slot of Q, or -1: A[Q,P] = A[P,Q]^T is then not written here
  const int32_t *it_pos_t;    // position of P's block inside Q's rows
  double *values;
  PdhBasisTab tab;
};

namespace pdh
{
// LDS bytes needed by the two kernels of pdh_kernels.h (host side helper).
inline size_t lds_bytes_diag(int dim, int n1d, int nt)
{
  const size_t recs = (size_t)(nt >= 3 ? PDH_WAVE : 32) * (dim * n1d * 2 + 2 + 2 + dim) * sizeof(double); // CH-point chunks
  const size_t strip = (size_t)16 * (16 * nt + 2) * sizeof(double);
  return recs > strip ? recs : strip;
}
inline size_t lds_bytes_offdiag(int dim, int n1d, int nt)
{
  const size_t recs = (size_t)32 * (2 * (dim * n1d * 2 + 2) + 2 + dim) * sizeof(double); // 32-point chunks
  const size_t strip = (size_t)16 * (16 * nt + 2) * sizeof(double);
  return recs > strip ? recs : strip;
}
// more than 64 dofs per polytope: is there a tiled kernel (pdh_tiled.h) for this element?
inline bool tiled_has_kind(int dim, int n1d, int n) { return dim == 3 && n1d >= 5 && n1d <= 8 && n > 64; }
} // namespace pdh
