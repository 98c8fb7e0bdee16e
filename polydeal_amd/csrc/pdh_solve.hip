// pdh_solve.hip — y = A x on the resident values, the point / block Jacobi preconditioners and the vector kernels of conjugate
// gradients and of the Chebyshev smoother (C ABI: pdh_vmult*, pdh_setup_preconditioner, pdh_setup_chebyshev, pdh_precondition_device,
// pdh_chebyshev_step_device, pdh_solve_cg*; layout: pdh_solve.h).
//
// Every sum has a fixed order: a lane adds its terms in index order, a wave adds its 64 lanes by a butterfly, the slots' partials
// are added by ONE workgroup in slot order (k_cg_finalise).  No atomics: the same call on the same data gives the same bits.
#include "pdh_solve.h"
#include "pdh_launch.h"
#include "pdh_vmult_row.h"

#include <hip/hip_runtime.h>

namespace
{
using pdh_row::row_dot;
using pdh_row::W;
using pdh_row::wave_sum;
constexpr int PREC_NONE = 0, PREC_JACOBI = 1, PREC_BLOCK = 2; // PDH_PREC_* of include/polydeal_hip.h

// (wave_sum, row_part and row_dot - the arithmetic of a row - live in pdh_vmult_row.h, shared with pdh_dist.hip)

// One wave per owned polytope.  The x of its column set (its blocks in value order) is gathered into LDS once and serves all n
// rows.  Rows go two at a time (both rows' loads in flight before either is summed); the sum of row i lands in lane i % 64, whose
// 64 rows are stored together.  part: the slot's sum_i y_i x_i (own rows: ascending positions diag_L + i of the column set).
template <bool DF>
__global__ void __launch_bounds__(W) k_vmult(const PdhSolveArgs A, const double *__restrict__ x, double *__restrict__ y,
                                             double *__restrict__ part)
{
  extern __shared__ double xs[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = A.n, rl = A.row_len[s], dL = A.diag_L[s];
  const int64_t b0 = A.blk_ptr[s];
  for (int a = lane; a < rl; a += W)
    {
      const int t = a / n;
      xs[a] = x[(int64_t)A.blk_dof[b0 + t] + (a - t * n)];
    }
  __syncthreads();
  const double *__restrict__ v = A.values + A.row_base[s];
  double *__restrict__ ys = y + A.own_row[s];
  double yv = 0.0, acc = 0.0;
  for (int i = 0; i < n; i += 2)
    {
      const int i1 = i + 1 < n ? i + 1 : i; // (odd n: the last row twice, the copy is dropped)
      double s0 = row_dot<DF>(v + (int64_t)i * rl, xs, rl, dL + i, lane);
      double s1 = row_dot<DF>(v + (int64_t)i1 * rl, xs, rl, dL + i1, lane);
      s0 = wave_sum(s0);
      s1 = wave_sum(s1);
      if ((i & (W - 1)) == lane)
        yv = s0;
      if ((i1 & (W - 1)) == lane && i1 != i)
        yv = s1;
      if ((i1 & (W - 1)) == W - 1 || i1 == n - 1)
        { // rows r0 .. i1 are complete
          const int r0 = i1 & ~(W - 1);
          if (lane <= i1 - r0)
            {
              ys[r0 + lane] = yv;
              acc += yv * xs[dL + r0 + lane];
            }
        }
    }
  if (part)
    {
      acc = wave_sum(acc);
      if (lane == 0)
        part[s] = acc;
    }
}

constexpr int LD = W + 1; // LDS row stride of an n x n block (doubles)

// One wave per owned polytope (n <= 64): its diagonal block into LDS, Cholesky A = L L^T (lane r owns row r; L in the lower
// triangle, its diagonal in dg), W = L^-1 column by column (lane j solves L w = e_j and keeps w_i, i >= j, in row j's upper part),
// then A^-1 = W^T W: entry (i, j) = sum_{k >= max(i, j)} W[k][i] W[k][j], the same products in the same order for (j, i) - the
// stored inverse is exactly symmetric, so the apply may read it by columns.  flag[s] = 1: a pivot <= 0 or not finite.
template <bool DF>
__global__ void __launch_bounds__(W) k_block_inverse(const PdhSolveArgs A, double *__restrict__ dinv, int32_t *__restrict__ flag)
{
  __shared__ double M[W * LD];
  __shared__ double dg[W];
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  const int rl = A.row_len[s], dL = A.diag_L[s];
  const double *__restrict__ v = A.values + A.row_base[s];
  for (int i = 0; i < n; ++i)
    if (lane < n)
      {
        const int a = dL + lane; // ascending position of column lane of the own block
        const int k = DF ? (lane == i ? 0 : (lane < i ? a + 1 : a)) : a;
        M[i * LD + lane] = v[(int64_t)i * rl + k];
      }
  __syncthreads();
  bool bad = false;
  for (int k = 0; k < n && !bad; ++k)
    {
      const double piv = M[k * LD + k]; // the same value in every lane
      if (!(piv > 0.0) || !isfinite(piv))
        {
          bad = true;
          break;
        }
      const double d = sqrt(piv);
      if (lane > k && lane < n)
        M[lane * LD + k] /= d;
      if (lane == k)
        dg[k] = d;
      __syncthreads();
      if (lane > k && lane < n)
        {
          const double lrk = M[lane * LD + k];
          for (int j = k + 1; j <= lane; ++j)
            M[lane * LD + j] -= lrk * M[j * LD + k];
        }
      __syncthreads();
    }
  if (lane == 0)
    flag[s] = bad ? 1 : 0;
  if (bad)
    return;
  if (lane < n)
    {
      const int j = lane;
      for (int i = j; i < n; ++i)
        {
          double t = (i == j) ? 1.0 : 0.0;
          for (int k = j; k < i; ++k)
            t -= M[i * LD + k] * M[j * LD + k];
          M[j * LD + i] = t / dg[i];
        }
    }
  __syncthreads();
  double *__restrict__ out = dinv + (int64_t)s * n * n;
  for (int i = 0; i < n; ++i)
    if (lane < n)
      {
        double t = 0.0;
        for (int k = i > lane ? i : lane; k < n; ++k)
          t += M[i * LD + k] * M[lane * LD + k];
        out[(int64_t)i * n + lane] = t;
      }
}

// Point Jacobi: 1 / a_ii of every owned row; flag[s] = 1 where one of the slot's is zero or not finite
template <bool DF>
__global__ void __launch_bounds__(W) k_diag_inverse(const PdhSolveArgs A, double *__restrict__ dinv, int32_t *__restrict__ flag)
{
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  const int rl = A.row_len[s], dL = A.diag_L[s];
  const double *__restrict__ v = A.values + A.row_base[s];
  int bad = 0;
  for (int i = lane; i < n; i += W)
    {
      const double d = v[(int64_t)i * rl + (DF ? 0 : dL + i)];
      bad |= (d == 0.0 || !isfinite(d)) ? 1 : 0;
      dinv[A.own_row[s] + i] = 1.0 / d;
    }
  bad = __any(bad);
  if (lane == 0)
    flag[s] = bad ? 1 : 0;
}

// One wave per owned polytope: the vector updates of a CG step fused with z = P^-1 r and the slot's partial sums (PdhCgMode).
// r and z may be the same array in the APPLY mode (a slot's r is read before its z is written).
template <int MODE, int KIND>
__global__ void __launch_bounds__(W) k_cg_update(const PdhSolveArgs A, const double *__restrict__ dinv, const double *__restrict__ b,
                                                 const double *__restrict__ q, const double *__restrict__ p, double *__restrict__ x,
                                                 double *r, double *z, const double *__restrict__ scal, double *__restrict__ part)
{
  __shared__ double rs[W];
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  const int64_t o = A.own_row[s];
  const double alpha = MODE == PDH_UPD_STEP ? scal[PDH_CG_ALPHA] : 0.0;
  double rz = 0.0, rr = 0.0, bb = 0.0;
  for (int i0 = 0; i0 < n; i0 += W)
    {
      const int i = i0 + lane;
      const bool on = i < n;
      double ri = 0.0;
      if (on)
        {
          if (MODE == PDH_UPD_INIT)
            {
              const double bi = b[o + i];
              ri = bi - q[o + i];
              bb += bi * bi;
            }
          else if (MODE == PDH_UPD_STEP)
            {
              x[o + i] += alpha * p[o + i];
              ri = r[o + i] - alpha * q[o + i];
            }
          else
            ri = r[o + i];
        }
      double zi = ri;
      if (KIND == PREC_BLOCK)
        { // n <= 64: one pass; z_i = sum_j Dinv[j][i] r_j (= Dinv[i][j]: stored symmetric), row j read whole by the wave
          rs[lane] = ri;
          __syncthreads();
          const double *__restrict__ D = dinv + (int64_t)s * n * n + i;
          zi = 0.0;
          if (on)
            {
#pragma unroll 8
              for (int j = 0; j < n; ++j)
                zi += __builtin_nontemporal_load(D + (int64_t)j * n) * rs[j];
            }
        }
      else if (KIND == PREC_JACOBI)
        zi = on ? dinv[o + i] * ri : 0.0;
      if (on)
        {
          if (MODE != PDH_UPD_APPLY)
            r[o + i] = ri;
          z[o + i] = zi;
        }
      rz += ri * zi;
      rr += ri * ri;
    }
  if (MODE != PDH_UPD_APPLY)
    {
      rz = wave_sum(rz);
      rr = wave_sum(rr);
      bb = wave_sum(bb);
      if (lane == 0)
        {
          part[PDH_PART_RZ * (int64_t)A.n_owned + s] = rz;
          part[PDH_PART_RR * (int64_t)A.n_owned + s] = rr;
          if (MODE == PDH_UPD_INIT)
            part[PDH_PART_BB * (int64_t)A.n_owned + s] = bb;
        }
    }
}

// One wave per owned polytope: one step of the Chebyshev chain of pdh_setup_chebyshev (same slot walk as k_cg_update),
//   r <- FIRST ? b (- q if the start is not zero) : r - q;   z = P^-1 r;   d <- FIRST ? c2 z : c1 d + c2 z;   x <- x + d
// (FIRST from a zero start: x <- d, x is not read).  q = A x0 (FIRST) or A d of the previous step, by k_vmult.  b and x may be the
// same array (a slot's b is read before its x is written).  rcg (may be NULL; may be b): the slot's partial of rcg^T x goes to
// part[PDH_PART_RZ] - the last step of an application inside CG, so that k_cg_finalise stays the one place where partials are added.
template <bool FIRST, int KIND>
__global__ void __launch_bounds__(W) k_cheb_update(const PdhSolveArgs A, const double *__restrict__ dinv, const double *b,
                                                   const double *__restrict__ q, double *__restrict__ d, double *__restrict__ r, double *x,
                                                   double c1, double c2, int zero_start, const double *rcg, double *__restrict__ part)
{
  __shared__ double rs[W];
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  const int64_t o = A.own_row[s];
  double rz = 0.0;
  for (int i0 = 0; i0 < n; i0 += W)
    {
      const int i = i0 + lane;
      const bool on = i < n;
      double ri = 0.0;
      if (on)
        {
          if (FIRST)
            ri = q ? b[o + i] - q[o + i] : b[o + i];
          else
            ri = r[o + i] - q[o + i];
        }
      double zi = 0.0;
      if (KIND == PREC_BLOCK)
        { // n <= 64: one pass; row j of the symmetric inverse read whole by the wave, as in k_cg_update
          rs[lane] = ri;
          __syncthreads();
          const double *__restrict__ D = dinv + (int64_t)s * n * n + i;
          if (on)
            {
#pragma unroll 8
              for (int j = 0; j < n; ++j)
                zi += __builtin_nontemporal_load(D + (int64_t)j * n) * rs[j];
            }
        }
      else
        zi = on ? dinv[o + i] * ri : 0.0;
      if (on)
        {
          const double di = FIRST ? c2 * zi : c1 * d[o + i] + c2 * zi;
          const double xi = (FIRST && zero_start) ? di : x[o + i] + di;
          r[o + i] = ri;
          d[o + i] = di;
          x[o + i] = xi;
          if (rcg)
            rz += rcg[o + i] * xi;
        }
    }
  if (rcg)
    {
      rz = wave_sum(rz);
      if (lane == 0)
        part[PDH_PART_RZ * (int64_t)A.n_owned + s] = rz;
    }
}

__global__ void __launch_bounds__(256) k_cg_direction(int64_t N, int init, const double *__restrict__ z, double *__restrict__ p,
                                                      const double *__restrict__ scal)
{
  const double beta = init ? 0.0 : scal[PDH_CG_BETA];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    p[i] = init ? z[i] : z[i] + beta * p[i];
}

// The two halves of turning partials into scalars.  cg_local_sum - one workgroup: thread t adds the partials t, t + 256, ... in order,
// then a fixed tree over the 256 threads; the (up to three) sums of the stage are left in red[c][0].  cg_finish - one thread: the
// scalars of the stage from its sums.  One rank runs both in one kernel (k_cg_finalise); over several ranks the sums of all ranks are
// added between the two (k_cg_local_sum, the caller's all-reduce, k_cg_finish: pdh_dcg_*).
__device__ __forceinline__ void cg_local_sum(const double *__restrict__ part, int n_owned, int stage, double (*red)[256])
{
  const int t = threadIdx.x;
  const int rows[3][3] = {{PDH_PART_RZ, PDH_PART_RR, PDH_PART_BB}, {PDH_PART_PQ, -1, -1}, {PDH_PART_RZ, PDH_PART_RR, -1}};
  for (int c = 0; c < 3; ++c)
    {
      const int row = rows[stage][c];
      double acc = 0.0;
      if (row >= 0)
        for (int k = t; k < n_owned; k += 256)
          acc += part[(int64_t)row * n_owned + k];
      red[c][t] = acc;
    }
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1)
    {
      if (t < h)
        for (int c = 0; c < 3; ++c)
          red[c][t] += red[c][t + h];
      __syncthreads();
    }
}

__device__ __forceinline__ void cg_finish(int stage, double s0, double s1, double s2, double *__restrict__ scal)
{
  if (stage == 0)
    {
      scal[PDH_CG_RZ] = s0;
      scal[PDH_CG_RR] = s1;
      scal[PDH_CG_BB] = s2;
    }
  else if (stage == 1)
    {
      scal[PDH_CG_PQ] = s0;
      scal[PDH_CG_ALPHA] = s0 != 0.0 ? scal[PDH_CG_RZ] / s0 : 0.0;
    }
  else
    {
      const double rz0 = scal[PDH_CG_RZ];
      scal[PDH_CG_BETA] = rz0 != 0.0 ? s0 / rz0 : 0.0;
      scal[PDH_CG_RZ] = s0;
      scal[PDH_CG_RR] = s1;
    }
}

__global__ void __launch_bounds__(256) k_cg_finalise(const double *__restrict__ part, int n_owned, int stage, double *__restrict__ scal)
{
  __shared__ double red[3][256];
  cg_local_sum(part, n_owned, stage, red);
  if (threadIdx.x == 0)
    cg_finish(stage, red[0][0], red[1][0], red[2][0], scal);
}

// sums [3]: the stage's local sums (unused ones 0)
__global__ void __launch_bounds__(256) k_cg_local_sum(const double *__restrict__ part, int n_owned, int stage, double *__restrict__ sums)
{
  __shared__ double red[3][256];
  cg_local_sum(part, n_owned, stage, red);
  if (threadIdx.x < 3)
    sums[threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(64) k_cg_finish(int stage, const double *__restrict__ sums, double *__restrict__ scal)
{
  if (threadIdx.x == 0)
    cg_finish(stage, sums[0], sums[1], sums[2], scal);
}
} // namespace

extern "C" hipError_t pdh_launch_vmult(const PdhSolveArgs *A, const double *x, double *y, double *part, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  const size_t lds = (size_t)A->max_row_len * sizeof(double);
  if (A->diag_first)
    hipLaunchKernelGGL(k_vmult<true>, dim3(A->n_owned), dim3(W), lds, stream, *A, x, y, part);
  else
    hipLaunchKernelGGL(k_vmult<false>, dim3(A->n_owned), dim3(W), lds, stream, *A, x, y, part);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_block_inverse(const PdhSolveArgs *A, double *dinv, int32_t *flag, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if (A->n > W)
    return hipErrorInvalidValue;
  if (A->diag_first)
    hipLaunchKernelGGL(k_block_inverse<true>, dim3(A->n_owned), dim3(W), 0, stream, *A, dinv, flag);
  else
    hipLaunchKernelGGL(k_block_inverse<false>, dim3(A->n_owned), dim3(W), 0, stream, *A, dinv, flag);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_diag_inverse(const PdhSolveArgs *A, double *dinv, int32_t *flag, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if (A->diag_first)
    hipLaunchKernelGGL(k_diag_inverse<true>, dim3(A->n_owned), dim3(W), 0, stream, *A, dinv, flag);
  else
    hipLaunchKernelGGL(k_diag_inverse<false>, dim3(A->n_owned), dim3(W), 0, stream, *A, dinv, flag);
  return hipGetLastError();
}

template <int MODE>
static void launch_update(const PdhSolveArgs *A, int kind, const double *dinv, const double *b, const double *q, const double *p,
                          double *x, double *r, double *z, const double *scal, double *part, hipStream_t stream)
{
  const dim3 g(A->n_owned), blk(W);
  if (kind == PREC_BLOCK)
    hipLaunchKernelGGL((k_cg_update<MODE, PREC_BLOCK>), g, blk, 0, stream, *A, dinv, b, q, p, x, r, z, scal, part);
  else if (kind == PREC_JACOBI)
    hipLaunchKernelGGL((k_cg_update<MODE, PREC_JACOBI>), g, blk, 0, stream, *A, dinv, b, q, p, x, r, z, scal, part);
  else
    hipLaunchKernelGGL((k_cg_update<MODE, PREC_NONE>), g, blk, 0, stream, *A, dinv, b, q, p, x, r, z, scal, part);
}

extern "C" hipError_t pdh_launch_cg_update(const PdhSolveArgs *A, int mode, int kind, const double *dinv, const double *b,
                                           const double *q, const double *p, double *x, double *r, double *z, const double *scal,
                                           double *part, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if (kind == PREC_BLOCK && A->n > W)
    return hipErrorInvalidValue;
  if (mode == PDH_UPD_INIT)
    launch_update<PDH_UPD_INIT>(A, kind, dinv, b, q, p, x, r, z, scal, part, stream);
  else if (mode == PDH_UPD_STEP)
    launch_update<PDH_UPD_STEP>(A, kind, dinv, b, q, p, x, r, z, scal, part, stream);
  else
    launch_update<PDH_UPD_APPLY>(A, kind, dinv, b, q, p, x, r, z, scal, part, stream);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_cg_direction(int64_t n_rows, int init, const double *z, double *p, const double *scal, hipStream_t stream)
{
  if (n_rows <= 0)
    return hipSuccess;
  const int64_t blocks = (n_rows + 255) / 256;
  hipLaunchKernelGGL(k_cg_direction, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, n_rows, init, z, p, scal);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_cg_finalise(const double *part, int n_owned, int stage, double *scal, hipStream_t stream)
{
  if (stage < 0 || stage > 2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cg_finalise, dim3(1), dim3(256), 0, stream, part, n_owned, stage, scal);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_cg_local_sum(const double *part, int n_owned, int stage, double *sums, hipStream_t stream)
{
  if (stage < 0 || stage > 2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cg_local_sum, dim3(1), dim3(256), 0, stream, part, n_owned, stage, sums);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_cg_finish(int stage, const double *sums, double *scal, hipStream_t stream)
{
  if (stage < 0 || stage > 2)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(64), 0, stream, stage, sums, scal);
  return hipGetLastError();
}

template <bool FIRST>
static void launch_cheb(const PdhSolveArgs *A, int kind, const double *dinv, const double *b, const double *q, double *d, double *r,
                        double *x, double c1, double c2, int zero_start, const double *rcg, double *part, hipStream_t stream)
{
  const dim3 g(A->n_owned), blk(W);
  if (kind == PREC_BLOCK)
    hipLaunchKernelGGL((k_cheb_update<FIRST, PREC_BLOCK>), g, blk, 0, stream, *A, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part);
  else
    hipLaunchKernelGGL((k_cheb_update<FIRST, PREC_JACOBI>), g, blk, 0, stream, *A, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part);
}

extern "C" hipError_t pdh_launch_cheb_update(const PdhSolveArgs *A, int first, int kind, const double *dinv, const double *b,
                                             const double *q, double *d, double *r, double *x, double c1, double c2, int zero_start,
                                             const double *rcg, double *part, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if ((kind != PREC_BLOCK && kind != PREC_JACOBI) || (kind == PREC_BLOCK && A->n > W) || (!first && !q) || (rcg && !part))
    return hipErrorInvalidValue;
  if (first)
    launch_cheb<true>(A, kind, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part, stream);
  else
    launch_cheb<false>(A, kind, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part, stream);
  return hipGetLastError();
}
