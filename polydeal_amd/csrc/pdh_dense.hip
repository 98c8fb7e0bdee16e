// pdh_dense.hip — the dense direct solve on the resident matrix (layout and the steps of the set-up: pdh_dense.h; C ABI:
// pdh_setup_direct, PDH_PREC_DIRECT of pdh_precondition_device and pdh_solve_cg*).
//
// As in pdh_solve.hip every sum has a fixed order - a thread adds its terms in index order, a wave adds its 64 lanes by a butterfly -
// and nothing is atomic: the same call on the same data gives the same bits.
#include "pdh_dense.h"
#include "pdh_launch.h"
#include "pdh_solve.h"

#include <hip/hip_runtime.h>

namespace
{
constexpr int W = PDH_DENSE_TILE;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int m = W / 2; m > 0; m >>= 1)
    v += __shfl_xor(v, m, W);
  return v;
}

// One wave per owned polytope: its n rows into the dense array D [ld][ld] (zeroed by the caller).  The value at position k of row i
// holds ascending position a(k) of the column set (pdh_solve.h; diagonal first: k = 0 -> diag_L + i, 1 <= k <= diag_L + i -> k - 1),
// column blk_dof[blk_ptr[s] + a / n] + a % n; the row is own_row[s] + i.  Nothing outside [0, N) x [0, N) is written.
template <bool DF>
__global__ void __launch_bounds__(W) k_dense_gather(const PdhSolveArgs A, double *__restrict__ D, int ld, int N)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = A.n, rl = A.row_len[s], dL = A.diag_L[s];
  const int64_t b0 = A.blk_ptr[s];
  const double *__restrict__ v = A.values + A.row_base[s];
  const int row0 = A.own_row[s];
  for (int i = 0; i < n; ++i)
    {
      const int row = row0 + i, di = dL + i;
      for (int k = lane; k < rl; k += W)
        {
          const int a = DF ? (k == 0 ? di : (k <= di ? k - 1 : k)) : k;
          const int t = a / n;
          const int col = A.blk_dof[b0 + t] + (a - t * n);
          if (row >= 0 && row < N && col >= 0 && col < N)
            D[(int64_t)row * ld + col] = v[(int64_t)i * rl + k];
        }
    }
}

// ONE workgroup of ld threads, thread c owns column c of U = L^T (coalesced: a wave touches 64 neighbours of one row).  Right-looking:
// step k reads the pivot p = U[k][k] (the same value in every thread), scales row k by 1 / sqrt(p) and subtracts u_kc u_kj from
// U[j][c], k < j <= c - thread c's terms in ascending k.  Rows and columns N .. ld - 1 are made the identity's first.  A pivot <= 0 or not
// finite ends the loop in every thread at once: flag[0] = k + 1 (else 0).  piv[0] / piv[1]: the smallest / largest pivot of rows < N.
__global__ void __launch_bounds__(PDH_DENSE_MAX_ROWS) k_dense_cholesky(double *U, int ld, int N, double *__restrict__ dg,
                                                                       double *__restrict__ piv, int32_t *__restrict__ flag)
{
  const int c = threadIdx.x;
  if (c >= N)
    U[(int64_t)c * ld + c] = 1.0;
  __syncthreads();
  double pmin = __builtin_huge_val(), pmax = 0.0;
  int bad = 0;
  for (int k = 0; k < ld; ++k)
    {
      const double p = U[(int64_t)k * ld + k];
      if (!(p > 0.0) || !isfinite(p))
        {
          bad = k + 1;
          break;
        }
      if (k < N)
        {
          pmin = p < pmin ? p : pmin;
          pmax = p > pmax ? p : pmax;
        }
      const double d = sqrt(p);
      double u = 0.0;
      if (c == k)
        dg[k] = d;
      if (c > k)
        {
          u = U[(int64_t)k * ld + c] / d;
          U[(int64_t)k * ld + c] = u;
        }
      __syncthreads();
      {
        const double *__restrict__ rk = U + (int64_t)k * ld; // row k: complete, read only from here on
        double *__restrict__ col = U + c;                    // rows k + 1 .. c of the own column
#pragma unroll 4
        for (int j = k + 1; j <= c; ++j)
          col[(int64_t)j * ld] -= u * rk[j];
      }
      __syncthreads();
    }
  if (c == 0)
    {
      flag[0] = bad;
      piv[0] = pmin;
      piv[1] = pmax;
    }
}

// Thread j solves L w = e_j by forward substitution and stores w as column j of Wd [ld][ld]: w_i = (delta_ij - sum_k L[i][k] w_k) /
// L[i][i], k ascending from the first column of the thread's wave (w_k = 0 for k < j, written as such), L[i][k] = U[k][i].  A thread
// reads only what it wrote itself.
__global__ void __launch_bounds__(W) k_dense_tri_inverse(const double *__restrict__ U, const double *__restrict__ dg, int ld, double *Wd)
{
  const int j0 = blockIdx.x * W, j = j0 + threadIdx.x;
  for (int i = j0; i < ld; ++i)
    {
      double t = i == j ? 1.0 : 0.0;
#pragma unroll 4
      for (int k = j0; k < i; ++k)
        t -= U[(int64_t)k * ld + i] * Wd[(int64_t)k * ld + j];
      Wd[(int64_t)i * ld + j] = i >= j ? t / dg[i] : 0.0;
    }
}

// G = W^T W: block (bx, j), lane i = 64 bx + lane, entry (i, j) for i >= j = sum_k Wd[k][i] Wd[k][j], k ascending from
// max(64 bx, j) (Wd[k][i] = 0 for k < i), stored at (i, j) and at (j, i)
__global__ void __launch_bounds__(W) k_dense_gram(const double *__restrict__ Wd, int ld, double *__restrict__ G)
{
  const int i0 = blockIdx.x * W, i = i0 + threadIdx.x, j = blockIdx.y;
  if (i0 + W - 1 < j)
    return;
  double t = 0.0;
#pragma unroll 4
  for (int k = i0 > j ? i0 : j; k < ld; ++k)
    t += Wd[(int64_t)k * ld + i] * Wd[(int64_t)k * ld + j];
  if (i >= j)
    {
      G[(int64_t)i * ld + j] = t;
      G[(int64_t)j * ld + i] = t;
    }
}

// z = G r.  One wave per owned polytope (the slot walk of k_vmult): r into LDS once (zeros from N on), then the slot's n rows, each
// read as ld / 64 whole 512-byte pieces; a lane adds its terms in index order, the wave its lanes by the butterfly, the sum of row i
// lands in lane i % 64 and 64 rows are stored together.  r and z must not overlap (the caller copies r for the in-place call).
// rcg (may be NULL): the slot's partial of rcg^T z goes to part[PDH_PART_RZ], as in k_cheb_update.
__global__ void __launch_bounds__(W) k_dense_symv(const PdhSolveArgs A, const double *__restrict__ G, int ld, int N,
                                                  const double *__restrict__ r, double *__restrict__ z, const double *rcg,
                                                  double *__restrict__ part)
{
  extern __shared__ double rs[];
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  for (int a = lane; a < ld; a += W)
    rs[a] = a < N ? r[a] : 0.0;
  __syncthreads();
  const int o = A.own_row[s];
  const int np = ld / W;
  double acc = 0.0, zv = 0.0;
  if (o >= 0 && o + n <= N)
    for (int i = 0; i < n; ++i)
      {
        const double *__restrict__ g = G + (int64_t)(o + i) * ld + lane;
        double sum = 0.0;
#pragma unroll 4
        for (int u = 0; u < np; ++u)
          sum += g[u * W] * rs[u * W + lane];
        sum = wave_sum(sum);
        if ((i & (W - 1)) == lane)
          zv = sum;
        if ((i & (W - 1)) == W - 1 || i == n - 1)
          {
            const int r0 = i & ~(W - 1);
            if (lane <= i - r0)
              {
                z[o + r0 + lane] = zv;
                if (rcg)
                  acc += rcg[o + r0 + lane] * zv;
              }
          }
      }
  if (rcg)
    {
      acc = wave_sum(acc);
      if (lane == 0)
        part[PDH_PART_RZ * (int64_t)A.n_owned + s] = acc;
    }
}

bool dense_size_ok(int ld, int N) { return N >= 1 && N <= PDH_DENSE_MAX_ROWS && ld == pdh_dense_ld(N); }
} // namespace

extern "C" hipError_t pdh_launch_dense_gather(const PdhSolveArgs *A, double *D, int ld, int n_rows, hipStream_t stream)
{
  if (!dense_size_ok(ld, n_rows))
    return hipErrorInvalidValue;
  if (A->n_owned <= 0)
    return hipSuccess;
  if (A->diag_first)
    hipLaunchKernelGGL(k_dense_gather<true>, dim3(A->n_owned), dim3(W), 0, stream, *A, D, ld, n_rows);
  else
    hipLaunchKernelGGL(k_dense_gather<false>, dim3(A->n_owned), dim3(W), 0, stream, *A, D, ld, n_rows);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_dense_cholesky(double *U, int ld, int n_rows, double *dg, double *piv, int32_t *flag, hipStream_t stream)
{
  if (!dense_size_ok(ld, n_rows))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dense_cholesky, dim3(1), dim3(ld), 0, stream, U, ld, n_rows, dg, piv, flag);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_dense_inverse(const double *U, const double *dg, int ld, int n_rows, double *Wd, double *G, hipStream_t stream)
{
  if (!dense_size_ok(ld, n_rows))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dense_tri_inverse, dim3(ld / W), dim3(W), 0, stream, U, dg, ld, Wd);
  hipLaunchKernelGGL(k_dense_gram, dim3(ld / W, ld), dim3(W), 0, stream, Wd, ld, G);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_dense_symv(const PdhSolveArgs *A, const double *G, int ld, int n_rows, const double *r, double *z,
                                            const double *rcg, double *part, hipStream_t stream)
{
  if (!dense_size_ok(ld, n_rows) || (rcg && !part))
    return hipErrorInvalidValue;
  if (A->n_owned <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_dense_symv, dim3(A->n_owned), dim3(W), (size_t)ld * sizeof(double), stream, *A, G, ld, n_rows, r, z, rcg, part);
  return hipGetLastError();
}
