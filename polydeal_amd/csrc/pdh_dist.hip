// pdh_dist.hip — the kernels of solving over several ranks (C ABI: pdh_halo_pack_device, pdh_vmult_local_device, pdh_dcg_*; layout
// and plan: pdh_dist.h): the gather of the halo send buffer and y = A v on a rank's LOCAL vector (owned rows, then the ghost blocks).
//
// k_vmult_local is k_vmult (pdh_solve.hip) with two indirections: the slot comes from a list (all, interior or boundary polytopes) and
// the columns from a block table of local positions.  The arithmetic of a row is the shared one of pdh_vmult_row.h, so the result
// equals k_vmult's to the bit.  No atomics anywhere.
#include "pdh_dist.h"
#include "pdh_launch.h"
#include "pdh_vmult_row.h"

#include <hip/hip_runtime.h>

namespace
{
using pdh_row::row_dot;
using pdh_row::W;
using pdh_row::wave_sum;

// L lanes per (peer, polytope) block, 256 / L blocks per workgroup: lane l of a block copies the entries l, l + L, ... - contiguous
// loads and stores within the block.  src[b]: first entry of block b in the owned part of v.
template <int L>
__global__ void __launch_bounds__(256) k_halo_pack(int n, int64_t n_blocks, const int64_t *__restrict__ src, const double *__restrict__ v,
                                                   double *__restrict__ send)
{
  const int64_t b = ((int64_t)blockIdx.x * 256 + threadIdx.x) / L;
  const int l = threadIdx.x % L;
  if (b >= n_blocks)
    return;
  const double *__restrict__ from = v + src[b];
  double *__restrict__ to = send + b * n;
  for (int i = l; i < n; i += L)
    to[i] = from[i];
}

// One wave per listed slot; see k_vmult for the walk.  A.blk_dof holds local positions.
template <bool DF>
__global__ void __launch_bounds__(W) k_vmult_local(const PdhSolveArgs A, const int32_t *__restrict__ slots, const double *__restrict__ x,
                                                   double *__restrict__ y, double *__restrict__ part)
{
  extern __shared__ double xs[];
  const int s = slots[blockIdx.x], lane = threadIdx.x;
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
} // namespace

extern "C" hipError_t pdh_launch_halo_pack(int n, int64_t n_blocks, const int64_t *src, const double *v, double *send, hipStream_t stream)
{
  if (n_blocks <= 0)
    return hipSuccess;
  if (n < 1)
    return hipErrorInvalidValue;
  const int L = n > 32 ? 64 : n > 16 ? 32 : n > 8 ? 16 : n > 4 ? 8 : 4;
  const int64_t groups = (n_blocks * L + 255) / 256;
  if (groups > 0x7fffffff)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)groups), blk(256);
  switch (L)
    {
    case 64: hipLaunchKernelGGL(k_halo_pack<64>, g, blk, 0, stream, n, n_blocks, src, v, send); break;
    case 32: hipLaunchKernelGGL(k_halo_pack<32>, g, blk, 0, stream, n, n_blocks, src, v, send); break;
    case 16: hipLaunchKernelGGL(k_halo_pack<16>, g, blk, 0, stream, n, n_blocks, src, v, send); break;
    case 8: hipLaunchKernelGGL(k_halo_pack<8>, g, blk, 0, stream, n, n_blocks, src, v, send); break;
    default: hipLaunchKernelGGL(k_halo_pack<4>, g, blk, 0, stream, n, n_blocks, src, v, send); break;
    }
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_vmult_local(const PdhSolveArgs *A, const int32_t *slots, int n_slots, const double *v, double *y,
                                             double *part, hipStream_t stream)
{
  if (n_slots <= 0)
    return hipSuccess;
  const size_t lds = (size_t)A->max_row_len * sizeof(double);
  if (A->diag_first)
    hipLaunchKernelGGL(k_vmult_local<true>, dim3(n_slots), dim3(W), lds, stream, *A, slots, v, y, part);
  else
    hipLaunchKernelGGL(k_vmult_local<false>, dim3(n_slots), dim3(W), lds, stream, *A, slots, v, y, part);
  return hipGetLastError();
}
