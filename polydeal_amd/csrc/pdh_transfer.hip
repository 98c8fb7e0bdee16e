// pdh_transfer.hip — level transfers between two nested polytopal FE_DGQ spaces (C ABI: pdh_prolongate*, pdh_restrict*; layout:
// pdh_transfer.h) and the subtraction of pdh_residual_device.  The injection block of a fine polytope is a Kronecker product of `dim`
// 1-D matrices: both kernels apply them axis by axis through LDS, one N1D-term sum per lane and pass.  A transfer is one pass over
// the two vectors plus dim N1D^2 doubles per fine polytope - no n x n block is stored or streamed.
//
// Every sum has a fixed order: a lane adds its N1D terms in index order, the restriction adds the children of a coarse polytope in
// the order of the children CSR (ascending fine index).  No atomics: the same call on the same data gives the same bits.
#include "pdh_transfer.h"
#include "pdh_launch.h"

#include <hip/hip_runtime.h>

namespace
{
constexpr int W = 64;
constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

// How a wave is cut: polytopes of up to 64 dofs share it (G of them, so that n = 4 .. 27 do not idle most lanes), larger ones take
// it in NCH chunks of 64 lanes.  A slot is one dof of one of the wave's polytopes: slot = g * n + i.
template <int DIM, int N1D>
struct Cut
{
  static constexpr int n = ipow(N1D, DIM);
  static constexpr int G = n >= W ? 1 : W / n;
  static constexpr int NCH = (n + W - 1) / W;
  static constexpr int SLOTS = G * n;
  static constexpr int TAB = DIM * N1D * N1D; // the 1-D matrices of one fine polytope
};

// the 1-D matrices of the wave's fine polytopes pol[g] (-1: none, zeros) into LDS
template <int DIM, int N1D>
__device__ __forceinline__ void load_tables(const PdhTransferArgs &A, const int32_t *pol, double *tb, int lane)
{
  using C = Cut<DIM, N1D>;
  for (int e = lane; e < C::G * C::TAB; e += W)
    {
      const int g = e / C::TAB, F = pol[g];
      tb[e] = F >= 0 ? A.tab[(int64_t)F * C::TAB + (e - g * C::TAB)] : 0.0;
    }
}

// One wave per G fine polytopes; lanes are fine dofs.  The parent's n coefficients and the polytope's tables go to LDS, then one
// pass per axis: out[.., i_c, ..] = sum_j B_c[i_c][j] in[.., j, ..].  The last pass writes fine[off_F + i] (ADD: adds to it).
template <int DIM, int N1D, bool ADD>
__global__ void __launch_bounds__(W) k_prolongate(const PdhTransferArgs A, const double *__restrict__ coarse, double *__restrict__ fine)
{
  using C = Cut<DIM, N1D>;
  __shared__ double u[2][C::SLOTS];
  __shared__ double tb[C::G * C::TAB];
  __shared__ int32_t pol[C::G];
  const int lane = threadIdx.x;
  if (lane < C::G)
    {
      const int64_t F = (int64_t)blockIdx.x * C::G + lane;
      pol[lane] = F < A.n_fine ? (int32_t)F : -1;
    }
  __syncthreads();
  load_tables<DIM, N1D>(A, pol, tb, lane);
#pragma unroll
  for (int k = 0; k < C::NCH; ++k)
    {
      const int slot = lane + k * W;
      if (slot < C::SLOTS)
        {
          const int g = slot / C::n, i = slot - g * C::n, F = pol[g];
          u[0][slot] = F >= 0 ? coarse[(int64_t)A.coarse_off[A.parent[F]] + i] : 0.0;
        }
    }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < DIM; ++c)
    {
      const int stride = ipow(N1D, c);
      const double *in = u[c & 1];
      double *out = u[(c & 1) ^ 1];
#pragma unroll
      for (int k = 0; k < C::NCH; ++k)
        {
          const int slot = lane + k * W;
          if (slot < C::SLOTS)
            {
              const int g = slot / C::n, i = slot - g * C::n;
              const int ic = (i / stride) % N1D;
              const double *B = tb + g * C::TAB + (c * N1D + ic) * N1D;
              const double *col = in + (slot - ic * stride);
              double sum = 0.0;
#pragma unroll
              for (int j = 0; j < N1D; ++j)
                sum += B[j] * col[j * stride];
              if (c < DIM - 1)
                out[slot] = sum;
              else
                {
                  const int F = pol[g];
                  if (F >= 0)
                    {
                      double *dst = fine + (int64_t)A.fine_off[F] + i;
                      *dst = ADD ? *dst + sum : sum;
                    }
                }
            }
        }
      if (c < DIM - 1)
        __syncthreads();
    }
}

// One wave per G coarse polytopes; lanes are coarse dofs.  The children are taken in CSR order: a child's n values and tables go to LDS,
// the transposed 1-D matrices are applied axis by axis, out[.., j_c, ..] = sum_i B_c[i][j_c] in[.., i, ..], and the result is added to
// the lane's accumulator.  One store (ADD: add) per coarse dof at the end.
template <int DIM, int N1D, bool ADD>
__global__ void __launch_bounds__(W) k_restrict(const PdhTransferArgs A, const double *__restrict__ fine, double *__restrict__ coarse)
{
  using C = Cut<DIM, N1D>;
  __shared__ double u[2][C::SLOTS];
  __shared__ double tb[C::G * C::TAB];
  __shared__ int32_t pol[C::G];
  const int lane = threadIdx.x;
  // the lane's group and dof are the same in every chunk (n > 64: one group)
  const int g = C::NCH > 1 ? 0 : lane / C::n;
  const int i0 = C::NCH > 1 ? lane : lane - g * C::n;
  const int64_t P = (int64_t)blockIdx.x * C::G + g;
  const bool on = g < C::G && P < A.n_coarse;
  const int begin = on ? A.child_ptr[P] : 0;
  const int n_children = on ? A.child_ptr[P + 1] - begin : 0;
  double acc[C::NCH];
#pragma unroll
  for (int k = 0; k < C::NCH; ++k)
    acc[k] = 0.0;
  for (int t = 0; __any(t < n_children); ++t)
    {
      const int F = t < n_children ? A.child_idx[begin + t] : -1;
      if (i0 == 0 && g < C::G)
        pol[g] = F;
      __syncthreads();
      load_tables<DIM, N1D>(A, pol, tb, lane);
#pragma unroll
      for (int k = 0; k < C::NCH; ++k)
        {
          const int slot = lane + k * W;
          if (slot < C::SLOTS)
            u[0][slot] = F >= 0 ? fine[(int64_t)A.fine_off[F] + i0 + k * W] : 0.0;
        }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < DIM; ++c)
        {
          const int stride = ipow(N1D, c);
          const double *in = u[c & 1];
          double *out = u[(c & 1) ^ 1];
#pragma unroll
          for (int k = 0; k < C::NCH; ++k)
            {
              const int slot = lane + k * W;
              if (slot < C::SLOTS)
                {
                  const int j = i0 + k * W;
                  const int jc = (j / stride) % N1D;
                  const double *B = tb + g * C::TAB + c * N1D * N1D + jc;
                  const double *col = in + (slot - jc * stride);
                  double sum = 0.0;
#pragma unroll
                  for (int i = 0; i < N1D; ++i)
                    sum += B[i * N1D] * col[i * stride];
                  if (c < DIM - 1)
                    out[slot] = sum;
                  else
                    acc[k] += sum;
                }
            }
          if (c < DIM - 1)
            __syncthreads();
        }
    }
  if (on)
    {
#pragma unroll
      for (int k = 0; k < C::NCH; ++k)
        if (i0 + k * W < C::n)
          {
            double *dst = coarse + (int64_t)A.coarse_off[P] + i0 + k * W;
            *dst = ADD ? *dst + acc[k] : acc[k];
          }
    }
}

// r <- b - r (r holds A x): the second half of pdh_residual_device
__global__ void __launch_bounds__(256) k_residual_sub(int64_t N, const double *__restrict__ b, double *__restrict__ r)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    r[i] = b[i] - r[i];
}

template <int DIM, int N1D>
hipError_t launch_pair(bool restrict_, bool add, const PdhTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  using C = Cut<DIM, N1D>;
  const int64_t count = restrict_ ? A.n_coarse : A.n_fine;
  const dim3 grid((unsigned)((count + C::G - 1) / C::G)), block(W);
  if (restrict_)
    {
      if (add)
        hipLaunchKernelGGL((k_restrict<DIM, N1D, true>), grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL((k_restrict<DIM, N1D, false>), grid, block, 0, stream, A, src, dst);
    }
  else
    {
      if (add)
        hipLaunchKernelGGL((k_prolongate<DIM, N1D, true>), grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL((k_prolongate<DIM, N1D, false>), grid, block, 0, stream, A, src, dst);
    }
  return hipGetLastError();
}

template <int DIM>
hipError_t launch_dim(int n1d, bool restrict_, bool add, const PdhTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  switch (n1d)
    {
    case 2: return launch_pair<DIM, 2>(restrict_, add, A, src, dst, stream);
    case 3: return launch_pair<DIM, 3>(restrict_, add, A, src, dst, stream);
    case 4: return launch_pair<DIM, 4>(restrict_, add, A, src, dst, stream);
    case 5: return launch_pair<DIM, 5>(restrict_, add, A, src, dst, stream);
    case 6: return launch_pair<DIM, 6>(restrict_, add, A, src, dst, stream);
    case 7: return launch_pair<DIM, 7>(restrict_, add, A, src, dst, stream);
    case 8: return launch_pair<DIM, 8>(restrict_, add, A, src, dst, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_transfer(int dim, int n1d, bool restrict_, bool add, const PdhTransferArgs *A, const double *src, double *dst,
                           hipStream_t stream)
{
  if (A->n_fine <= 0 || A->n_coarse <= 0)
    return hipSuccess;
  if (dim == 2)
    return launch_dim<2>(n1d, restrict_, add, *A, src, dst, stream);
  if (dim == 3)
    return launch_dim<3>(n1d, restrict_, add, *A, src, dst, stream);
  return hipErrorInvalidValue;
}
} // namespace

extern "C" hipError_t pdh_launch_prolongate(int dim, int n1d, int add, const PdhTransferArgs *A, const double *coarse, double *fine,
                                            hipStream_t stream)
{
  return launch_transfer(dim, n1d, false, add != 0, A, coarse, fine, stream);
}

extern "C" hipError_t pdh_launch_restrict(int dim, int n1d, int add, const PdhTransferArgs *A, const double *fine, double *coarse,
                                          hipStream_t stream)
{
  return launch_transfer(dim, n1d, true, add != 0, A, fine, coarse, stream);
}

extern "C" hipError_t pdh_launch_residual_sub(int64_t n_rows, const double *b, double *r, hipStream_t stream)
{
  if (n_rows <= 0)
    return hipSuccess;
  const int64_t blocks = (n_rows + 255) / 256;
  hipLaunchKernelGGL(k_residual_sub, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, n_rows, b, r);
  return hipGetLastError();
}
