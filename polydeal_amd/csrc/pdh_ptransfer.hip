// pdh_ptransfer.hip — transfers between two polynomial degrees q < p on the same polytopes (C ABI: pdh_ptransfer_create, served by
// pdh_prolongate*, pdh_restrict*; layout: pdh_ptransfer.h).
//
// FE_DGQ: the injection block of every polytope is the Kronecker power of ONE NF x NC matrix B (NF = p + 1, NC = q + 1).  Both kernels
// apply it axis by axis through LDS (rectangular sum factorisation): the extents go NC^3 -> NF NC^2 -> NF^2 NC -> NF^3 in the
// prolongation and back in the restriction, every pass loops over ITS output count.  B is wave-uniform: it arrives in the kernel
// arguments and is staged once in LDS - no table is read from memory.  A transfer is one pass over the two vectors.
// FE_AggloDGP: an index map, one copy per dof, no LDS.
//
// Every sum has a fixed order (a lane adds its NC or NF terms in index order) and there are no atomics: the same call on the same data
// gives the same bits.  Rows of the level vectors outside every polytope are not touched.
#include "pdh_ptransfer.h"
#include "pdh_launch.h"

#include <hip/hip_runtime.h>

namespace
{
constexpr int W = 64;
constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

// How a wave is cut (as pdh_transfer.hip): G polytopes of up to 64 FINE dofs share it, larger ones take it in chunks of 64 lanes.  Both
// LDS buffers give every polytope n_f doubles: no intermediate is larger (NC < NF).
template <int DIM, int NF, int NC>
struct PCut
{
  static_assert(NC < NF, "coarse degree below the fine one");
  static constexpr int n_f = ipow(NF, DIM);
  static constexpr int n_c = ipow(NC, DIM);
  static constexpr int G = n_f >= W ? 1 : W / n_f;
};

// the polytopes of the wave (-1: none) and B into LDS
template <int NF, int NC, int G>
__device__ __forceinline__ void stage(const PdhPTransferArgs &A, int32_t *pol, double *tb, int lane)
{
  if (lane < G)
    {
      const int64_t P = (int64_t)blockIdx.x * G + lane;
      pol[lane] = P < A.n_polytopes ? (int32_t)P : -1;
    }
  for (int e = lane; e < NF * NC; e += W)
    tb[e] = A.B[e];
}

// One pass of the prolongation over axis AX, whose extent goes from NC to NF: out[lo, i, hi] = sum_j B[i][j] in[lo, j, hi], lo over the
// axes already at NF, hi over those still at NC.  The last pass writes fine[off + i] (ADD: adds to it).
template <int DIM, int NF, int NC, bool ADD, int AX>
__device__ __forceinline__ void prolongate_pass(const PdhPTransferArgs &A, const double *tb, const int32_t *pol, const double *in, double *out,
                                                double *__restrict__ fine, int lane)
{
  using C = PCut<DIM, NF, NC>;
  constexpr int sl = ipow(NF, AX);                             // stride of the axis, on both sides
  constexpr int cnt = ipow(NF, AX + 1) * ipow(NC, DIM - 1 - AX); // outputs of this pass per polytope
#pragma unroll
  for (int s = lane; s < C::G * cnt; s += W)
    {
      const int g = s / cnt, o = s - g * cnt;
      const int lo = o % sl, i = (o / sl) % NF, hi = o / (sl * NF);
      const double *B = tb + i * NC;
      const double *col = in + g * C::n_f + lo + hi * (sl * NC);
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < NC; ++j)
        sum += B[j] * col[j * sl];
      if constexpr (AX < DIM - 1)
        out[g * C::n_f + o] = sum;
      else
        {
          const int P = pol[g];
          if (P >= 0)
            {
              double *dst = fine + (int64_t)A.fine_off[P] + o;
              *dst = ADD ? *dst + sum : sum;
            }
        }
    }
}

// One wave per G polytopes; the coarse coefficients go to LDS, then one pass per axis.
template <int DIM, int NF, int NC, bool ADD>
__global__ void __launch_bounds__(W) k_p_prolongate(const PdhPTransferArgs A, const double *__restrict__ coarse, double *__restrict__ fine)
{
  using C = PCut<DIM, NF, NC>;
  __shared__ double u[2][C::G * C::n_f];
  __shared__ double tb[NF * NC];
  __shared__ int32_t pol[C::G];
  const int lane = threadIdx.x;
  stage<NF, NC, C::G>(A, pol, tb, lane);
  __syncthreads();
#pragma unroll
  for (int s = lane; s < C::G * C::n_c; s += W)
    {
      const int g = s / C::n_c, j = s - g * C::n_c, P = pol[g];
      u[0][g * C::n_f + j] = P >= 0 ? coarse[(int64_t)A.coarse_off[P] + j] : 0.0;
    }
  __syncthreads();
  prolongate_pass<DIM, NF, NC, ADD, 0>(A, tb, pol, u[0], u[1], fine, lane);
  __syncthreads();
  if constexpr (DIM == 2)
    prolongate_pass<DIM, NF, NC, ADD, 1>(A, tb, pol, u[1], u[0], fine, lane);
  else
    {
      prolongate_pass<DIM, NF, NC, ADD, 1>(A, tb, pol, u[1], u[0], fine, lane);
      __syncthreads();
      prolongate_pass<DIM, NF, NC, ADD, 2>(A, tb, pol, u[0], u[1], fine, lane);
    }
}

// One pass of the restriction over axis AX, whose extent goes from NF to NC with the transposed matrix:
// out[lo, j, hi] = sum_i B[i][j] in[lo, i, hi], lo over the axes already at NC, hi over those still at NF.  The last pass writes
// coarse[off + j] (ADD: adds to it).
template <int DIM, int NF, int NC, bool ADD, int AX>
__device__ __forceinline__ void restrict_pass(const PdhPTransferArgs &A, const double *tb, const int32_t *pol, const double *in, double *out,
                                              double *__restrict__ coarse, int lane)
{
  using C = PCut<DIM, NF, NC>;
  constexpr int sl = ipow(NC, AX);                             // stride of the axis, on both sides
  constexpr int cnt = ipow(NC, AX + 1) * ipow(NF, DIM - 1 - AX); // outputs of this pass per polytope
#pragma unroll
  for (int s = lane; s < C::G * cnt; s += W)
    {
      const int g = s / cnt, o = s - g * cnt;
      const int lo = o % sl, j = (o / sl) % NC, hi = o / (sl * NC);
      const double *B = tb + j;
      const double *col = in + g * C::n_f + lo + hi * (sl * NF);
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < NF; ++i)
        sum += B[i * NC] * col[i * sl];
      if constexpr (AX < DIM - 1)
        out[g * C::n_f + o] = sum;
      else
        {
          const int P = pol[g];
          if (P >= 0)
            {
              double *dst = coarse + (int64_t)A.coarse_off[P] + o;
              *dst = ADD ? *dst + sum : sum;
            }
        }
    }
}

// One wave per G polytopes; the fine values go to LDS, then one pass per axis.
template <int DIM, int NF, int NC, bool ADD>
__global__ void __launch_bounds__(W) k_p_restrict(const PdhPTransferArgs A, const double *__restrict__ fine, double *__restrict__ coarse)
{
  using C = PCut<DIM, NF, NC>;
  __shared__ double u[2][C::G * C::n_f];
  __shared__ double tb[NF * NC];
  __shared__ int32_t pol[C::G];
  const int lane = threadIdx.x;
  stage<NF, NC, C::G>(A, pol, tb, lane);
  __syncthreads();
#pragma unroll
  for (int s = lane; s < C::G * C::n_f; s += W)
    {
      const int g = s / C::n_f, i = s - g * C::n_f, P = pol[g];
      u[0][s] = P >= 0 ? fine[(int64_t)A.fine_off[P] + i] : 0.0;
    }
  __syncthreads();
  restrict_pass<DIM, NF, NC, ADD, 0>(A, tb, pol, u[0], u[1], coarse, lane);
  __syncthreads();
  if constexpr (DIM == 2)
    restrict_pass<DIM, NF, NC, ADD, 1>(A, tb, pol, u[1], u[0], coarse, lane);
  else
    {
      restrict_pass<DIM, NF, NC, ADD, 1>(A, tb, pol, u[1], u[0], coarse, lane);
      __syncthreads();
      restrict_pass<DIM, NF, NC, ADD, 2>(A, tb, pol, u[0], u[1], coarse, lane);
    }
}

// FE_AggloDGP, one thread per fine dof: the coarse value with the same multi-index, or 0 (ADD: the dofs outside the image stay)
template <bool ADD>
__global__ void __launch_bounds__(256) k_p_map_prolongate(const PdhPTransferArgs A, const double *__restrict__ coarse, double *__restrict__ fine)
{
  const int64_t total = (int64_t)A.n_polytopes * A.n_f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256)
    {
      const int P = (int)(t / A.n_f), i = (int)(t - (int64_t)P * A.n_f);
      const int j = A.inv[i];
      double *dst = fine + (int64_t)A.fine_off[P] + i;
      if (j >= 0)
        {
          const double v = coarse[(int64_t)A.coarse_off[P] + j];
          *dst = ADD ? *dst + v : v;
        }
      else if (!ADD)
        *dst = 0.0;
    }
}

// FE_AggloDGP, one thread per coarse dof: the fine value with the same multi-index
template <bool ADD>
__global__ void __launch_bounds__(256) k_p_map_restrict(const PdhPTransferArgs A, const double *__restrict__ fine, double *__restrict__ coarse)
{
  const int64_t total = (int64_t)A.n_polytopes * A.n_c;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256)
    {
      const int P = (int)(t / A.n_c), j = (int)(t - (int64_t)P * A.n_c);
      const double v = fine[(int64_t)A.fine_off[P] + A.map[j]];
      double *dst = coarse + (int64_t)A.coarse_off[P] + j;
      *dst = ADD ? *dst + v : v;
    }
}

template <int DIM, int NF, int NC>
hipError_t launch_pair(bool restrict_, bool add, const PdhPTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  using C = PCut<DIM, NF, NC>;
  const dim3 grid((unsigned)(((int64_t)A.n_polytopes + C::G - 1) / C::G)), block(W);
  if (restrict_)
    {
      if (add)
        hipLaunchKernelGGL((k_p_restrict<DIM, NF, NC, true>), grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL((k_p_restrict<DIM, NF, NC, false>), grid, block, 0, stream, A, src, dst);
    }
  else
    {
      if (add)
        hipLaunchKernelGGL((k_p_prolongate<DIM, NF, NC, true>), grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL((k_p_prolongate<DIM, NF, NC, false>), grid, block, 0, stream, A, src, dst);
    }
  return hipGetLastError();
}

// the coarse extent NC = 2 .. NF - 1 of a fine extent NF
template <int DIM, int NF, int NC = 2>
hipError_t launch_nc(int nc, bool restrict_, bool add, const PdhPTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  if constexpr (NC >= NF)
    return hipErrorInvalidValue;
  else
    return nc == NC ? launch_pair<DIM, NF, NC>(restrict_, add, A, src, dst, stream) : launch_nc<DIM, NF, NC + 1>(nc, restrict_, add, A, src, dst, stream);
}

template <int DIM>
hipError_t launch_dim(bool restrict_, bool add, const PdhPTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  switch (A.nf1d)
    {
    case 3: return launch_nc<DIM, 3>(A.nc1d, restrict_, add, A, src, dst, stream);
    case 4: return launch_nc<DIM, 4>(A.nc1d, restrict_, add, A, src, dst, stream);
    case 5: return launch_nc<DIM, 5>(A.nc1d, restrict_, add, A, src, dst, stream);
    case 6: return launch_nc<DIM, 6>(A.nc1d, restrict_, add, A, src, dst, stream);
    case 7: return launch_nc<DIM, 7>(A.nc1d, restrict_, add, A, src, dst, stream);
    case 8: return launch_nc<DIM, 8>(A.nc1d, restrict_, add, A, src, dst, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_map(bool restrict_, bool add, const PdhPTransferArgs &A, const double *src, double *dst, hipStream_t stream)
{
  if (A.n_f <= 0 || A.n_c <= 0 || A.n_c >= A.n_f || !A.map || !A.inv)
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)A.n_polytopes * (restrict_ ? A.n_c : A.n_f), blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(256);
  if (restrict_)
    {
      if (add)
        hipLaunchKernelGGL(k_p_map_restrict<true>, grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL(k_p_map_restrict<false>, grid, block, 0, stream, A, src, dst);
    }
  else
    {
      if (add)
        hipLaunchKernelGGL(k_p_map_prolongate<true>, grid, block, 0, stream, A, src, dst);
      else
        hipLaunchKernelGGL(k_p_map_prolongate<false>, grid, block, 0, stream, A, src, dst);
    }
  return hipGetLastError();
}
} // namespace

extern "C" hipError_t pdh_launch_ptransfer(int dim, int dgq, int restriction, int add, const PdhPTransferArgs *A, const double *src, double *dst,
                                           hipStream_t stream)
{
  if (A->n_polytopes <= 0)
    return hipSuccess;
  if (!dgq)
    return launch_map(restriction != 0, add != 0, *A, src, dst, stream);
  if (dim == 2)
    return launch_dim<2>(restriction != 0, add != 0, *A, src, dst, stream);
  if (dim == 3)
    return launch_dim<3>(restriction != 0, add != 0, *A, src, dst, stream);
  return hipErrorInvalidValue;
}
