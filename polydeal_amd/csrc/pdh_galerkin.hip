// pdh_galerkin.hip — the coarse level matrix as the Galerkin product P^T A_f P of the resident fine matrix (C ABI: pdh_galerkin_device;
// layout and plan: pdh_galerkin.h).  One wave owns one coarse block from the first read to the last store: it walks the fine blocks the
// plan gives it, applies the 1-D matrices of the transfer to both sides of each (sum factorisation, pdh_transfer.h) and adds the result
// to an accumulator in registers.  The fine matrix is read once, no n x n injection block is formed.
//
// Every sum has a fixed order: a lane adds the N1D terms of a 1-D contraction in index order, the wave adds the fine blocks in plan order
// (ascending fine slot, then block position).  No atomics: the same call on the same data gives the same bits.
//
// Lanes.  A fine block goes through LDS twice: lane i contracts the COLUMN index of row i with the matrices of the column polytope F',
// then lane j contracts the ROW index of column j with those of the row polytope F - n lanes work, each on n values in registers with
// compile-time indices.  Blocks of n < 64 dofs leave 64 - n lanes idle in these two phases (their loads and stores still use 64 / n rows
// per step).  Packing several coarse blocks into one wave, as k_prolongate packs polytopes, would put blocks with different numbers of
// contributions (1 .. 4^dim on block agglomerates) into one loop; the small elements are the small matrices, so the lanes stay idle.
#include "pdh_galerkin.h"
#include "pdh_launch.h"

#include <hip/hip_runtime.h>

namespace
{
constexpr int W = 64;
constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }

template <int DIM, int N1D>
struct Cut
{
  static constexpr int n = ipow(N1D, DIM);
  static constexpr int LD = n | 1;                  // LDS row stride (doubles): odd, rows and columns are both read without bank conflicts
  static constexpr int G = W / n;                   // rows of a block one load / store step of the wave covers
  static constexpr int NL = (n + G - 1) / G;        // such steps per block
  static constexpr int TAB = DIM * N1D * N1D;       // the 1-D matrices of one fine polytope
};

// value position of ascending position a in a row whose diagonal entry is at ascending position di (pdh_solve.h)
__device__ __forceinline__ int value_pos(bool diag_first, int a, int di) { return diag_first ? (a == di ? 0 : (a < di ? a + 1 : a)) : a; }

// r <- (B_(DIM-1) (x) .. (x) B_0)^T r, axis by axis: out[.., j_c, ..] = sum_i B_c[i][j_c] in[.., i, ..] (the sums of k_restrict).  B is
// the same for the whole wave.
template <int DIM, int N1D>
__device__ __forceinline__ void contract(double (&r)[ipow(N1D, DIM)], const double *__restrict__ B)
{
  constexpr int n = Cut<DIM, N1D>::n;
#pragma unroll
  for (int c = 0; c < DIM; ++c)
    {
      const int stride = ipow(N1D, c);
      double Bc[N1D * N1D];
#pragma unroll
      for (int e = 0; e < N1D * N1D; ++e)
        Bc[e] = B[c * N1D * N1D + e];
#pragma unroll
      for (int q = 0; q < n; ++q)
        if ((q / stride) % N1D == 0)
          {
            double in[N1D];
#pragma unroll
            for (int i = 0; i < N1D; ++i)
              in[i] = r[q + i * stride];
#pragma unroll
            for (int j = 0; j < N1D; ++j)
              {
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < N1D; ++i)
                  sum += Bc[i * N1D + j] * in[i];
                r[q + j * stride] = sum;
              }
          }
    }
}

// One wave per coarse block b.  The next fine block is on its way from memory (registers pf) while the current one is contracted.
template <int DIM, int N1D>
__global__ void __launch_bounds__(W) k_galerkin(const PdhGalerkinArgs A)
{
  using C = Cut<DIM, N1D>;
  constexpr int n = C::n;
  __shared__ double S[n * C::LD];
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  const int li = lane / n, lj = lane - li * n; // the lane's row within a load / store step, and its column
  const bool mover = lane < C::G * n;
  const bool worker = lane < n;
  const int64_t e0 = A.plan_ptr[b], e1 = A.plan_ptr[b + 1];
  const bool f_df = A.f_diag_first != 0, c_df = A.c_diag_first != 0;

  double acc[n], pf[C::NL];
#pragma unroll
  for (int i = 0; i < n; ++i)
    acc[i] = 0.0;
#pragma unroll
  for (int u = 0; u < C::NL; ++u)
    pf[u] = 0.0;

  // block t of fine slot F as whole rows' pieces: row i at row_base[F] + i * row_len[F], every byte of it read once
  auto fetch = [&](int64_t e) {
    const int F = A.plan_slot[e], t = A.plan_pos[e];
    const int rl = A.f_row_len[F], dL = A.f_diag_L[F];
    const double *__restrict__ v = A.fine_values + A.f_row_base[F];
#pragma unroll
    for (int u = 0; u < C::NL; ++u)
      {
        const int i = u * C::G + li;
        if (mover && i < n)
          pf[u] = __builtin_nontemporal_load(v + (int64_t)i * rl + value_pos(f_df, t * n + lj, dL + i));
      }
  };

  fetch(e0);
  for (int64_t e = e0; e < e1; ++e)
    {
#pragma unroll
      for (int u = 0; u < C::NL; ++u)
        {
          const int i = u * C::G + li;
          if (mover && i < n)
            S[i * C::LD + lj] = pf[u];
        }
      const int F = __builtin_amdgcn_readfirstlane(A.plan_slot[e]), F2 = __builtin_amdgcn_readfirstlane(A.plan_col[e]);
      __syncthreads();
      if (e + 1 < e1)
        fetch(e + 1);
      if (worker)
        { // columns: row `lane` times the injection block of F'
          double r[n];
#pragma unroll
          for (int j = 0; j < n; ++j)
            r[j] = S[lane * C::LD + j];
          contract<DIM, N1D>(r, A.tab + (int64_t)F2 * C::TAB);
#pragma unroll
          for (int j = 0; j < n; ++j)
            S[lane * C::LD + j] = r[j];
        }
      __syncthreads();
      if (worker)
        { // rows: the transposed injection block of F times column `lane`
          double r[n];
#pragma unroll
          for (int i = 0; i < n; ++i)
            r[i] = S[i * C::LD + lane];
          contract<DIM, N1D>(r, A.tab + (int64_t)F * C::TAB);
#pragma unroll
          for (int i = 0; i < n; ++i)
            acc[i] += r[i];
        }
      __syncthreads();
    }

  // lane j holds column j of the block: through LDS into rows, each row one run of n doubles at the block's place in the coarse layout
  if (worker)
    {
#pragma unroll
      for (int i = 0; i < n; ++i)
        S[i * C::LD + lane] = acc[i];
    }
  __syncthreads();
  const int Cs = A.blk_slot[b], tc = A.blk_pos[b];
  const int rl = A.c_row_len[Cs], dL = A.c_diag_L[Cs];
  double *__restrict__ v = A.coarse_values + A.c_row_base[Cs];
#pragma unroll
  for (int u = 0; u < C::NL; ++u)
    {
      const int i = u * C::G + li;
      if (mover && i < n)
        v[(int64_t)i * rl + value_pos(c_df, tc * n + lj, dL + i)] = S[i * C::LD + lj];
    }
}

template <int DIM, int N1D>
hipError_t launch(const PdhGalerkinArgs &A, hipStream_t stream)
{
  hipLaunchKernelGGL((k_galerkin<DIM, N1D>), dim3((unsigned)A.n_blocks), dim3(W), 0, stream, A);
  return hipGetLastError();
}
} // namespace

extern "C" hipError_t pdh_launch_galerkin(int dim, int n1d, const PdhGalerkinArgs *A, hipStream_t stream)
{
  if (A->n_blocks <= 0)
    return hipSuccess;
  if (dim == 2)
    switch (n1d)
      {
      case 2: return launch<2, 2>(*A, stream);
      case 3: return launch<2, 3>(*A, stream);
      case 4: return launch<2, 4>(*A, stream);
      case 5: return launch<2, 5>(*A, stream);
      case 6: return launch<2, 6>(*A, stream);
      case 7: return launch<2, 7>(*A, stream);
      case 8: return launch<2, 8>(*A, stream);
      default: return hipErrorInvalidValue;
      }
  if (dim == 3)
    switch (n1d)
      {
      case 2: return launch<3, 2>(*A, stream);
      case 3: return launch<3, 3>(*A, stream);
      case 4: return launch<3, 4>(*A, stream);
      default: return hipErrorInvalidValue;
      }
  return hipErrorInvalidValue;
}
