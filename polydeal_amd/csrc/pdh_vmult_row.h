// pdh_vmult_row.h — the arithmetic of one row of y = A x, shared by the kernels that form it (pdh_solve.hip: k_vmult over the global
// numbering; pdh_dist.hip: k_vmult_local over a rank's local vector).  Both sum the same terms in the same order, so they agree to
// the bit.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace pdh_row
{
constexpr int W = 64;

// sum over the 64 lanes; every lane gets the same bits (a + b = b + a at every butterfly stage)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int m = W / 2; m > 0; m >>= 1)
    v += __shfl_xor(v, m, W);
  return v;
}

// Lane's share of one row: the terms k = k0 + 64 u + lane, u < NP.  The NP loads are issued before any of them is used (the last
// piece of a row is clamped to its last entry and its surplus lanes discarded), so a wave has NP 512-byte pieces in flight.
// Value position k holds ascending position a(k): k itself, or in the deal.II layout the diagonal first (k = 0 -> di = diag_L + i)
// and the entries before it shifted by one (1 <= k <= di -> k - 1).
template <int NP, bool DF>
__device__ __forceinline__ double row_part(const double *__restrict__ vr, const double *xs, int k0, int rl, int di, int lane)
{
  double val[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u)
    {
      const int k = k0 + u * W + lane;
      val[u] = __builtin_nontemporal_load(vr + (k < rl ? k : rl - 1));
    }
  double sum = 0.0;
#pragma unroll
  for (int u = 0; u < NP; ++u)
    {
      const int k = k0 + u * W + lane;
      const int a = DF ? (k == 0 ? di : (k <= di ? k - 1 : k)) : k;
      sum += k < rl ? val[u] * xs[a < rl ? a : 0] : 0.0;
    }
  return sum;
}

template <bool DF>
__device__ __forceinline__ double row_dot(const double *__restrict__ vr, const double *xs, int rl, int di, int lane)
{
  switch ((rl + W - 1) / W)
    {
    case 1: return row_part<1, DF>(vr, xs, 0, rl, di, lane);
    case 2: return row_part<2, DF>(vr, xs, 0, rl, di, lane);
    case 3: return row_part<3, DF>(vr, xs, 0, rl, di, lane);
    case 4: return row_part<4, DF>(vr, xs, 0, rl, di, lane);
    case 5: return row_part<5, DF>(vr, xs, 0, rl, di, lane);
    case 6: return row_part<6, DF>(vr, xs, 0, rl, di, lane);
    case 7: return row_part<7, DF>(vr, xs, 0, rl, di, lane);
    case 8: return row_part<8, DF>(vr, xs, 0, rl, di, lane);
    default:
      {
        double sum = 0.0;
        for (int k0 = 0; k0 < rl; k0 += 8 * W)
          sum += row_part<8, DF>(vr, xs, k0, rl, di, lane);
        return sum;
      }
    }
}
} // namespace pdh_row
