// pdh_shadow.hip — the float32 shadow of a level's matrix and block inverses, the product with it and the Chebyshev update that reads
// the float inverses (layout and launchers: pdh_shadow.h; C ABI: pdh_set_smoother_precision, pdh_smoother_vmult_device).
//
// Only the matrix entries are single precision: x is gathered as doubles, every product is (double)a * x and every sum is a double sum
// in the fixed orders of pdh_solve.hip (a lane adds its terms in index order, a wave adds its 64 lanes by a butterfly).  No atomics:
// the same call on the same data gives the same bits.
#include "pdh_shadow.h"

namespace
{
constexpr int W = 64;
constexpr int PW = 2 * W; // entries of one wave-wide piece: 8 bytes per lane, 512 bytes like a piece of k_vmult
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// sum over the 64 lanes; every lane gets the same bits (pdh_solve.hip)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int m = W / 2; m > 0; m >>= 1)
    v += __shfl_xor(v, m, W);
  return v;
}

// One wave per owned polytope: its n shadow rows are contiguous (stride rs), so the wave writes them as ONE run of float2 in address
// order.  Output position a of row i takes value position k(a): a itself, or in the deal.II layout k = 0 for the diagonal
// (a = diag_L + i), a + 1 below it and a above (the inverse of row_part's a(k) in pdh_solve.hip); the pad entry of an odd row is zero.
template <bool DF>
__global__ void __launch_bounds__(W) k_shadow_rows(const PdhSolveArgs A, const int64_t *__restrict__ base, float *__restrict__ out)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = A.n, rl = A.row_len[s], dL = A.diag_L[s];
  const int half = pdh_shadow_stride(rl) >> 1;
  const double *__restrict__ v = A.values + A.row_base[s];
  f32x2 *__restrict__ o = reinterpret_cast<f32x2 *>(out + base[s]);
  const int total = n * half;
#pragma unroll 4
  for (int t = lane; t < total; t += W)
    {
      const int i = t / half, a = 2 * (t - i * half), di = dL + i;
      const double *__restrict__ vr = v + (int64_t)i * rl;
      const int k0 = DF ? (a == di ? 0 : (a < di ? a + 1 : a)) : a;
      const int k1 = DF ? (a + 1 == di ? 0 : (a + 1 < di ? a + 2 : a + 1)) : a + 1;
      f32x2 w;
      w.x = (float)__builtin_nontemporal_load(vr + k0); // (a <= stride - 2 < rl)
      w.y = a + 1 < rl ? (float)__builtin_nontemporal_load(vr + k1) : 0.0f;
      o[t] = w;
    }
}

// out[k] = (float)in[k]: two entries per thread, the last thread of an odd count one
__global__ void __launch_bounds__(256) k_shadow_round(const double *__restrict__ in, float *__restrict__ out, int64_t count)
{
  const int64_t pairs = count >> 1;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < pairs; t += (int64_t)gridDim.x * 256)
    {
      const f64x2 v = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(in) + t);
      f32x2 w;
      w.x = (float)v.x;
      w.y = (float)v.y;
      reinterpret_cast<f32x2 *>(out)[t] = w;
    }
  if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    out[count - 1] = (float)in[count - 1];
}

// Lane's share of one shadow row: the entries k, k + 1 with k = k0 + 128 u + 2 lane, u < NP.  The NP loads are issued before any of them
// is used; a piece that reaches past the row (stride rs, rl entries and a zero pad) is clamped to the row's last pair and its surplus
// lanes discarded.
template <int NP>
__device__ __forceinline__ double row_part(const float *__restrict__ vr, const double *xs, int k0, int rl, int rs, int lane)
{
  f32x2 val[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u)
    {
      const int k = k0 + u * PW + 2 * lane;
      val[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x2 *>(vr + (k < rs ? k : rs - 2)));
    }
  double sum = 0.0;
#pragma unroll
  for (int u = 0; u < NP; ++u)
    {
      const int k = k0 + u * PW + 2 * lane;
      sum += k < rl ? (double)val[u].x * xs[k] : 0.0;
      sum += k + 1 < rl ? (double)val[u].y * xs[k + 1] : 0.0;
    }
  return sum;
}

__device__ __forceinline__ double row_dot(const float *__restrict__ vr, const double *xs, int rl, int rs, int lane)
{
  switch ((rl + PW - 1) / PW)
    {
    case 1: return row_part<1>(vr, xs, 0, rl, rs, lane);
    case 2: return row_part<2>(vr, xs, 0, rl, rs, lane);
    case 3: return row_part<3>(vr, xs, 0, rl, rs, lane);
    case 4: return row_part<4>(vr, xs, 0, rl, rs, lane);
    case 5: return row_part<5>(vr, xs, 0, rl, rs, lane);
    case 6: return row_part<6>(vr, xs, 0, rl, rs, lane);
    case 7: return row_part<7>(vr, xs, 0, rl, rs, lane);
    case 8: return row_part<8>(vr, xs, 0, rl, rs, lane);
    default:
      {
        double sum = 0.0;
        for (int k0 = 0; k0 < rl; k0 += 8 * PW)
          sum += row_part<8>(vr, xs, k0, rl, rs, lane);
        return sum;
      }
    }
}

// k_vmult of pdh_solve.hip over the shadow rows: one wave per owned polytope, the x of its column set gathered into LDS as doubles
// once, rows two at a time, the sum of row i in lane i % 64, 64 rows stored together.  One instantiation: the shadow is ascending.
__global__ void __launch_bounds__(W) k_vmult_f32(const PdhSolveArgs A, const PdhShadowArgs S, const double *__restrict__ x,
                                                 double *__restrict__ y)
{
  extern __shared__ double xs[];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int n = A.n, rl = A.row_len[s], rs = pdh_shadow_stride(rl);
  const int64_t b0 = A.blk_ptr[s];
  for (int a = lane; a < rl; a += W)
    {
      const int t = a / n;
      xs[a] = x[(int64_t)A.blk_dof[b0 + t] + (a - t * n)];
    }
  __syncthreads();
  const float *__restrict__ v = S.values + S.base[s];
  double *__restrict__ ys = y + A.own_row[s];
  double yv = 0.0;
  for (int i = 0; i < n; i += 2)
    {
      const int i1 = i + 1 < n ? i + 1 : i; // (odd n: the last row twice, the copy is dropped)
      double s0 = row_dot(v + (int64_t)i * rs, xs, rl, rs, lane);
      double s1 = row_dot(v + (int64_t)i1 * rs, xs, rl, rs, lane);
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
            ys[r0 + lane] = yv;
        }
    }
}

// k_cheb_update<FIRST, PDH_PREC_BLOCK_JACOBI> of pdh_solve.hip with the inverse read as floats (n <= 64: one pass per slot),
//   r <- FIRST ? b (- q if the start is not zero) : r - q;   z = P~^-1 r;   d <- FIRST ? c2 z : c1 d + c2 z;   x <- x + d
// rcg (may be NULL): the slot's partial of rcg^T x goes to part[PDH_PART_RZ], k_cg_finalise stays the one place where partials are added.
template <bool FIRST>
__global__ void __launch_bounds__(W) k_cheb_update_f32(const PdhSolveArgs A, const float *__restrict__ dinv, const double *b,
                                                       const double *__restrict__ q, double *__restrict__ d, double *__restrict__ r, double *x,
                                                       double c1, double c2, int zero_start, const double *rcg, double *__restrict__ part)
{
  __shared__ double rs[W];
  const int s = blockIdx.x, lane = threadIdx.x, n = A.n;
  const int64_t o = A.own_row[s];
  const int i = lane;
  const bool on = i < n;
  double ri = 0.0;
  if (on)
    {
      if (FIRST)
        ri = q ? b[o + i] - q[o + i] : b[o + i];
      else
        ri = r[o + i] - q[o + i];
    }
  rs[lane] = ri;
  __syncthreads();
  double zi = 0.0, rz = 0.0;
  if (on)
    { // z_i = sum_j Dinv[j][i] r_j (= Dinv[i][j]: stored symmetric), row j read whole by the wave
      const float *__restrict__ D = dinv + (int64_t)s * n * n + i;
#pragma unroll 8
      for (int j = 0; j < n; ++j)
        zi += (double)__builtin_nontemporal_load(D + (int64_t)j * n) * rs[j];
      const double di = FIRST ? c2 * zi : c1 * d[o + i] + c2 * zi;
      const double xi = (FIRST && zero_start) ? di : x[o + i] + di;
      r[o + i] = ri;
      d[o + i] = di;
      x[o + i] = xi;
      if (rcg)
        rz = rcg[o + i] * xi;
    }
  if (rcg)
    {
      rz = wave_sum(rz);
      if (lane == 0)
        part[PDH_PART_RZ * (int64_t)A.n_owned + s] = rz;
    }
}
} // namespace

extern "C" hipError_t pdh_launch_shadow_rows(const PdhSolveArgs *A, const int64_t *base, float *out, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if (A->diag_first)
    hipLaunchKernelGGL(k_shadow_rows<true>, dim3(A->n_owned), dim3(W), 0, stream, *A, base, out);
  else
    hipLaunchKernelGGL(k_shadow_rows<false>, dim3(A->n_owned), dim3(W), 0, stream, *A, base, out);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_shadow_round(const double *in, float *out, int64_t count, hipStream_t stream)
{
  if (count <= 0)
    return hipSuccess;
  const int64_t blocks = (count / 2 + 255) / 256;
  hipLaunchKernelGGL(k_shadow_round, dim3((unsigned)(blocks < 1 ? 1 : (blocks < 8192 ? blocks : 8192))), dim3(256), 0, stream, in, out, count);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_vmult_f32(const PdhSolveArgs *A, const PdhShadowArgs *S, const double *x, double *y, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  const size_t lds = (size_t)A->max_row_len * sizeof(double);
  hipLaunchKernelGGL(k_vmult_f32, dim3(A->n_owned), dim3(W), lds, stream, *A, *S, x, y);
  return hipGetLastError();
}

extern "C" hipError_t pdh_launch_cheb_update_f32(const PdhSolveArgs *A, int first, const float *dinv, const double *b, const double *q,
                                                 double *d, double *r, double *x, double c1, double c2, int zero_start, const double *rcg,
                                                 double *part, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  if (A->n > W || (!first && !q) || (rcg && !part))
    return hipErrorInvalidValue;
  const dim3 g(A->n_owned), blk(W);
  if (first)
    hipLaunchKernelGGL(k_cheb_update_f32<true>, g, blk, 0, stream, *A, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part);
  else
    hipLaunchKernelGGL(k_cheb_update_f32<false>, g, blk, 0, stream, *A, dinv, b, q, d, r, x, c1, c2, zero_start, rcg, part);
  return hipGetLastError();
}
