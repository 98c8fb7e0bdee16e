// pdh_terms_tables.h — the PdhTerms struct and the layout arithmetic shared by the term kernels (pdh_terms.h, pdh_terms_wg.h: device)
// and the host (pdh_plan.cpp builds the tables, pdh_capi.cpp uploads them).  Compiles with and without HIP.
#pragma once
#include <stdint.h>
#include <type_traits>

#include "pdh_dev.h"
#define TERMS_MI 4 // most intervals of a composite 1-D rule (8 points of 2-point rules)
struct PdhTerms
{
  // per owned polytope one record of TERMS_HDR + maxruns * TERMS_ENT doubles (pdh_terms.h):
  //   header: [0] runs | cells << 16 | boundary sub-faces << 32 (integers), [1..3] lower corner of the box, [4..6] 1 / side,
  //           [7] first value of the polytope's rows, [8] row length, [9] ascending position L of the own block,
  //           [10] first volume point, [11] sub-faces (integer)
  //   run t (a polytopal face = all sub-faces shared with one neighbour; the boundary run first, then ascending block rank):
  //           [0] first sub-face of the run in the polytope's list | sub-faces << 32, [1] block rank (-1: boundary),
  //           [2] sigma as stored per point, [3..5] lower corner of the neighbour's box, [6..8] 1 / side
  const double *meta;
  // "Sub-face" and "cell" below are what the kernel sums over; they may be MERGED ones (pdh_plan.cpp: build_terms_tables): where the
  // cells of a polytope (the sub-faces of a plane of a run) form a tensor grid, the sum over a sub-grid of them of products of three 1-D
  // matrices is the product of the three 1-D sums - one cell (sub-face) with composite rules of several intervals per direction.
  const int64_t *sf_pt;   // [n_owned][maxsf] first own-side point (ap_* arrays) of every sub-face of a polytope, run by run (rest: 0)
  const int32_t *sf_info; // run | axis << 8 | (own outward normal along +axis) << 10 | (second tangential axis runs fastest) << 11
                          // | intervals along the first tangential axis << 12 | along the second << 15
  const int32_t *sf_ivl;  // [n_owned][maxsf][2][TERMS_MI] per tangential direction: first point of every interval's rule, relative to sf_pt
  const int32_t *cell_ivl; // [n_owned][maxcell][3][TERMS_MI] per direction: the polytope's cell (rule of vq_tensor_n^3 points) that carries
                          // the 1-D rule of every interval, -1: no such interval
  int32_t task_pts;       // most points of a 1-D composite rule (vq_tensor_n / fq_tensor_n x intervals): 4 or 8 register slots per lane task
  // The 1-D rules the kernels work from, gathered ONCE per problem on the device (pdh_terms.hip: k_terms_gather) from the point arrays
  // through the descriptors above - per owned polytope one record of tstride doubles (pdh_terms.h: terms_task_doubles):
  //   task (sub-face sf, tangential direction dir) at (2 sf + dir) * 3 tpm: coordinates [tpm] | own-side weights [tpm] | side-1 weights [tpm]
  //   task (cell c, direction d) at (2 maxsf + 3 c + d) * 3 tpm: coordinates | weights | unused          (slots behind a rule: zeros)
  //   then the plane coordinate of every sub-face [maxsf] and its descriptor sf_info [maxsf] (integer bits)
  // An assembly reads these 3 KB per polytope (block agglomerates) in one contiguous request instead of chasing descriptor -> interval
  // -> point through three dependent loads into the point arrays.
  const double *tdata;
  int32_t tstride, tpm;   // tpm = 4 or 8: slots per 1-D rule in the records = PMAX of the kernel instantiation that is launched
  int32_t maxruns;        // runs a record provides for
  int32_t maxsf, maxsi, maxcell; // most sub-faces / interior sub-faces / cells of one owned polytope
  int32_t vq_tensor_n, fq_tensor_n; // verified points per direction of the sub-cell / sub-face rules
  int32_t lds_bytes;      // dynamic LDS of a workgroup for these maxima
  int32_t split;          // 1: X tables made in a second pass over the D tables (pdh_terms.h: SPLIT) - lds_bytes is that form's
  long long *stamps;      // [n_owned][16] cycle counter at the phase boundaries; written by -DPDHT_STAMP builds only
  unsigned int *sched;    // [2] pdh_terms_wg.h: work counter of its workgroups and count of those that have left (both zero between launches)
};

namespace pdht
{
constexpr int TERMS_HDR = 12, TERMS_ENT = 10;

template <int N1D, int BASIS>
struct Kind
{
  static constexpr int NF = BASIS == 0 ? N1D * N1D * N1D : N1D * (N1D + 1) * (N1D + 2) / 6; // functions
  static constexpr int NS = BASIS == 0 ? N1D * N1D : N1D * (N1D + 1) / 2;                   // pairs (k1, k2) that occur
  static constexpr int NSYM = N1D * (N1D + 1) / 2, FULL = N1D * N1D;
  static constexpr int SYMS = NSYM | 1, FULLS = FULL | 1; // odd strides: the lane tasks of phase A write table after table
  static constexpr int NSUB = 64 / NF > 0 ? 64 / NF : 1;  // subsets of the diagonal block's terms (lanes = NSUB x NF columns)
  struct Dig
  {
    int k0, k1, k2;
  };
  // digits of function R (x fastest; BASIS 1: k0 + k1 + k2 <= p, pdh_basis.h: multi_indices)
  PDH_HD static constexpr Dig dig(int R)
  {
    if (BASIS == 0)
      return Dig{R % N1D, (R / N1D) % N1D, R / (N1D * N1D)};
    int cnt = 0;
    for (int iz = 0; iz < N1D; ++iz)
      for (int iy = 0; iy < N1D - iz; ++iy)
        for (int ix = 0; ix < N1D - iy - iz; ++ix)
          {
            if (cnt == R)
              return Dig{ix, iy, iz};
            ++cnt;
          }
    return Dig{0, 0, 0};
  }
  PDH_HD static constexpr int pair(int k1, int k2) { return BASIS == 0 ? k1 + N1D * k2 : k2 * N1D - k2 * (k2 - 1) / 2 + k1; }
  PDH_HD static constexpr bool pair_ok(int k1, int k2) { return BASIS == 0 || k1 + k2 < N1D; }
  PDH_HD static constexpr int sym(int k, int l) { return k <= l ? l * (l + 1) / 2 + k : k * (k + 1) / 2 + l; }
};

// pdh_terms_wg.h, how its writers store a polytope's rows: the cache-policy bits of the row stores (gfx940+: 1 = sc0, 2 = nt, 16 = sc1)
// and whether a writer waits for its stores before the barrier that ends a step.  The one form the library ships: sc1|nt, drained -
// 2.6-3.3 % ahead of nt stores left in flight on each of eight contexts, paired on the same allocation (profiles/r14_paired_variants.txt)
constexpr int WG_STORE_AUX = 18;
constexpr bool WG_DRAIN = true;
// the form before, which -DPDHT_VARIANTS builds keep as the baseline of tools/paired_bench.py
constexpr int WG_BASE_STORE_AUX = 2;
constexpr bool WG_BASE_DRAIN = false;

// LDS of a workgroup in doubles (host and device agree through this one function)
PDH_HD constexpr int terms_rec_doubles(int maxruns) { return (TERMS_HDR + maxruns * TERMS_ENT + 1) & ~1; }
// Two-phase tables (SPLIT): the D / M / K tables are needed by the diagonal block only, the X tables by the row pieces only.  Made
// in one pass they cost FE_AggloDGP(3) on block polytopes 21 KB of LDS per wave = 7 resident waves per CU, 30-40 KB on METIS-like
// agglomerates, and the kernel runs at the speed its occupancy allows; made one after the other - the X tables from the point data
// still held in registers, behind the finished block - 13.7 KB = 11 waves, for 250 more VALU instructions per polytope (the bases
// at the tangential points are evaluated twice): 0.384 -> 0.373 ms on the bench mesh, 0.71 -> 0.56 ms on its grown agglomerates
// (profiles/r04_terms_split.txt).  The host takes the form that gives a polytope's workgroup more resident waves (PdhTerms::split).
// (BLOCK_IN_LDS: the wave-per-polytope kernel leaves the diagonal block in LDS over the dead tables; the workgroup kernel of
// pdh_terms_wg.h stores it from registers)
template <int N1D, int BASIS, bool BLOCK_IN_LDS = true, bool SPLIT = false>
PDH_HD constexpr int terms_lds_doubles(int maxruns, int maxsf, int maxsi, int maxcell)
{
  using K = Kind<N1D, BASIS>;
  const int dg = (K::NF + 1) / 2 + ((K::NF + 1) / 2 & 1);
  const int xa = maxsi * 3 * K::FULLS + ((maxsi * 3 * K::FULLS) & 1);
  int da = maxsf * 3 * K::SYMS + maxcell * 6 * K::SYMS;
  if (BLOCK_IN_LDS && SPLIT)
    { // the X tables are made after the diagonal block and stand BEHIND it, over the D tables (dead by then)
      const int xb = K::NF * K::NF + xa;
      da = da > xb ? da : xb;
      return terms_rec_doubles(maxruns) + dg + da + (da & 1);
    }
  if (BLOCK_IN_LDS)
    da = da > K::NF * K::NF ? da : K::NF * K::NF;
  return terms_rec_doubles(maxruns) + dg + xa + da + (da & 1);
}

// A polytope's record of 1-D rules (PdhTerms::tdata): the points of every (sub-face, tangential direction) and (cell, direction) task
// [task][x | w_self | w_cross][pmax], then per sub-face its plane coordinate and descriptor
PDH_HD constexpr int terms_task_doubles(int maxsf, int maxcell, int pmax)
{
  return (2 * maxsf + 3 * maxcell) * pmax * 3 + 2 * maxsf;
}

// A polytope's record of FINISHED tables in HBM (pdh_matfree.h: the matrix-free product reads them), at a fixed stride for the maxima
// of the problem: the X tables [interior sub-face][axis] (FULLS stride, entry (k, l) at l * N1D + k, k the own index) | the D tables
// [sub-face][axis] (packed symmetric, SYMS stride) | the M | K tables [cell][axis][M | K] (SYMS stride; reaction term folded into K of
// axis 0).  The strides are Kind's (they depend on N1D alone).
PDH_HD constexpr int matfree_off_d(int n1d, int maxsi) { return maxsi * 3 * ((n1d * n1d) | 1); }
PDH_HD constexpr int matfree_off_c(int n1d, int maxsf, int maxsi)
{
  return matfree_off_d(n1d, maxsi) + maxsf * 3 * ((n1d * (n1d + 1) / 2) | 1);
}
PDH_HD constexpr int matfree_rec_doubles(int n1d, int maxsf, int maxsi, int maxcell)
{
  return matfree_off_c(n1d, maxsf, maxsi) + maxcell * 6 * ((n1d * (n1d + 1) / 2) | 1);
}

// the kinds of the wave-per-polytope kernel (pdh_terms.h) that are instantiated: f(N1D, BASIS) as integral constants; false: none
template <class F>
bool for_kind(int n1d, int basis, F &&f)
{
  using std::integral_constant;
  if (n1d == 4 && basis == 1)
    f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  else if (n1d == 3 && basis == 0)
    f(integral_constant<int, 3>{}, integral_constant<int, 0>{});
  else if (n1d == 3 && basis == 1)
    f(integral_constant<int, 3>{}, integral_constant<int, 1>{});
  else if (n1d == 2 && basis == 0)
    f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
  else if (n1d == 2 && basis == 1)
    f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
  else
    return false;
  return true;
}

// 1 if the term kernel (pdh_terms.h, a wave per polytope) is instantiated for this element, 2: FE_DGQ(3), which has the
// workgroup-per-polytope kernel of pdh_terms_wg.h instead
inline int terms_has_kind(int n1d, int basis)
{
  if (n1d == 4 && basis == 0)
    return 2;
  return for_kind(n1d, basis, [](auto, auto) {}) ? 1 : 0;
}

// dynamic LDS of a workgroup for the maxima of a resident problem, bytes (0: no such kind)
// split: the two-phase form of the wave-per-polytope kernel (pdh_terms.h: SPLIT; ignored for the workgroup kernel)
inline int terms_lds_bytes(int n1d, int basis, int maxruns, int maxsf, int maxsi, int maxcell, int split)
{
  int bytes = 0;
  if (n1d == 4 && basis == 0)
    return 8 * terms_lds_doubles<4, 0, false>(maxruns, maxsf, maxsi, maxcell);
  for_kind(n1d, basis, [&](auto n_, auto b_) {
    constexpr int N = decltype(n_)::value, B = decltype(b_)::value;
    bytes = 8 * (split ? terms_lds_doubles<N, B, true, true>(maxruns, maxsf, maxsi, maxcell)
                       : terms_lds_doubles<N, B, true, false>(maxruns, maxsf, maxsi, maxcell));
  });
  return bytes;
}
} // namespace pdht
