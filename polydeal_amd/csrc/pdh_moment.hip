// pdh_moment.hip — instantiations, resolvers and launchers of the moment-form kernels (pdh_moment.h: 3-D, degree <= 3) and of the row
// kernel (pdh_rows.h).
#include <cstdio>
#include "pdh_moment.h"
#include "pdh_rows.h"
#include "pdh_launch.h"

using std::integral_constant;

// L[0]: diagonal blocks of the n_own owned polytopes, L[1]: coupling blocks of the n_items interior-face items
extern "C" void pdh_resolve_moment(int n1d, int n, int n_own, int n_items, PdhLaunch *L)
{
  L[0] = L[1] = PdhLaunch{};
  auto pick = [&](auto n1d_, auto mfma_) {
    constexpr int N = decltype(n1d_)::value;
    constexpr bool MFMA = decltype(mfma_)::value;
    const PdhMomentKernel diag = pdhm::k_mdiag<N, MFMA>, off = pdhm::k_moffdiag<N, MFMA>;
    L[0] = pdh_record(diag, n_own, PDH_WAVE, pdhm::lds_doubles_diag<N>() * sizeof(double));
    L[1] = pdh_record(off, n_items, PDH_WAVE, pdhm::lds_doubles_offdiag<N>() * sizeof(double));
  };
  if (n1d == 4 && n == 64) // FE_DGQ(3): contraction stages 2 and 3 on the MFMA
    pick(integral_constant<int, 4>{}, std::true_type{});
  else if (n1d == 4)
    pick(integral_constant<int, 4>{}, std::false_type{});
  else if (n1d == 3)
    pick(integral_constant<int, 3>{}, std::false_type{});
  else if (n1d == 2)
    pick(integral_constant<int, 2>{}, std::false_type{});
}
extern "C" hipError_t pdh_launch_moment(const PdhLaunch *L, const PdhDev *P, const double *mtab, int count, hipStream_t stream)
{
  return pdh_launch_as(PdhMomentKernel(), *L, stream, *P, mtab, count);
}

// the kinds of the row kernel (pdh_rows.h: RowsKind), as pdht::for_kind has those of the term kernel
template <class F>
static void for_rows_kind(int n1d, int basis, F &&f)
{
  if (n1d == 4 && basis == 0)
    f(integral_constant<int, 4>{}, integral_constant<int, 0>{});
  else if (n1d == 4)
    f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  else if (n1d == 3 && basis == 0)
    f(integral_constant<int, 3>{}, integral_constant<int, 0>{});
  else if (n1d == 3)
    f(integral_constant<int, 3>{}, integral_constant<int, 1>{});
  else if (n1d == 2 && basis == 0)
    f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
  else if (n1d == 2)
    f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
}

// Row kernel (pdh_rows.h): one wave per owned polytope writes all blocks of its rows; FE_DGQ(3) or FE_AggloDGP(3) in 3-D,
// axis-aligned planar faces.  FE_DGQ(3) is the row-piece kernel, the other kinds stream their rows.
extern "C" PdhLaunch pdh_resolve_rows(const PdhDev *P, const PdhRows *R, int count, int cus, int waves_per_cu, size_t lds_pad, bool verbose,
                                      bool *zero_sched)
{
  PdhLaunch L{};
  *zero_sched = false;
  const int basis = P->n == P->n1d * P->n1d * P->n1d ? 0 : 1;
  for_rows_kind(P->n1d, basis, [&](auto n1d_, auto basis_) {
    constexpr int N = decltype(n1d_)::value, B = decltype(basis_)::value;
    if (P->n != pdhr::RowsKind<N, B>::NF)
      return;
    *zero_sched = !pdhr::RowsKind<N, B>::SMALL;
    // (MULTI: the coupling moments of the interior entries are parked in PdhRows::m2c_scratch, not in LDS - the layout of the
    // block-shaped kernel, whose six slots serve as staging there).  lds_pad (PDH_ROWS_LDS_PAD, diagnostics): fewer resident waves
    // per CU, to see how the kernel's time scales with occupancy (tools/README)
    const size_t lds = pdhr::lds_doubles_rows<N, B>() * sizeof(double) + lds_pad;
    // degree 3: the instantiation without general-point paths when the host verified tensor rules everywhere (PdhRows::tensor_only,
    // pdh_plan.cpp: rows_kind_applies); MULTI (FE_DGQ(3), PdhRows::multi): the coupling-moment slots, one per interior plane entry,
    // are sized for the resident problem
    pdh_for_bools(
      [&](auto general_, auto shifted_, auto multi_) {
        constexpr bool G = decltype(general_)::value, S = decltype(shifted_)::value, MU = decltype(multi_)::value;
        if constexpr ((N == 4 || !G) && ((N == 4 && B == 0) || !MU))
          {
            const PdhRowsKernel k = pdhr::k_rows<N, B, G, S, MU>;
            // persistent waves: as many single-wave workgroups as fit on the device at once, each working through slots blockIdx.x,
            // blockIdx.x + gridDim.x, ...  Resident per CU: by LDS (160 KB, handed out in granules of 1280 bytes - measured: 26 624
            // bytes fit six times, 27 136 do not) and by the registers of the instantiation (the runtime's occupancy query: two
            // waves per SIMD above 168 VGPRs, three up to 168); waves_per_cu (PDH_ROWS_WAVES_PER_CU, diagnostics) overrides
            const int fit_lds = (int)(160 * 1024 / ((lds + 1279) / 1280 * 1280));
            int occ = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, PDH_WAVE, lds) != hipSuccess || occ < 1)
              occ = 8;
            const int per_cu = waves_per_cu > 0 ? waves_per_cu : (fit_lds < occ ? fit_lds : occ);
            int resident = cus * per_cu;
            if (MU && resident > R->scratch_waves)
              resident = R->scratch_waves; // (one row of the moment scratch per workgroup)
            L = pdh_record(k, count < resident ? count : resident, PDH_WAVE, lds);
            if (verbose)
              fprintf(stderr, "k_rows<%d,%d,%d,%d,%d>: lds %zu bytes, resident waves per CU: %d by LDS, %d by the occupancy query, %d taken, grid %u\n",
                      N, B, (int)G, (int)S, (int)MU, lds, fit_lds, occ, per_cu, L.grid);
          }
      },
      N == 4 && !R->tensor_only, P->diag_first != 0, N == 4 && B == 0 && R->multi != 0);
  });
  return L;
}
extern "C" hipError_t pdh_launch_rows(const PdhLaunch *L, bool zero_sched, const PdhDev *P, const PdhRows *R, const double *mtab, int count,
                                      hipStream_t stream)
{
  // FE_DGQ(3) (zero_sched): the work counter and the count of leavers start every launch at zero.  The last wave out of a launch resets them, but a
  // launch that was aborted, or two launches of one context overlapping after a change of stream, would leave them dirty -
  // and a dirty counter silently skips or repeats polytopes.  Eight bytes, stream-ordered in front of the kernel.
  if (zero_sched && L->kernel && L->grid)
    if (const hipError_t e = hipMemsetAsync(R->sched, 0, 2 * sizeof(unsigned int), stream); e != hipSuccess)
      return e;
  return pdh_launch_as(PdhRowsKernel(), *L, stream, *P, *R, mtab, count);
}
