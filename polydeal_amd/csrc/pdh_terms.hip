// pdh_terms.hip — instantiations, resolver and launcher of the term kernel (pdh_terms.h): 3-D FE_DGQ(1,2), FE_AggloDGP(1..3).
#include "pdh_terms.h"
#include "pdh_terms_wg.h"
#include "pdh_launch.h"

#include <algorithm>

using pdht::for_kind;

// Set-up, once per problem: the records of 1-D rules (PdhTerms::tdata) from the point arrays resident in HBM
__global__ void __launch_bounds__(PDH_WAVE) k_terms_gather(const PdhDev P, const PdhTerms T, double *__restrict__ out, const int n_owned)
{
  const int slot = blockIdx.x;
  if (slot < n_owned)
    pdht::terms_gather_record(P, T, slot, threadIdx.x, PDH_WAVE, out + (int64_t)slot * T.tstride);
}
extern "C" hipError_t pdh_launch_terms_gather(const PdhDev *P, const PdhTerms *T, double *out, int count, hipStream_t stream)
{
  if (count <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(k_terms_gather, dim3((unsigned)count), dim3(PDH_WAVE), 0, stream, *P, *T, out, count);
  return hipGetLastError();
}

// The wave-per-polytope kernel (pdh_terms.h): one workgroup per owned polytope.  FE_DGQ(3) (pdh_terms_wg.h): workgroups of wg_waves = 8 | 4
// writer waves (PDH_TERMS_WG_WAVES) and 4 builder waves, each ALONE on its CU: it asks for just over half of the CU's LDS as the device
// reports it (its two table buffers always fit: the planner caps PdhTerms::lds_bytes at 40 KB, a quarter of a CDNA CU's 160 KB), and
// nothing is resolved unless the occupancy query confirms one workgroup per CU - *why then says what failed, for the error of the
// set-up.  The workgroups take the polytopes from a device-wide counter: min(count, cus) of them, or ceil(count / wg_batch) on request
// (PDH_TERMS_WG_BATCH, so that a small test reaches workgroups of several polytopes).  Rules of up to 4 / up to 8 points per direction
// (PdhTerms::task_pts) have their own instantiations.
// store_aux, drain: how the writers of the FE_DGQ(3) kernel store (template arguments AUX, DRAIN of its body).  The library holds the
// defaults of pdh_terms_tables.h alone (k_terms_wg); a -DPDHT_VARIANTS build also the baseline they were measured against
// (k_terms_wg_base: WG_BASE_*).
extern "C" PdhLaunch pdh_resolve_terms(const PdhDev *P, const PdhTerms *T, int count, int cus, int wg_waves, int wg_batch, int store_aux,
                                       int drain, const char **why)
{
  PdhLaunch L{};
  *why = "no instantiation of the term kernel for this element, or a grid beyond 2^31 - 1 workgroups";
  const int basis = P->n == P->n1d * P->n1d * P->n1d ? 0 : 1;
  const bool shifted = P->diag_first != 0, small = T->task_pts <= 4;
  if (P->n1d == 4 && basis == 0)
    pdh_for_bools(
      [&](auto eight_, auto shifted_, auto small_) {
        constexpr int W = decltype(eight_)::value ? 8 : 4, PM = decltype(small_)::value ? 4 : 8;
        constexpr bool SH = decltype(shifted_)::value;
        constexpr unsigned block = PDH_WAVE * (W + pdht::WG_BUILDERS);
        PdhTermsKernel k = nullptr;
        if (store_aux == pdht::WG_STORE_AUX && (drain != 0) == pdht::WG_DRAIN)
          k = pdht::k_terms_wg<W, SH, PM>;
#ifdef PDHT_VARIANTS
        else if (store_aux == pdht::WG_BASE_STORE_AUX && (drain != 0) == pdht::WG_BASE_DRAIN)
          k = pdht::k_terms_wg_base<W, SH, PM>;
#endif
        if (!k)
          {
            *why = "FE_DGQ(3) term kernel: this store policy of the writers is not instantiated (the library: sc1 nt stores, drained; "
                   "diagnostic builds -DPDHT_VARIANTS also nt stores left in flight)";
            return;
          }
        int dev = 0, cu_lds = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cu_lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || cu_lds <= 0)
          {
            (void)hipGetLastError();
            *why = "FE_DGQ(3) term kernel: the device does not report the LDS of a compute unit";
            return;
          }
        const size_t lds = (size_t)cu_lds / 2 + 1024;
        if (lds < 2 * (size_t)T->lds_bytes + 64)
          {
            *why = "FE_DGQ(3) term kernel: two table buffers do not fit the LDS request that keeps a workgroup alone on its compute unit";
            return;
          }
        int per_cu = 0;
        if (hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
          {
            (void)hipGetLastError();
            *why = "FE_DGQ(3) term kernel: the device refuses the dynamic LDS of its workgroup (hipFuncSetAttribute)";
            return;
          }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, (int)block, lds) != hipSuccess || per_cu != 1)
          {
            (void)hipGetLastError();
            *why = "FE_DGQ(3) term kernel: the occupancy query does not answer one workgroup per compute unit";
            return;
          }
        const long long n = count > 0 ? count : 0;
        const long long grid = wg_batch > 0 ? (n + wg_batch - 1) / wg_batch : std::min<long long>(n, cus > 0 ? cus : 1);
        L = pdh_record(k, grid, block, lds);
      },
      wg_waves != 4, shifted, small);
  else
    for_kind(P->n1d, basis, [&](auto n_, auto b_) {
      constexpr int N = decltype(n_)::value, B = decltype(b_)::value;
      if (P->n != pdht::Kind<N, B>::NF)
        return;
      pdh_for_bools(
        [&](auto shifted_, auto small_, auto split_) {
          constexpr int PM = decltype(small_)::value ? 4 : 8;
          const PdhTermsKernel k = pdht::k_terms<N, B, decltype(shifted_)::value, PM, decltype(split_)::value>;
          L = pdh_record(k, count, PDH_WAVE, (size_t)T->lds_bytes);
        },
        shifted, small, T->split != 0);
    });
  return L;
}
// (pdh_terms_wg.h: the launches of one resident problem share PdhTerms::sched, which a launch leaves at zero for the next - they must be
// issued in ONE stream, one behind the other, as pdh_assemble_device does on the context's stream)
extern "C" hipError_t pdh_launch_terms(const PdhLaunch *L, const PdhDev *P, const PdhTerms *T, int count, hipStream_t stream)
{
  return pdh_launch_as(PdhTermsKernel(), *L, stream, *P, *T, count);
}
