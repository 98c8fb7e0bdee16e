// pdh_terms.hip — instantiations, resolver and launcher of the term kernel (pdh_terms.h): 3-D FE_DGQ(1,2), FE_AggloDGP(1..3).
#include "pdh_terms.h"
#include "pdh_terms_wg.h"
#include "pdh_launch.h"

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

// one workgroup per owned polytope: of one wave (pdh_terms.h), FE_DGQ(3) of wg_waves = 4 | 8 waves (pdh_terms_wg.h; PDH_TERMS_WG_WAVES,
// diagnostics).  Rules of up to 4 / up to 8 points per direction (PdhTerms::task_pts) have their own instantiations.
extern "C" PdhLaunch pdh_resolve_terms(const PdhDev *P, const PdhTerms *T, int count, int wg_waves)
{
  PdhLaunch L{};
  const int basis = P->n == P->n1d * P->n1d * P->n1d ? 0 : 1;
  const bool shifted = P->diag_first != 0, small = T->task_pts <= 4;
  if (P->n1d == 4 && basis == 0)
    pdh_for_bools(
      [&](auto eight_, auto shifted_, auto small_) {
        constexpr int W = decltype(eight_)::value ? 8 : 4, PM = decltype(small_)::value ? 4 : 8;
        const PdhTermsKernel k = pdht::k_terms_wg<W, decltype(shifted_)::value, PM>;
        L = pdh_record(k, count, PDH_WAVE * W, (size_t)T->lds_bytes);
      },
      wg_waves == 8, shifted, small);
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
extern "C" hipError_t pdh_launch_terms(const PdhLaunch *L, const PdhDev *P, const PdhTerms *T, int count, hipStream_t stream)
{
  return pdh_launch_as(PdhTermsKernel(), *L, stream, *P, *T, count);
}
