// pdh_matfree.hip — instantiations and launchers of the matrix-free SIP operator (pdh_matfree.h): 3-D FE_DGQ(1..3), FE_AggloDGP(1..3).
#include "pdh_matfree.h"
#include "pdh_launch.h"

namespace
{
// f(N1D, BASIS) as integral constants for the six kinds of the term kernels; false: none
template <class F>
bool for_mf_kind(int n1d, int n, F &&f)
{
  using std::integral_constant;
  bool done = false;
  auto offer = [&](auto n_, auto b_) {
    constexpr int N = decltype(n_)::value, B = decltype(b_)::value;
    if (!done && n1d == N && n == pdht::Kind<N, B>::NF)
      {
        f(n_, b_);
        done = true;
      }
  };
  offer(integral_constant<int, 2>{}, integral_constant<int, 0>{});
  offer(integral_constant<int, 2>{}, integral_constant<int, 1>{});
  offer(integral_constant<int, 3>{}, integral_constant<int, 0>{});
  offer(integral_constant<int, 3>{}, integral_constant<int, 1>{});
  offer(integral_constant<int, 4>{}, integral_constant<int, 0>{});
  offer(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  return done;
}
} // namespace

extern "C" hipError_t pdh_launch_mf_tables(const PdhDev *P, const PdhTerms *T, double *out, int count, hipStream_t stream)
{
  if (count <= 0)
    return hipSuccess;
  const bool found = for_mf_kind(P->n1d, P->n, [&](auto n_, auto b_) {
    constexpr int N = decltype(n_)::value, B = decltype(b_)::value;
    if (T->tpm > 4)
      hipLaunchKernelGGL((pdht::k_mf_tables<N, B, true>), dim3((unsigned)count), dim3(PDH_WAVE), 0, stream, *P, *T, out, count);
    else
      hipLaunchKernelGGL((pdht::k_mf_tables<N, B, false>), dim3((unsigned)count), dim3(PDH_WAVE), 0, stream, *P, *T, out, count);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

extern "C" hipError_t pdh_launch_mf_vmult(const PdhSolveArgs *A, int n1d, const PdhTerms *T, const double *tables, const double *x, double *y,
                                          double *part, hipStream_t stream)
{
  if (A->n_owned <= 0)
    return hipSuccess;
  const bool found = for_mf_kind(n1d, A->n, [&](auto n_, auto b_) {
    constexpr int N = decltype(n_)::value, B = decltype(b_)::value;
    hipLaunchKernelGGL((pdht::k_mf_vmult<N, B>), dim3((unsigned)A->n_owned), dim3(PDH_WAVE), 0, stream, *A, *T, tables, x, y, part);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}
