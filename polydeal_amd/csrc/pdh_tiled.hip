// pdh_tiled.hip — instantiations, resolver and launcher of the tiled kernels (pdh_tiled.h): 3-D, N1D = degree + 1 = 5 .. 8.
#include "pdh_tiled.h"
#include "pdh_launch.h"

template <int N1D>
static void resolve_n1d(bool reaction, long long ntile, int n_own, int n_items, PdhLaunch *L)
{
  const size_t lds = pdht2::lds_bytes_tdiag(3, N1D);
  // own blocks: the symmetric tiles ti == tj, then the pairs ti < tj
  const PdhTiledKernel sym = reaction ? pdht2::k_tdiag<3, N1D, true, true> : pdht2::k_tdiag<3, N1D, false, true>;
  const PdhTiledKernel pairs = reaction ? pdht2::k_tdiag<3, N1D, true, false> : pdht2::k_tdiag<3, N1D, false, false>;
  L[0] = pdh_record(sym, ntile * n_own, PDH_WAVE, lds);
  L[2] = pdh_record(pairs, ntile * (ntile - 1) / 2 * n_own, PDH_WAVE, lds);
  if (!L[0].kernel || !L[2].kernel)
    L[0] = L[2] = PdhLaunch{};
  const PdhTiledKernel coupling = pdht2::k_toffdiag<3, N1D>;
  L[1] = pdh_record(coupling, ntile * ntile * n_items, PDH_WAVE, pdht2::lds_bytes_toffdiag(3, N1D));
}

extern "C" void pdh_resolve_tiled(int dim, int n1d, int n, bool reaction, int n_own, int n_items, PdhLaunch *L)
{
  L[0] = L[1] = L[2] = PdhLaunch{};
  if (dim != 3)
    return;
  const int ntile = (n + 63) / 64;
  switch (n1d)
    {
    case 5:
      return resolve_n1d<5>(reaction, ntile, n_own, n_items, L);
    case 6:
      return resolve_n1d<6>(reaction, ntile, n_own, n_items, L);
    case 7:
      return resolve_n1d<7>(reaction, ntile, n_own, n_items, L);
    case 8:
      return resolve_n1d<8>(reaction, ntile, n_own, n_items, L);
    }
}

// the direct form of up to 64 dofs per polytope (pdh_inst.hip resolves it, one unit per group; launched here, in a unit compiled once)
extern "C" hipError_t pdh_launch_direct(const PdhLaunch *L, const PdhDev *P, int count, hipStream_t stream)
{
  return pdh_launch_as(PdhDirectKernel(), *L, stream, *P, count);
}

// count = owned polytopes / face items
extern "C" hipError_t pdh_launch_tiled(const PdhLaunch *L, const PdhDev *P, int count, hipStream_t stream)
{
  return pdh_launch_as(PdhTiledKernel(), *L, stream, *P, count, (P->n + 63) / 64);
}
