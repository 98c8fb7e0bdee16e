// pdh_inst.hip — one translation unit per PDH_GROUP: instantiates k_diag (with and without reaction
// term) and k_offdiag for the combos of that group (pdh_combos.h) and resolves their launches (pdh_launch.h).
#include "pdh_combos.h"
#include "pdh_kernels.h"
#include "pdh_launch.h"

#ifndef PDH_GROUP
#error "compile with -DPDH_GROUP=0..7"
#endif

#define PDH_CAT_(a, b) a##b
#define PDH_CAT(a, b) PDH_CAT_(a, b)

#define PDH_RESOLVE_CASE(D, N, T, L)                                                                      \
  if (dim == D && n1d == N && nt == T && lb == L)                                                          \
    {                                                                                                      \
      const PdhDirectKernel own = reaction ? pdh::k_diag<D, N, T, L, true> : pdh::k_diag<D, N, T, L, false>; \
      const PdhDirectKernel off = pdh::k_offdiag<D, N, T, L>;                                              \
      out[0] = pdh_record(own, n_own, PDH_WAVE, pdh::lds_bytes_diag(D, N, T));                             \
      out[1] = pdh_record(off, n_items, PDH_WAVE, pdh::lds_bytes_offdiag(D, N, T));                        \
    }
#define PDH_SKIP(D, N, T, L)
#define PDH_SEL_0 PDH_SKIP
#define PDH_SEL_1 PDH_SKIP
#define PDH_SEL_2 PDH_SKIP
#define PDH_SEL_3 PDH_SKIP
#define PDH_SEL_4 PDH_SKIP
#define PDH_SEL_5 PDH_SKIP
#define PDH_SEL_6 PDH_SKIP
#define PDH_SEL_7 PDH_SKIP
#if PDH_GROUP == 0
#undef PDH_SEL_0
#define PDH_SEL_0 PDH_RESOLVE_CASE
#elif PDH_GROUP == 1
#undef PDH_SEL_1
#define PDH_SEL_1 PDH_RESOLVE_CASE
#elif PDH_GROUP == 2
#undef PDH_SEL_2
#define PDH_SEL_2 PDH_RESOLVE_CASE
#elif PDH_GROUP == 3
#undef PDH_SEL_3
#define PDH_SEL_3 PDH_RESOLVE_CASE
#elif PDH_GROUP == 4
#undef PDH_SEL_4
#define PDH_SEL_4 PDH_RESOLVE_CASE
#elif PDH_GROUP == 5
#undef PDH_SEL_5
#define PDH_SEL_5 PDH_RESOLVE_CASE
#elif PDH_GROUP == 6
#undef PDH_SEL_6
#define PDH_SEL_6 PDH_RESOLVE_CASE
#elif PDH_GROUP == 7
#undef PDH_SEL_7
#define PDH_SEL_7 PDH_RESOLVE_CASE
#endif
#define PDH_X(G, D, N, T, L) PDH_CAT(PDH_SEL_, G)(D, N, T, L)

// out[0]: k_diag (reaction: with reaction term) over the n_own owned slots, out[1]: k_offdiag over the n_items face items
extern "C" void PDH_CAT(pdh_resolve_g, PDH_GROUP)(int dim, int n1d, int nt, int lb, bool reaction, int n_own, int n_items, PdhLaunch *out)
{
  out[0] = out[1] = PdhLaunch{};
  PDH_COMBOS(PDH_X)
}
