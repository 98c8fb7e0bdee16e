// pdh_moment_tables.h — layout of the table buffer of the moment form, shared by the kernels (pdh_moment.h, pdh_rows.h: device) and
// the host that fills and uploads it (pdh_basis.h: moment_tables, pdh_capi.cpp: upload_problem).  Compiles with and without HIP.
#pragma once

namespace pdhm
{
template <int N1D>
struct MT
{
  static constexpr int NA = 2 * N1D - 1; // Legendre modes 0 .. 2p
  static constexpr int NAP = NA + 1;     // padded (even: 16-byte rows)
  static constexpr int NG = 2 * N1D;     // Gauss points of the per-face table rule: exact to degree 4p+3 >= 4p
  static constexpr int PAIRS = N1D * N1D;
  static constexpr int TAB = PAIRS * NAP; // one expansion table [k][l][NAP] in the global buffer
  // In LDS the table rows and the T2 rows use a stride of NAP + 2 doubles: with 64-byte rows the 16 rows a wave
  // touches in one ds_read_b128 (lanes differing in two 1-D indices) fall on four bank groups only - a 16-way conflict
  // that made the contraction 8x slower than its instruction count; 80-byte rows are conflict-free.
  static constexpr int RS = NAP + 2;
  static constexpr int LTAB = PAIRS * RS;
  // layout of the device table buffer (doubles); filled by pdh_basis.h: moment_tables
  static constexpr int OFF_E = 0, OFF_D = TAB, OFF_FS = 2 * TAB, OFF_GX = 3 * TAB, OFF_GL = OFF_GX + NG /* [NA][NG] */,
                       OFF_BV = OFF_GL + NA * NG /* [N1D][NG] */, OFF_BD = OFF_BV + N1D * NG, SIZE = OFF_BD + N1D * NG;
};

// doubles of the table buffer of an element with n1d functions per direction (0: no moment form)
inline int moment_table_doubles(int n1d)
{
  switch (n1d)
    {
    case 2: return MT<2>::SIZE;
    case 3: return MT<3>::SIZE;
    case 4: return MT<4>::SIZE;
    }
  return 0;
}
} // namespace pdhm
