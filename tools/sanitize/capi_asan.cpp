// ASan / UBSan smoke of the planner of the C ABI (pdh_plan.cpp: validation, packing, choice of the row kernel) on flattened problems.
#include "../../polydeal_amd/csrc/host/polydeal_host.h"
#include "../../polydeal_amd/csrc/pdh_plan.h"
#include <cmath>
#include <cstdio>
using namespace polydeal_hip;
extern "C" int pdh_check_problem(const pdh_problem *, int32_t, int32_t, int64_t *);
extern "C" int pdh_check_rows(const pdh_problem *, int32_t, int32_t);
extern "C" int pdh_check_terms(const pdh_problem *, int32_t, int32_t, int64_t *);
extern "C" int pdh_check_exchange(const pdh_problem *, int32_t, int32_t, int, int64_t *, int64_t *);
extern "C" int pdh_tridiagonal_eigenvalues(int, const double *, const double *, double *, double *);
int main()
{
  for (int dim = 2; dim <= 3; ++dim)
    for (int basis = 0; basis < 2; ++basis)
      {
        BackgroundGrid g = BackgroundGrid::hyper_cube_refined(dim, 0., 1., dim == 2 ? 4 : 3);
        AgglomerationHandler ah(g);
        define_block_agglomerates(ah, 2);
        FiniteElement fe;
        fe.dim = dim;
        fe.degree = 3;
        fe.basis = basis;
        ah.initialize_fe_values(4, 4);
        ah.distribute_agglomerated_dofs(fe);
        FlatProblem F;
        ah.flatten(SipVariant::poisson_example(fe), F, true, true);
        int64_t st[8];
        const int n = fe.n_dofs_per_cell();
        const int nA = F.c.n_agg;
        int rc = pdh_check_problem(&F.c, 0, F.c.n_rows, st);
        int rc2 = pdh_check_problem(&F.c, (nA / 3) * n, (2 * nA / 3) * n, st);
        std::printf("dim %d basis %d: rc %d %d owned %lld items %lld\n", dim, basis, rc, rc2, (long long)st[0], (long long)st[1]);
        if (rc || rc2)
          return 1;
        // eligibility test of the row kernel (planes, tensor rules, per-slot records) on the whole problem and on a row range,
        // and a rank-local description with the exchange layout
        const int rr = pdh_check_rows(&F.c, 0, F.c.n_rows), rr2 = pdh_check_rows(&F.c, (nA / 3) * n, (2 * nA / 3) * n);
        std::printf("  row kernel applies: %d %d\n", rr, rr2);
        if (rr != (dim == 3 ? 1 : 0) || rr2 != rr)
          return 1;
        if (dim == 3)
          {
            // the term kernels: block agglomerates of Cartesian cells with tensor rules take them, through the kernels' own LDS
            // gate - the LDS of a workgroup is positive and within the 40 KB cap
            int64_t ts[5] = {0, 0, 0, 0, 0}, ts2[5] = {0, 0, 0, 0, 0};
            const int rt = pdh_check_terms(&F.c, 0, F.c.n_rows, ts), rt2 = pdh_check_terms(&F.c, (nA / 3) * n, (2 * nA / 3) * n, ts2);
            std::printf("  term kernel applies: %d %d, LDS bytes %lld %lld\n", rt, rt2, (long long)ts[4], (long long)ts2[4]);
            if (rt != 1 || rt2 != 1 || ts[4] <= 0 || ts[4] > 40 * 1024 || ts2[4] <= 0 || ts2[4] > 40 * 1024)
              return 1;
            FlatProblem L;
            std::vector<int> splits = {0, (nA / 2) * n, nA * n};
            ah.flatten_local(SipVariant::poisson_example(fe), L, 0, (nA / 2) * n, true, true, nullptr, &splits);
            int64_t sc[2], rcv[2];
            if (pdh_check_problem(&L.c, 0, (nA / 2) * n, st) || pdh_check_rows(&L.c, 0, (nA / 2) * n) != 1 ||
                pdh_check_exchange(&L.c, 0, (nA / 2) * n, 2, sc, rcv))
              return 1;
            std::printf("  local description: owned %lld, exchange send %lld recv %lld doubles\n", (long long)st[0], (long long)sc[1], (long long)rcv[1]);
          }
      }
  // the eigenvalue routine of the Chebyshev set-up: -1 2 -1 matrices of every size it takes (largest eigenvalue 2 - 2 cos(k pi / (k + 1))),
  // and its refusals
  for (int k = 1; k <= 256; ++k)
    {
      std::vector<double> d((size_t)k, 2.0), e((size_t)(k > 1 ? k - 1 : 0), -1.0);
      double lo = 0, hi = 0;
      if (pdh_tridiagonal_eigenvalues(k, d.data(), k > 1 ? e.data() : nullptr, &lo, &hi) != PDH_OK ||
          std::fabs(hi - (2.0 - 2.0 * std::cos(k * M_PI / (k + 1)))) > 1e-12 || std::fabs(lo - (2.0 - 2.0 * std::cos(M_PI / (k + 1)))) > 1e-12)
        {
          std::printf("pdh_tridiagonal_eigenvalues: k %d lo %.17g hi %.17g\n", k, lo, hi);
          return 1;
        }
    }
  double lo, hi, one = 1.0;
  if (pdh_tridiagonal_eigenvalues(0, &one, nullptr, &lo, &hi) != PDH_EINVAL || pdh_tridiagonal_eigenvalues(257, &one, &one, &lo, &hi) != PDH_EINVAL ||
      pdh_tridiagonal_eigenvalues(2, &one, nullptr, &lo, &hi) != PDH_EINVAL)
    return 1;
  std::printf("tridiagonal eigenvalues: k = 1 .. 256 ok\n");
  // the host arithmetic of the Chebyshev set-up.  Coefficients: every degree and range is finite, lo < hi, the first step is 1 / theta
  for (int degree = 1; degree <= 8; ++degree)
    for (double range : {2.0, 20.0, 1e6})
      {
        std::vector<double> c1, c2;
        double clo = 0, chi = 0;
        pdh_chebyshev_coefficients(degree, 1.75, range, &clo, &chi, c1, c2);
        bool ok = (int)c1.size() == degree && (int)c2.size() == degree && std::isfinite(clo) && std::isfinite(chi) && clo < chi &&
                  c2[0] == 1 / ((chi + clo) / 2);
        for (int k = 0; k < degree && ok; ++k)
          ok = std::isfinite(c1[k]) && std::isfinite(c2[k]);
        if (!ok)
          {
            std::printf("pdh_chebyshev_coefficients: degree %d range %g\n", degree, range);
            return 1;
          }
      }
  // Lanczos matrix: alpha and beta of m = 1 .. 64 CG steps on the -1 2.5 -1 matrix of size 64 (SPD, eigenvalues in (0.5, 4.5))
  {
    const int n = 64;
    auto mult = [&](const std::vector<double> &v, std::vector<double> &Av) {
      for (int i = 0; i < n; ++i)
        Av[i] = 2.5 * v[i] - (i > 0 ? v[i - 1] : 0.0) - (i + 1 < n ? v[i + 1] : 0.0);
    };
    auto dot = [&](const std::vector<double> &a, const std::vector<double> &b) {
      double s = 0;
      for (int i = 0; i < n; ++i)
        s += a[i] * b[i];
      return s;
    };
    std::vector<double> r((size_t)n), p, q((size_t)n), alpha, beta;
    for (int i = 0; i < n; ++i)
      r[i] = (double)((i * 37) % 11) - 4.5;
    p = r;
    double rr = dot(r, r);
    for (int m = 1; m <= 64; ++m)
      {
        mult(p, q);
        const double a = rr / dot(p, q);
        for (int i = 0; i < n; ++i)
          r[i] -= a * q[i];
        const double rr_new = dot(r, r), b = rr_new / rr;
        for (int i = 0; i < n; ++i)
          p[i] = r[i] + b * p[i];
        rr = rr_new;
        alpha.push_back(a);
        beta.push_back(b);
        std::vector<double> dg, od;
        pdh_lanczos_tridiagonal(alpha, beta, dg, od);
        bool ok = (int)dg.size() == m && (int)od.size() == (m > 1 ? m - 1 : 1);
        for (double v : dg)
          ok = ok && std::isfinite(v);
        for (double v : od)
          ok = ok && std::isfinite(v);
        double tlo = 0, thi = 0;
        if (!ok || pdh_tridiagonal_eigenvalues(m, dg.data(), od.data(), &tlo, &thi) != PDH_OK || !(thi > 0.0))
          {
            std::printf("pdh_lanczos_tridiagonal: m %d hi %.17g\n", m, thi);
            return 1;
          }
      }
  }
  std::printf("chebyshev coefficients: degrees 1 .. 8 ok; lanczos matrices: m = 1 .. 64 ok\n");
  return 0;
}
