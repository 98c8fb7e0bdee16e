// pdh_plan.h — the host-only planner of a problem (pdh_plan.cpp): validation and repacking of a description (Packed) and the choice
// of the row kernel with its host tables (KernelPlan).  No HIP here or in anything it includes: pdh_set_problem (pdh_capi.cpp) uploads
// what the planner built, the pdh_check_* entry points (pdh_plan.cpp) run it on machines without a GPU.
#pragma once
#include "../../include/polydeal_hip.h"
#include "pdh_dev.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

// setup-time loops over all quadrature points run on all host threads (PDH_HOST_THREADS overrides the count)
template <class F>
void host_parallel_for(size_t n, F &&fn)
{
  unsigned nt = std::thread::hardware_concurrency();
  if (const char *e = std::getenv("PDH_HOST_THREADS"))
    nt = (unsigned)std::max(1, std::atoi(e));
  nt = std::max(1u, std::min<unsigned>(nt, 64u));
  if (nt == 1 || n < 256)
    {
      for (size_t i = 0; i < n; ++i)
        fn(i);
      return;
    }
  std::vector<std::thread> th;
  const size_t chunk = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; ++t)
    {
      const size_t b = (size_t)t * chunk, e = std::min(n, b + chunk);
      if (b >= e)
        break;
      th.emplace_back([&fn, b, e] {
        for (size_t i = b; i < e; ++i)
          fn(i);
      });
    }
  for (auto &t : th)
    t.join();
}

// which row kernel serves a problem (plan_kernels): none, the kinds of pdh_rows.h, or the term kernels (pdh_terms.h /
// pdh_terms_wg.h)
enum class RowKernel { none, rows, terms };

// std::vector whose resize() leaves the new elements uninitialised: the big point arrays are filled by all host threads
// right after they are sized, a serial zero-fill of 1.3 GB in between costs more than the fill itself
template <class T>
struct UninitAlloc : std::allocator<T>
{
  template <class U>
  struct rebind { using other = UninitAlloc<U>; };
  template <class U, class... A>
  void construct(U *ptr, A &&...a)
  {
    if constexpr (sizeof...(A) == 0)
      ::new ((void *)ptr) U;
    else
      ::new ((void *)ptr) U(std::forward<A>(a)...);
  }
};
using dvec = std::vector<double, UninitAlloc<double>>;

struct Packed
{
  int n = 0, n1d = 0, NT = 0, LB = 0;
  bool tiled = false; // n > 64: blocks in 64 x 64 tiles (pdh_tiled.h)
  std::vector<int32_t> midx;
  PdhBasisTab tab;
  std::vector<int32_t> own_agg, own_row, row_len, diag_L, it_own, it_nbr, it_pcnt, it_pos, it_nbr_slot, it_pos_t;
  std::vector<int64_t> row_base, vq_ptr, ap_ptr, it_pbeg;
  // per owned slot: first global dof of every coupled block in value order (CSR; pdh_solve.h), and the longest row
  std::vector<int64_t> blk_ptr{0};
  std::vector<int32_t> blk_dof;
  int max_row_len = 0;
  dvec vq_x, vq_w;
  // Own-side face points are NOT built on the host: set_problem uploads the caller's face arrays as they are and a kernel
  // (pdh_exchange.hip: k_pack_faces) writes the per-polytope runs in HBM from these tables - one entry per run, owned slots
  // first, then the pseudo slots of the exchange variant: first packed point, first caller point, count, flags
  // (bit 0: the polytope is side 0 of the face, bit 1: boundary face), sigma of the face
  std::vector<int64_t> pk_at, pk_fq;
  std::vector<int32_t> pk_cnt, pk_flags;
  std::vector<double> pk_sig;
  int64_t n_ap = 0;
  // volume points of the owned slots: the caller's own arrays when the slots are its polytopes in its order (no copy),
  // else vq_x / vq_w above; [dim][vq_stride] and [n_vq]
  const double *vqx_h = nullptr, *vqw_h = nullptr;
  int64_t vq_stride_h = 0, n_vq = 0;
  std::vector<int64_t> vq_src, run_ap, run_fq;
  std::vector<int32_t> run_cnt, run_bdry;
  // per run (owned slots only, same order): owning slot, neighbour polytope (-1 boundary) and the ascending rank of the
  // neighbour's block in the slot's rows, penalty as stored per point - input of the row kernel's face table (pdh_rows.h)
  std::vector<int32_t> run_slot, run_nbr, run_blk;
  std::vector<double> run_sig;
  // pdh_set_problem_cartesian: the point arrays of `src` are NULL, the points are generated on the device from these
  const pdh_cartesian_points *cart = nullptr;
  bool ghost = false; // packed for the ghost-block exchange (PDH_EXCHANGE_GHOST)
  // host view of a packed face point (what the kernel writes): run r of the owned slots, point q of the run
  const pdh_problem *src = nullptr;
  int64_t nqf_src = 0;
  double ap_x(int d, size_t r, int64_t q) const { return src->fq_x[d * nqf_src + pk_fq[r] + q]; }
  double ap_n(int d, size_t r, int64_t q) const { return ((pk_flags[r] & 1) ? 1.0 : -1.0) * src->fq_n[d * nqf_src + pk_fq[r] + q]; }
  double ap_wself(size_t r, int64_t q) const
  {
    const int64_t i = pk_fq[r] + q;
    if (pk_flags[r] & 2)
      return 2.0 * src->fq_w[i];
    return ((pk_flags[r] & 1) || !src->fq_w_out) ? src->fq_w[i] : src->fq_w_out[i];
  }
  double ap_wcross(size_t r, int64_t q) const
  {
    const int64_t i = pk_fq[r] + q;
    return (pk_flags[r] & 2) ? 0.0 : (src->fq_w_out ? src->fq_w_out[i] : src->fq_w[i]);
  }
  int64_t n_values = 0;
  int n_owned = 0; // own_agg / ap_ptr / ... may carry pseudo slots behind the owned ones (ghost-block exchange)
  // ghost-block exchange (PDH_EXCHANGE_GHOST): doubles per peer rank, and where the received blocks go
  std::vector<int64_t> send_count, recv_count;
  int64_t n_send = 0, n_recv = 0;
  std::vector<int32_t> r21_rlen, r22_slot;
  std::vector<int64_t> r21_src, r21_dst, r22_ptr, r22_src;
};

struct RowsHost
{
  std::vector<int32_t> fr_ptr, fr_pcnt, fr_nbr, fr_axis, fr_blk, fr_flags;
  std::vector<int64_t> fr_pbeg;
  std::vector<double> fr_coord, fr_sigma, fr_nsign;
  std::vector<double> meta; // per-slot records of the kernel (pdh_rows.h: 12 + 12 maxe doubles each)
  int fq_tensor_n = 0; // verified (or detected) points per direction of the sub-face rules, 0: none
  // pdh_rows.h, MULTI instantiation: some neighbour is met along several planes, or a polytope has more interior plane
  // entries / entries than the block-shaped kernel provides for (6 / 16)
  bool multi = false;
  int maxe = 16, maxf = 6;
  int maxs = 0; // most sub-faces (groups of a tensor rule) of the interior entries of one polytope
  // every face point of every owned polytope has an axis-aligned normal and lies in the plane of its sub-face: established
  // before the element-specific limits of the kinds of pdh_rows.h are looked at (the term kernel, pdh_terms.h, needs no more)
  bool planar_ok = false;
  std::vector<signed char> fast_j; // per run and normal axis: does the second tangential axis run fastest in the sub-face rules?
};

// Tables of the term kernel (pdh_terms.h): per owned polytope one record (header + one entry per run = polytopal face, the
// boundary run first, then ascending block rank) and the list of its sub-faces (groups of a verified tensor rule), run by run:
// first own-side point, run, normal axis and sign, orientation of the rule.  Applies when build_rows_tables established planar
// axis-aligned faces (RowsHost::planar_ok) and both kinds of rule are verified tensor rules; any number of planes per neighbour.
struct TermsHost
{
  std::vector<double> meta;
  std::vector<int64_t> sf_pt;
  std::vector<int32_t> sf_info, sf_ivl, cell_ivl;
  int maxruns = 0, maxsf = 0, maxsi = 0, maxcell = 0, lds_bytes = 0, split = 0, task_pts = 0;
  int64_t n_cells_in = 0, n_cells_out = 0, n_sf_in = 0, n_sf_out = 0; // before / after merging (reporting)
};

// ---- which row kernel serves a problem ----------------------------------------------------------------------------------------------
// Decided on the host, before anything of the problem goes to the device; pdh_set_problem and the pdh_check_* functions share it.
// AUTO prefers the term kernels (pdh_terms.h; FE_DGQ(3): pdh_terms_wg.h) to the kinds of pdh_rows.h wherever both apply.
struct KernelPlan
{
  RowKernel kernel = RowKernel::none;
  RowsHost rows;  // tables of pdh_rows.h (cartesian description: what the term kernels need of them, by construction)
  TermsHost terms;
  int vq_n = -1;  // points per direction of the verified tensor volume rules, 0: none, -1: not looked at
  bool tensor_only = false;
  std::string why_rows, why_terms; // why each family refuses the problem
};

// Validates the description and repacks it for the owned rows [row_begin, row_end).  A failure returns its PDH_E* code and leaves the
// message in `err` (the context's string, or pdh_noctx_error()).
int pack_problem(std::string &err, const pdh_problem *p, int32_t row_begin, int32_t row_end, Packed &K,
                 int exchange_mode = PDH_EXCHANGE_NONE, const pdh_cartesian_points *cart = nullptr);

// The diagnostic switches of the library: PDH_TERMS_MERGE (0, 2, else 1), PDH_TERMS_SPLIT (0 / 1, unset: -1), PDH_TRACE_SETUP,
// PDH_ROWS_VERBOSE, PDH_TERMS=0, PDH_TERMS_DGQ3=0 for the planner; PDH_ROWS_WAVES_PER_CU (> 0: resident waves per CU of the row kernel),
// PDH_ROWS_LDS_PAD (bytes), PDH_TERMS_WG_WAVES (writer waves: 4, else 8) and PDH_TERMS_WG_BATCH (N > 0: ceil(n_owned / N) workgroups, so that
// small problems reach workgroups of several polytopes) for the resolvers of the launches (pdh_launch.h).  read_plan_switches is
// the library's only reader of the environment but for PDH_HOST_THREADS above; pdh_set_problem* and pdh_check_* call it on every call, so
// every switch takes effect at the next set-up and holds for that resident problem (the tests compare the kernels in one process).
struct PlanSwitches
{
  int terms_merge = 1, terms_split = -1;
  bool trace = false, rows_verbose = false, terms_off = false, terms_dgq3_off = false;
  int rows_waves_per_cu = 0, terms_wg_waves = 8, terms_wg_batch = 0;
  size_t rows_lds_pad = 0;
};
PlanSwitches read_plan_switches();

KernelPlan plan_kernels(const pdh_problem *p, const Packed &K, const PlanSwitches &sw);

// translation-unit group holding the kernels of a combo (pdh_combos.h), or -1 if that combo is not instantiated
int combo_group(int dim, int n1d, int nt, int lb);

// the error string of calls without a context (per thread): what pdh_last_error(NULL) returns
std::string &pdh_noctx_error();

// ---- host arithmetic of pdh_setup_chebyshev (the driver calls these; plain C++, not part of the C ABI) --------------------------------
// Lanczos matrix of m >= 1 steps of preconditioned CG (step lengths alpha, ratios beta = r'z_new / r'z_old): its diagonal [m] and
// off-diagonal [max(m - 1, 1)], the input of pdh_tridiagonal_eigenvalues
void pdh_lanczos_tridiagonal(const std::vector<double> &alpha, const std::vector<double> &beta, std::vector<double> &diag,
                             std::vector<double> &offdiag);
// Chebyshev iteration of `degree` steps on [lambda_hi / smoothing_range, lambda_hi], lambda_hi = 1.2 estimate: per step k the
// factors c1[k] of d_(k-1) and c2[k] of P^-1 r_k in d_k (step 0: 0 and 1 / theta, theta the centre of the interval)
void pdh_chebyshev_coefficients(int degree, double estimate, double smoothing_range, double *lambda_lo, double *lambda_hi,
                                std::vector<double> &c1, std::vector<double> &c2);
