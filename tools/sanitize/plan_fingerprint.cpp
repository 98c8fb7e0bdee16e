// Fingerprint of the planner's output (pdh_plan.cpp): for a fixed list of small descriptions, the return code and message of
// pack_problem, the choice of plan_kernels and, field by field as name:elements:hash, a 64-bit FNV-1a hash of every table the driver
// reads (scalars as name=value; four fields to a line, which keeps the recorded text small).  tests/data/plan_fingerprint.txt
// holds the expected text (tests/test_plan_fingerprint.py compares); a change to the planner that MEANS to alter a table regenerates
// that file with this tool.  Host only:
//   g++ -std=c++17 -O1 -ffp-contract=off -pthread -I include -I polydeal_amd/csrc polydeal_amd/csrc/pdh_plan.cpp
//       tools/sanitize/plan_fingerprint.cpp
// -DPLAN_FINGERPRINT_BOOL_SWITCHES builds it against a planner whose plan_kernels still takes `bool switches` (the commit before
// PlanSwitches: how the expected text was first produced).
#include "../../polydeal_amd/csrc/host/polydeal_host.h"
#include "../../polydeal_amd/csrc/pdh_plan.h"
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
using namespace polydeal_hip;

static std::string out;                  // text of the case being printed
static std::vector<std::string> pending; // fields not yet written
static void flush()
{
  for (size_t i = 0; i < pending.size(); ++i)
    out += (i % 4 ? " " : "  ") + pending[i] + (i % 4 == 3 || i + 1 == pending.size() ? "\n" : "");
  pending.clear();
}
static std::string text(const char *fmt, ...)
{
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}
#define put(...) (flush(), out += text(__VA_ARGS__))
static uint64_t fnv1a(const void *data, size_t bytes)
{
  uint64_t h = 1469598103934665603ull;
  const unsigned char *b = (const unsigned char *)data;
  for (size_t i = 0; i < bytes; ++i)
    h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
static void raw(const char *name, const void *data, size_t count, size_t size)
{
  pending.push_back(text("%s:%zu:%016" PRIx64, name, count, fnv1a(data, count * size)));
}
template <class V>
static void vec(const char *name, const V &v)
{
  raw(name, v.data(), v.size(), sizeof(v[0]));
}
static void num(const char *name, long long v) { pending.push_back(text("%s=%lld", name, v)); }
#define VEC(S, f) vec(#f, S.f)
#define NUM(S, f) num(#f, (long long)S.f)

static KernelPlan plan_like_check(const pdh_problem *p, const Packed &K)
{ // as the pdh_check_* entry points: PDH_TERMS_MERGE / PDH_TERMS_SPLIT honoured, PDH_TERMS / PDH_TERMS_DGQ3 not
#ifdef PLAN_FINGERPRINT_BOOL_SWITCHES
  return plan_kernels(p, K, false);
#else
  PlanSwitches s = read_plan_switches();
  s.terms_off = s.terms_dgq3_off = false;
  return plan_kernels(p, K, s);
#endif
}

static void env(const char *name, const char *value) { value ? setenv(name, value, 1) : unsetenv(name); }
struct Switches { const char *merge, *split; }; // values of PDH_TERMS_MERGE / PDH_TERMS_SPLIT, nullptr: unset

// the packed problem once, then the plan under every setting of the switches
static std::string fingerprint(const std::string &label, const pdh_problem *p, int rb, int re, int mode = PDH_EXCHANGE_NONE,
                               const pdh_cartesian_points *cart = nullptr, const std::vector<Switches> &settings = {{nullptr, nullptr}})
{
  out.clear();
  put("== %s\n", label.c_str());
  std::string err;
  Packed K;
  const int rc = pack_problem(err, p, rb, re, K, mode, cart);
  put("  rc %d \"%s\"\n", rc, err.c_str());
  if (rc != PDH_OK)
    return out;
  put("  Packed\n");
  NUM(K, n), NUM(K, n1d), NUM(K, NT), NUM(K, LB), NUM(K, tiled), NUM(K, ghost), NUM(K, n_owned), NUM(K, n_values), NUM(K, n_vq), NUM(K, n_ap);
  NUM(K, vq_stride_h), NUM(K, max_row_len), NUM(K, n_send), NUM(K, n_recv);
  raw("tab", &K.tab, 1, sizeof(K.tab));
  VEC(K, midx), VEC(K, own_agg), VEC(K, own_row), VEC(K, row_len), VEC(K, diag_L), VEC(K, row_base), VEC(K, vq_ptr), VEC(K, ap_ptr);
  VEC(K, it_own), VEC(K, it_nbr), VEC(K, it_pbeg), VEC(K, it_pcnt), VEC(K, it_pos), VEC(K, it_nbr_slot), VEC(K, it_pos_t);
  VEC(K, blk_ptr), VEC(K, blk_dof), VEC(K, pk_at), VEC(K, pk_fq), VEC(K, pk_cnt), VEC(K, pk_flags), VEC(K, pk_sig), VEC(K, vq_src);
  VEC(K, run_ap), VEC(K, run_fq), VEC(K, run_cnt), VEC(K, run_bdry), VEC(K, run_slot), VEC(K, run_nbr), VEC(K, run_blk), VEC(K, run_sig);
  VEC(K, send_count), VEC(K, recv_count), VEC(K, r21_rlen), VEC(K, r21_src), VEC(K, r21_dst), VEC(K, r22_slot), VEC(K, r22_ptr), VEC(K, r22_src);
  if (!K.vqx_h)
    pending.push_back("vqx_h,vqw_h=null");
  else if (K.vqx_h == p->vq_x && K.vqw_h == p->vq_w)
    pending.push_back("vqx_h,vqw_h=caller");
  else
    raw("vqx_h", K.vqx_h, (size_t)p->dim * K.vq_stride_h, 8), raw("vqw_h", K.vqw_h, (size_t)K.n_vq, 8);
  for (const Switches &sw : settings)
    {
      env("PDH_TERMS_MERGE", sw.merge);
      env("PDH_TERMS_SPLIT", sw.split);
      if (settings.size() > 1)
        put("  KernelPlan PDH_TERMS_MERGE=%s PDH_TERMS_SPLIT=%s\n", sw.merge ? sw.merge : "unset", sw.split ? sw.split : "unset");
      const KernelPlan P = plan_like_check(p, K);
      const RowsHost &R = P.rows;
      const TermsHost &T = P.terms;
      put("  kernel %s vq_n %d tensor_only %d\n", P.kernel == RowKernel::rows ? "rows" : (P.kernel == RowKernel::terms ? "terms" : "none"), P.vq_n,
          (int)P.tensor_only);
      put("  why_rows \"%s\"\n  why_terms \"%s\"\n", P.why_rows.c_str(), P.why_terms.c_str());
      NUM(R, planar_ok), NUM(R, fq_tensor_n), VEC(R, fast_j);
      if (P.why_rows.empty())
        { // the tables of pdh_rows.h are complete (a refusal leaves them where it stopped; nothing reads them then)
          NUM(R, multi), NUM(R, maxe), NUM(R, maxf), NUM(R, maxs);
          VEC(R, fr_ptr), VEC(R, fr_pbeg), VEC(R, fr_pcnt), VEC(R, fr_nbr), VEC(R, fr_axis), VEC(R, fr_blk), VEC(R, fr_flags), VEC(R, fr_coord);
          VEC(R, fr_sigma), VEC(R, fr_nsign);
          vec("rows.meta", R.meta);
        }
      NUM(T, maxruns), NUM(T, maxsf), NUM(T, maxsi), NUM(T, maxcell), NUM(T, lds_bytes); // (pdh_check_terms reports these on refusal too)
      if (P.kernel == RowKernel::terms)
        {
          NUM(T, split), NUM(T, task_pts), NUM(T, n_cells_in), NUM(T, n_cells_out), NUM(T, n_sf_in), NUM(T, n_sf_out);
          VEC(T, sf_pt), VEC(T, sf_info), VEC(T, sf_ivl), VEC(T, cell_ivl);
          vec("terms.meta", T.meta);
        }
    }
  env("PDH_TERMS_MERGE", nullptr);
  env("PDH_TERMS_SPLIT", nullptr);
  flush();
  return out;
}

static void show(const std::string &text) { std::fputs(text.c_str(), stdout); }

struct Mesh
{
  BackgroundGrid grid;
  std::unique_ptr<AgglomerationHandler> ah;
  FiniteElement fe;
  int n = 0;
  // block > 0: block agglomerates; block < 0: grown agglomerates of -block cells (seed)
  Mesh(int dim, int cells, int block, int basis, int degree, unsigned seed = 0, double distort = 0.0)
    : grid(BackgroundGrid::subdivided_hyper_cube(dim, cells, 0., 1.))
  {
    if (distort != 0.0)
      grid.distort(distort, seed);
    ah = std::make_unique<AgglomerationHandler>(grid);
    if (block > 0)
      define_block_agglomerates(*ah, block);
    else
      define_grown_agglomerates(*ah, -block, seed);
    fe.dim = dim, fe.degree = degree, fe.basis = basis;
    ah->initialize_fe_values(degree + 1, degree + 1);
    ah->distribute_agglomerated_dofs(fe);
    n = fe.n_dofs_per_cell();
  }
  SipVariant variant() const { return SipVariant::poisson_example(fe); }
  std::string name() const { return std::string(fe.basis ? "AggloDGP(" : "DGQ(") + std::to_string(fe.degree) + ")"; }
};

// inserts a copy of face f behind it that takes the points from `cut` on
static void split_face(FlatProblem &F, int f, int64_t cut)
{
  F.face_in.insert(F.face_in.begin() + f + 1, F.face_in[f]);
  F.face_out.insert(F.face_out.begin() + f + 1, F.face_out[f]);
  F.face_sigma.insert(F.face_sigma.begin() + f + 1, F.face_sigma[f]);
  F.fq_ptr.insert(F.fq_ptr.begin() + f + 1, cut);
  F.c.n_faces += 1;
  F.bind();
}

int main()
{
  const std::pair<int, int> dgq123_dgp123[] = {{0, 1}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}};
  // 1. 2-D, 8 x 8 cells in 2 x 2 blocks, with colind
  for (auto bd : {std::pair<int, int>{0, 1}, {0, 2}, {0, 3}, {1, 2}})
    for (int diag_first = 0; diag_first < 2; ++diag_first)
      {
        Mesh M(2, 8, 2, bd.first, bd.second);
        FlatProblem F;
        M.ah->flatten(M.variant(), F, diag_first != 0, true);
        show(fingerprint("1 2-D 8x8/2x2 " + M.name() + " diag_first " + std::to_string(diag_first), &F.c, 0, F.c.n_rows));
      }
  // 2. 3-D, 4^3 cells in 2^3 blocks: the whole problem and the middle third of the rows; 7. a second boundary face on polytope 0
  for (auto bd : dgq123_dgp123)
    {
      Mesh M(3, 4, 2, bd.first, bd.second);
      FlatProblem F;
      M.ah->flatten(M.variant(), F, true, true);
      const int nA = F.c.n_agg;
      show(fingerprint("2 3-D 4^3/2^3 " + M.name() + " all rows", &F.c, 0, F.c.n_rows));
      show(fingerprint("2 3-D 4^3/2^3 " + M.name() + " middle third", &F.c, (nA / 3) * M.n, (2 * nA / 3) * M.n));
      for (int f = 0; f < F.c.n_faces && bd == std::pair<int, int>{0, 3}; ++f)
        if (F.face_in[f] == 0 && F.face_out[f] < 0)
          {
            const int64_t g = (int64_t)(bd.second + 1) * (bd.second + 1), ng = (F.fq_ptr[f + 1] - F.fq_ptr[f]) / g;
            split_face(F, f, F.fq_ptr[f] + ng / 2 * g);
            show(fingerprint("7 3-D 4^3/2^3 " + M.name() + " two boundary faces on polytope 0", &F.c, 0, F.c.n_rows));
            break;
          }
    }
  // 3. 3-D, 8^3 cells in 4^3 blocks (merged sub-grids, boundary runs of more than 32 sub-faces), points and cartesian;
  // 4. 6^3 cells in grown agglomerates of 8 (staircase faces, MULTI, partial merges) under the merge / split switches;
  // 10. both once more on one host thread
  for (int pass = 0; pass < 2; ++pass)
    {
      std::vector<std::string> texts;
      for (int threads1 = 0; threads1 < 2; ++threads1)
        {
          env("PDH_HOST_THREADS", threads1 ? "1" : nullptr);
          std::string all;
          for (int basis = 0; basis < 2; ++basis)
            if (pass == 0)
              {
                Mesh M(3, 8, 4, basis, 3);
                FlatProblem F, C;
                M.ah->flatten(M.variant(), F, true, false);
                all += fingerprint("3 3-D 8^3/4^3 " + M.name() + " points", &F.c, 0, F.c.n_rows);
                M.ah->flatten_cartesian(M.variant(), C, true, false);
                all += fingerprint("3 3-D 8^3/4^3 " + M.name() + " cartesian", &C.c, 0, C.c.n_rows, PDH_EXCHANGE_NONE, &C.cart);
              }
            else
              for (unsigned seed : {1u, 2u})
                {
                  Mesh M(3, 6, -8, basis, 3, seed);
                  FlatProblem F;
                  M.ah->flatten(M.variant(), F, true, false);
                  std::vector<Switches> settings = {{"0", nullptr}, {"1", nullptr}, {"2", nullptr}};
                  if (basis)
                    for (const char *merge : {"0", "1", "2"})
                      for (const char *split : {"0", "1"})
                        settings.push_back({merge, split});
                  all += fingerprint("4 3-D 6^3 grown(8, seed " + std::to_string(seed) + ") " + M.name(), &F.c, 0, F.c.n_rows, PDH_EXCHANGE_NONE,
                                     nullptr, settings);
                }
          texts.push_back(all);
        }
      env("PDH_HOST_THREADS", nullptr);
      show(texts[0]);
      std::printf("== 10 case %d with PDH_HOST_THREADS=1: %s\n", pass == 0 ? 3 : 4, texts[0] == texts[1] ? "identical" : "DIFFERENT");
      if (texts[0] != texts[1])
        show(texts[1]);
    }
  // 5. distorted cells: both families refuse
  {
    Mesh M(3, 4, 2, 0, 3, 5u, 0.1);
    FlatProblem F;
    M.ah->flatten(M.variant(), F, true, false);
    show(fingerprint("5 3-D 4^3/2^3 distort(0.1, 5) DGQ(3)", &F.c, 0, F.c.n_rows));
  }
  // 6. more than 64 functions: tiled
  {
    Mesh M(3, 8, 4, 0, 4);
    FlatProblem F;
    M.ah->flatten(M.variant(), F, true, false);
    show(fingerprint("6 3-D 8^3/4^3 DGQ(4)", &F.c, 0, F.c.n_rows));
  }
  // 8. rank-local descriptions of case 2 cut in half, with and without the ghost-block exchange
  for (auto bd : {std::pair<int, int>{0, 3}, {1, 2}})
      {
        const int diag_first = bd.first ? 0 : 1;
        Mesh M(3, 4, 2, bd.first, bd.second);
        const int nA = (int)M.ah->n_dofs() / M.n, cut = (nA / 2) * M.n;
        std::vector<int> splits = {0, cut, nA * M.n};
        for (int half = 0; half < 2; ++half)
          {
            FlatProblem L;
            const int rb = half ? cut : 0, re = half ? nA * M.n : cut;
            M.ah->flatten_local(M.variant(), L, rb, re, diag_first != 0, true, nullptr, &splits);
            for (int mode : {PDH_EXCHANGE_NONE, PDH_EXCHANGE_GHOST})
              show(fingerprint("8 3-D 4^3/2^3 " + M.name() + " local half " + std::to_string(half) + " diag_first " + std::to_string(diag_first) +
                                 (mode == PDH_EXCHANGE_GHOST ? " ghost" : " none"),
                               &L.c, rb, re, mode));
          }
      }
  // 9. malformed descriptions that fail at different stages
  {
    Mesh M(3, 4, 2, 0, 2);
    FlatProblem F;
    M.ah->flatten(M.variant(), F, true, true);
    show(fingerprint("9 NULL problem", nullptr, 0, 0));
    pdh_problem c = F.c;
    c.bbox = nullptr;
    show(fingerprint("9 bbox NULL", &c, 0, c.n_rows));
    show(fingerprint("9 row range not aligned", &F.c, 1, F.c.n_rows));
    FlatProblem G = F;
    G.bind();
    G.face_out[3] = G.c.n_agg;
    show(fingerprint("9 face_out out of range", &G.c, 0, G.c.n_rows));
    G = F;
    G.bind();
    for (size_t i = 0; i < G.rowptr.size(); ++i)
      G.rowptr[i] += (int64_t)i;
    show(fingerprint("9 wrong row length", &G.c, 0, G.c.n_rows));
    G = F;
    G.bind();
    G.colind[5] += 1;
    show(fingerprint("9 wrong colind", &G.c, 0, G.c.n_rows));
    G = F;
    for (int f = 0; f < G.c.n_faces; ++f)
      if (G.face_out[f] >= 0)
        {
          split_face(G, f, G.fq_ptr[f + 1]); // (an empty second face for the same pair)
          break;
        }
    show(fingerprint("9 two faces for one pair", &G.c, 0, G.c.n_rows));
  }
  return 0;
}
