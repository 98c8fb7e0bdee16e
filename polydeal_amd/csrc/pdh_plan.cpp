// pdh_plan.cpp — the host-only planner of a problem (pdh_plan.h): the choice of the row kernel (plan_kernels), the pdh_check_* entry
// points that run what pdh_set_problem does before anything goes to the device on machines without a GPU, and the host arithmetic of
// the Chebyshev set-up, after validation and repacking (pack_problem, in stages), the face analysis both kernel families need, the
// tables of pdh_rows.h and those of the term kernels.  Plain C++: no HIP header, no HIP call; what must agree with the kernels comes from
// the layout headers they include too (pdh_dev.h, pdh_rows_tables.h, pdh_terms_tables.h).
#include "pdh_plan_internal.h"

#include "pdh_basis.h"
#include "pdh_combos.h"
#include "pdh_rows_tables.h"
#include "pdh_terms_tables.h"

#include <chrono>
#include <cstdio>

static thread_local std::string g_err_noctx;
std::string &pdh_noctx_error() { return g_err_noctx; }

// translation-unit group holding the kernels of a combo, or -1 if that combo is not instantiated
int combo_group(int dim, int n1d, int nt, int lb)
{
#define PDH_X(G, D, N, T, L)                                                                       \
  if (dim == D && n1d == N && nt == T && lb == L)                                                  \
    return G;
  PDH_COMBOS(PDH_X)
#undef PDH_X
  return -1;
}


// Host-only part of set_problem: validation + repacking, as a sequence of stages over Packed.
namespace
{
// what every stage needs of the call
struct PackCtx
{
  const pdh_problem *p;
  int32_t row_begin, row_end;
  int n;
  bool ghost;
  int64_t rp_shift; // rowptr covers all rows (global description) or the owned rows only (rank-local description)
  // number that orders the blocks of a row: the global dof number, or the caller's column numbering (Epetra local ids)
  int colnum(int a) const { return p->col_offset ? p->col_offset[a] : p->dof_offset[a]; }
  bool owned(int a) const { return p->dof_offset[a] >= row_begin && p->dof_offset[a] < row_end; }
};

// The refusals of a description that need no repacking, in the order callers rely on; sets the sizes of K (n, n1d, NT, LB, tiled).
int validate_description(std::string &err, const pdh_problem *p, int32_t row_begin, int32_t row_end, const pdh_cartesian_points *cart, Packed &K)
{
  if (!p)
    return fail(err, PDH_EINVAL, "problem is NULL");
  K.cart = cart;
  if (p->dim != 2 && p->dim != 3)
    return fail(err, PDH_EINVAL, "dim must be 2 or 3");
  if (p->basis != PDH_BASIS_DGQ && p->basis != PDH_BASIS_AGGLODGP)
    return fail(err, PDH_EINVAL, "unknown basis");
  if (p->degree < 0 || p->degree + 1 > PDH_MAX_N1D)
    return fail(err, PDH_EUNSUPPORTED, "degree must be in [0,7]");
  if (p->n_agg <= 0 || p->n_faces < 0)
    return fail(err, PDH_EINVAL, "n_agg must be positive and n_faces non-negative");
  if (!p->bbox || !p->dof_offset || !p->vq_ptr || (!cart && (!p->vq_x || !p->vq_w)) || !p->rowptr)
    return fail(err, PDH_EINVAL, "a required array is NULL");
  if (p->n_faces > 0 && (!p->face_in || !p->face_out || !p->fq_ptr || (!cart && (!p->fq_x || !p->fq_n || !p->fq_w)) || !p->face_sigma))
    return fail(err, PDH_EINVAL, "a required face array is NULL");
  if (cart)
    { // compact description of Cartesian cells: the groups of points must be whole rules on valid cells
      if (p->dim != 3 || cart->nq < 1 || cart->nq > PDH_MAX_N1D || cart->nqf < 1 || cart->nqf > PDH_MAX_N1D)
        return fail(err, PDH_EINVAL, "cartesian description: dim must be 3 and 1 <= nq, nqf <= 8");
      if (cart->n_cells <= 0 || !cart->cell_box || !cart->vq_cell || (p->n_faces > 0 && (!cart->fq_cell || !cart->fq_face)))
        return fail(err, PDH_EINVAL, "cartesian description: a required array is NULL");
      const int64_t m3 = (int64_t)cart->nq * cart->nq * cart->nq, m2 = (int64_t)cart->nqf * cart->nqf;
      for (int a = 0; a < p->n_agg; ++a)
        if ((p->vq_ptr[a + 1] - p->vq_ptr[a]) % m3)
          return fail(err, PDH_EINVAL, "cartesian description: the volume points of a polytope are not whole groups of nq^3");
      for (int f = 0; f < p->n_faces; ++f)
        if ((p->fq_ptr[f + 1] - p->fq_ptr[f]) % m2)
          return fail(err, PDH_EINVAL, "cartesian description: the points of a face are not whole groups of nqf^2");
      for (int64_t g = 0; g < p->vq_ptr[p->n_agg] / m3; ++g)
        if (cart->vq_cell[g] < 0 || cart->vq_cell[g] >= cart->n_cells)
          return fail(err, PDH_EINVAL, "cartesian description: vq_cell out of range");
      for (int64_t g = 0; g < (p->n_faces ? p->fq_ptr[p->n_faces] / m2 : 0); ++g)
        if (cart->fq_cell[g] < 0 || cart->fq_cell[g] >= cart->n_cells || cart->fq_face[g] < 0 || cart->fq_face[g] > 5)
          return fail(err, PDH_EINVAL, "cartesian description: fq_cell / fq_face out of range");
      for (int64_t c = 0; c < cart->n_cells; ++c)
        for (int d = 0; d < 3; ++d)
          if (!std::isfinite(cart->cell_box[c * 6 + d]) || !(cart->cell_box[c * 6 + 3 + d] > cart->cell_box[c * 6 + d]))
            return fail(err, PDH_EINVAL, "cartesian description: degenerate cell box");
    }
  const int dim = p->dim, n = pdh::n_dofs_per_cell(dim, p->degree, p->basis);
  // more than 64 dofs per polytope: blocks are computed in 64 x 64 tiles (pdh_tiled.h; 3-D, degree 4 .. 7)
  K.tiled = n > 64;
  if (K.tiled && !pdh::tiled_has_kind(p->dim, p->degree + 1, n))
    return fail(err, PDH_EUNSUPPORTED, "more than 64 dofs per polytope are supported in 3-D for degree 4 .. 7 only");
  if (!p->local && (int64_t)n * p->n_agg != p->n_rows)
    return fail(err, PDH_EINVAL, "n_rows != dofs_per_cell * n_agg (global description)");
  if (p->n_rows <= 0 || p->n_rows % n)
    return fail(err, PDH_EINVAL, "n_rows must be a positive multiple of dofs_per_cell");
  if (row_begin < 0 || row_end > p->n_rows || row_begin > row_end || row_begin % n || row_end % n)
    return fail(err, PDH_EINVAL, "owned row range must be aligned to whole polytopes");
  if (p->col_offset && p->diag_first)
    return fail(err, PDH_EINVAL, "col_offset (Epetra column order) requires diag_first = 0");
  if (p->rowptr[0] != 0)
    return fail(err, PDH_EINVAL, "rowptr[0] must be 0");
  K.n = n, K.n1d = p->degree + 1;
  const int T = (n + 3) / 4;
  K.NT = (T + 3) / 4;
  K.LB = T - 4 * (K.NT - 1);
  if (K.tiled)
    K.NT = K.LB = 4; // every tile is the full 64 x 64 product
  else if (combo_group(dim, K.n1d, K.NT, K.LB) < 0)
    return fail(err, PDH_EUNSUPPORTED, "no kernel instantiated for this (dim, basis, degree)");

  const int nA = p->n_agg, nF = p->n_faces;
  if (p->vq_ptr[0] != 0 || (nF > 0 && p->fq_ptr[0] != 0))
    return fail(err, PDH_EINVAL, "vq_ptr[0] and fq_ptr[0] must be 0");
  for (int a = 0; a < nA; ++a)
    {
      const int off = p->dof_offset[a];
      if (off < 0 || off % n || off + n > p->n_rows)
        return fail(err, PDH_EINVAL, "dof_offset must be a multiple of dofs_per_cell inside [0,n_rows)");
      if (p->col_offset && (p->col_offset[a] < 0 || p->col_offset[a] % n))
        return fail(err, PDH_EINVAL, "col_offset must be a non-negative multiple of dofs_per_cell");
      for (int c = 0; c < 2 * dim; ++c)
        if (!std::isfinite(p->bbox[(size_t)a * 2 * dim + c]))
          return fail(err, PDH_EINVAL, "bounding box is not finite");
      if (p->vq_ptr[a + 1] < p->vq_ptr[a])
        return fail(err, PDH_EINVAL, "vq_ptr must be non-decreasing");
      // (the weights themselves are checked below, by all host threads)
      for (int c = 0; c < dim; ++c)
        if (!(p->bbox[(size_t)a * 2 * dim + dim + c] > p->bbox[(size_t)a * 2 * dim + c]))
          return fail(err, PDH_EINVAL, "degenerate bounding box");
    }
  for (int f = 0; f < nF; ++f)
    {
      const int in = p->face_in[f], out = p->face_out[f];
      if (in < 0 || in >= nA || out < -1 || out >= nA || out == in)
        return fail(err, PDH_EINVAL, "face_in/face_out out of range");
      if (!std::isfinite(p->face_sigma[f]))
        return fail(err, PDH_EINVAL, "face_sigma is not finite");
      if (p->fq_ptr[f + 1] < p->fq_ptr[f])
        return fail(err, PDH_EINVAL, "fq_ptr must be non-decreasing");
    }
  if (cart) // (generated weights are products of positive box sides and Gauss weights)
    return PDH_OK;
  // JxW must be non-negative (and not NaN): chunks of 64k points per task
  const int64_t nq_tot = p->vq_ptr[nA], n_tot = nq_tot + (nF ? p->fq_ptr[nF] : 0);
  const bool ok = host_parallel_all((size_t)(n_tot / 65536 + 1), [&](size_t k) {
    bool bad = false;
    for (int64_t i = (int64_t)k * 65536, e = std::min<int64_t>(i + 65536, n_tot); i < e; ++i)
      if (i < nq_tot)
        bad |= !(p->vq_w[i] >= 0.0);
      else
        bad |= !(p->fq_w[i - nq_tot] >= 0.0) || (p->fq_w_out && !(p->fq_w_out[i - nq_tot] >= 0.0));
    return !bad;
  });
  return ok ? PDH_OK : fail(err, PDH_EINVAL, "quadrature weights (JxW) must be non-negative");
}

void fill_basis_tables(const pdh_problem *p, Packed &K)
{
  const pdh::Basis1D b1 = (p->basis == PDH_BASIS_DGQ) ? pdh::lagrange_basis(p->degree) : pdh::legendre_basis(p->degree);
  std::memset(&K.tab, 0, sizeof(K.tab));
  for (int k = 0; k < K.n1d; ++k)
    for (int m = 0; m < K.n1d; ++m)
      K.tab.coef[k][m] = (double)b1.coef[k][m];
  const auto mi = pdh::multi_indices(p->dim, p->degree, p->basis);
  K.midx.assign(K.tiled ? (size_t)(K.n + 63) / 64 * 64 : (size_t)16 * K.NT, (int32_t)0xffffffffu);
  for (int i = 0; i < K.n; ++i)
    K.midx[i] = (int32_t)mi[i];
}

// faces per polytope (CSR by counting), in face order
struct FaceAdjacency
{
  const pdh_problem *p;
  std::vector<int64_t> fptr;
  std::vector<int32_t> flist;
  explicit FaceAdjacency(const pdh_problem *p_)
    : p(p_)
    , fptr(p_->n_agg + 1, 0)
  {
    auto for_sides = [&](auto &&fn) { // (every face under side 0, then side 1)
      for (int f = 0; f < p->n_faces; ++f)
        for (int a : {p->face_in[f], p->face_out[f]})
          if (a >= 0)
            fn(a, f);
    };
    for_sides([&](int a, int) { ++fptr[a + 1]; });
    for (int a = 0; a < p->n_agg; ++a)
      fptr[a + 1] += fptr[a];
    flist.resize(fptr[p->n_agg]);
    std::vector<int64_t> cur(fptr.begin(), fptr.end() - 1);
    for_sides([&](int a, int f) { flist[cur[a]++] = f; });
  }
  int other_side(int a, int f) const { return p->face_in[f] == a ? p->face_out[f] : p->face_in[f]; }
};

// coupled blocks of the rows of a polytope, ascending by column number (reference :954-975)
struct RowBlocks
{
  std::vector<std::pair<int32_t, int32_t>> b; // (column number, polytope)
  void assign(const PackCtx &C, const FaceAdjacency &adj, int a)
  {
    b.clear();
    b.emplace_back(C.colnum(a), a);
    for (int64_t t = adj.fptr[a]; t < adj.fptr[a + 1]; ++t)
      {
        const int other = adj.other_side(a, adj.flist[t]);
        if (other >= 0)
          b.emplace_back(C.colnum(other), other);
      }
    std::sort(b.begin(), b.end());
  }
  int rank_of(int polytope) const // -1: no block (the boundary)
  {
    for (size_t u = 0; u < b.size(); ++u)
      if (b[u].second == polytope)
        return (int)u;
    return -1;
  }
  // first value of block `rank` (column number col) in a row whose own block has column number own_col: the diagonal-first layout
  // moves the diagonal entry to the front, which shifts the blocks left of it by one
  static int pos_of(int rank, int col, int own_col, bool diag_first, int n) { return rank * n + (diag_first && col < own_col ? 1 : 0); }
};

// ---- ghost-block exchange variant (pdh_set_exchange_mode): which faces are cut by the partition ------------------
// A face whose sides live on different ranks is assembled by the rank that owns side 0 (the caller lists every face from
// its owner side: the reference's `id() < neighbor->id()` rule, include/poly_utils.h:2089, 2134-2190): that rank adds
// M11, M12 to its own rows and ships M21 (one block per face) and M22 (summed per remote polytope) to the other rank.
struct Cut { int peer, dof_in, dof_out, f; };
// blocks (units of n^2 doubles) of one direction of the exchange, peer by peer: the M21 blocks of the cut faces ascending by
// (side-0 dof, side-1 dof), then one M22 block per distinct side-1 polytope, ascending by its dof
struct PeerBlocks
{
  std::vector<int64_t> block_of_face; // M21 of a face, -1: not cut
  struct M22 { int peer, polytope; int64_t block; };
  std::vector<M22> m22;
  int64_t n_blocks = 0;
};
PeerBlocks group_cut_faces_by_peer(const pdh_problem *p, std::vector<Cut> &cuts, size_t n_faces, int n, std::vector<int64_t> &count)
{
  std::sort(cuts.begin(), cuts.end(), [](const Cut &x, const Cut &y) {
    return x.peer != y.peer ? x.peer < y.peer : (x.dof_in != y.dof_in ? x.dof_in < y.dof_in : x.dof_out < y.dof_out);
  });
  PeerBlocks B;
  B.block_of_face.assign(n_faces, -1);
  int64_t &blk = B.n_blocks;
  for (size_t i = 0; i < cuts.size();)
    {
      const int peer = cuts[i].peer;
      const int64_t blk0 = blk;
      std::vector<std::pair<int, int>> outs; // (dof, polytope)
      for (; i < cuts.size() && cuts[i].peer == peer; ++i)
        {
          B.block_of_face[cuts[i].f] = blk++;
          outs.emplace_back(cuts[i].dof_out, p->face_out[cuts[i].f]);
        }
      std::sort(outs.begin(), outs.end());
      outs.erase(std::unique(outs.begin(), outs.end()), outs.end());
      for (const auto &o : outs)
        B.m22.push_back({peer, o.second, blk++});
      count[peer] = (blk - blk0) * (int64_t)n * n;
    }
  return B;
}

// send / recv: faces owned here with a remote side 1 / owned remotely with side 1 here
int plan_exchange(std::string &err, const PackCtx &C, Packed &K, PeerBlocks &send, PeerBlocks &recv)
{
  const pdh_problem *p = C.p;
  if (C.ghost && K.tiled)
    return fail(err, PDH_EUNSUPPORTED, "more than 64 dofs per polytope run owner-computes-rows only (no ghost-block exchange)");
  int my_rank = -1, n_ranks = 1;
  std::vector<Cut> cut_send, cut_recv;
  if (C.ghost)
    {
      if (!p->agg_rank)
        return fail(err, PDH_EINVAL, "the ghost-block exchange needs agg_rank (owning rank of every polytope)");
      for (int a = 0; a < p->n_agg; ++a)
        {
          if (p->agg_rank[a] < 0)
            return fail(err, PDH_EINVAL, "agg_rank must be non-negative");
          n_ranks = std::max(n_ranks, p->agg_rank[a] + 1);
          if (C.owned(a))
            {
              if (my_rank >= 0 && p->agg_rank[a] != my_rank)
                return fail(err, PDH_EINVAL, "owned polytopes carry different ranks in agg_rank");
              my_rank = p->agg_rank[a];
            }
        }
      for (int a = 0; a < p->n_agg; ++a)
        if (!C.owned(a) && p->agg_rank[a] == my_rank)
          return fail(err, PDH_EINVAL, "a polytope outside the owned row range carries the owner's rank in agg_rank");
      for (int f = 0; f < p->n_faces; ++f)
        {
          const int in = p->face_in[f], out = p->face_out[f];
          if (out < 0)
            continue;
          if (C.owned(in) && !C.owned(out))
            cut_send.push_back({p->agg_rank[out], p->dof_offset[in], p->dof_offset[out], f});
          else if (!C.owned(in) && C.owned(out))
            cut_recv.push_back({p->agg_rank[in], p->dof_offset[in], p->dof_offset[out], f});
        }
    }
  K.send_count.assign(n_ranks, 0);
  K.recv_count.assign(n_ranks, 0);
  const size_t nF = C.ghost ? (size_t)p->n_faces : 0;
  send = group_cut_faces_by_peer(p, cut_send, nF, C.n, K.send_count);
  recv = group_cut_faces_by_peer(p, cut_recv, nF, C.n, K.recv_count);
  K.n_send = send.n_blocks * (int64_t)C.n * C.n;
  K.n_recv = recv.n_blocks * (int64_t)C.n * C.n;
  return PDH_OK;
}

// The rows of polytope a against its blocks: equal length (1 + #neighbours) n, and - given colind - EVERY row against the positions
// the kernels write to (each row carries its own diagonal-first shift); O(nnz) host work, once per problem
int check_rows_of_polytope(std::string &err, const PackCtx &C, int a, const RowBlocks &blocks, int64_t &r0, int64_t &rl)
{
  const pdh_problem *p = C.p;
  const int n = C.n, off = p->dof_offset[a];
  const int64_t *rp = p->rowptr + (off - C.rp_shift);
  r0 = rp[0];
  rl = rp[1] - r0;
  if (rl != (int64_t)blocks.b.size() * n)
    return fail(err, PDH_EINVAL, "row length does not match (1 + #neighbours) * dofs_per_cell for polytope " + std::to_string(a));
  for (int i = 1; i < n; ++i)
    if (rp[i + 1] - rp[i] != rl)
      return fail(err, PDH_EINVAL, "rows of one polytope must have equal length");
  if (!p->colind)
    return PDH_OK;
  for (int i = 0; i < n; ++i)
    {
      const int32_t *ci = p->colind + r0 + (int64_t)i * rl;
      const int dcol = C.colnum(a) + i;
      for (size_t t = 0; t < blocks.b.size(); ++t)
        for (int j = 0; j < n; ++j)
          {
            const int col = blocks.b[t].first + j;
            int64_t pos = (int64_t)t * n + j;
            if (p->diag_first)
              pos = (col == dcol) ? 0 : (col < dcol ? pos + 1 : pos);
            if (ci[pos] != col)
              return fail(err, PDH_EINVAL, "colind does not have the DG block layout expected for polytope " + std::to_string(a) + " (row " +
                                             std::to_string(off + i) + ")");
          }
    }
  return PDH_OK;
}

// One entry of the tables of the device-side face repack (k_pack_faces) for the points of face f seen from polytope a, appended
// to the slot being filled: weights and signs as the kernels want them -
//   boundary: w_self = 2 JxW, sigma / 2 (Nitsche boundary = interior self-block with these exact scalings), w_cross = 0;
//   interior: w_self = JxW of the own side (M11 uses JxW_0, M22 JxW_1: poly_utils.h:1898, 1922), w_cross = JxW_1
//   (M12, M21: poly_utils.h:1906, 1914), normal = outward normal of the owning polytope
void append_face_run(const pdh_problem *p, Packed &K, int a, int f)
{
  const bool side0 = p->face_in[f] == a;
  const int other = side0 ? p->face_out[f] : p->face_in[f];
  K.pk_at.push_back(K.n_ap);
  K.pk_fq.push_back(p->fq_ptr[f]);
  K.pk_cnt.push_back((int32_t)(p->fq_ptr[f + 1] - p->fq_ptr[f]));
  K.pk_flags.push_back((side0 ? 1 : 0) | (other < 0 ? 2 : 0));
  K.pk_sig.push_back(other < 0 ? 0.5 * p->face_sigma[f] : p->face_sigma[f]);
  K.n_ap += K.pk_cnt.back();
}

// The owned polytopes in polytope order, one slot each: rows, blocks, volume points, own-side face runs and coupling items.
// r21_face: the cut faces whose M21 arrives through the exchange, in the order of r21_dst.
int pack_owned_slots(std::string &err, const PackCtx &C, const FaceAdjacency &adj, Packed &K, std::vector<int32_t> &slot_of,
                     std::vector<int32_t> &r21_face)
{
  const pdh_problem *p = C.p;
  const int n = C.n;
  const int64_t val_base = p->rowptr[C.row_begin - C.rp_shift];
  K.vq_ptr.push_back(0);
  K.ap_ptr.push_back(0);
  RowBlocks blocks;
  for (int a = 0; a < p->n_agg; ++a)
    {
      if (!C.owned(a))
        continue;
      const int slot = (int)K.own_agg.size(), ocol = C.colnum(a);
      slot_of[a] = slot;
      K.own_agg.push_back(a);
      K.own_row.push_back(p->dof_offset[a] - C.row_begin);
      blocks.assign(C, adj, a);
      for (size_t t = 1; t < blocks.b.size(); ++t)
        if (blocks.b[t].first == blocks.b[t - 1].first)
          return fail(err, PDH_EINVAL, "two faces couple the same pair of polytopes (faces must be merged per neighbour)");
      int64_t r0, rl;
      PDH_TRY(check_rows_of_polytope(err, C, a, blocks, r0, rl));
      K.row_base.push_back(r0 - val_base);
      K.row_len.push_back((int32_t)rl);
      for (const auto &b : blocks.b)
        K.blk_dof.push_back(p->dof_offset[b.second]);
      K.blk_ptr.push_back((int64_t)K.blk_dof.size());
      K.max_row_len = std::max(K.max_row_len, (int)rl);
      K.diag_L.push_back(blocks.rank_of(a) * n);
      K.vq_src.push_back(p->vq_ptr[a]);
      K.n_vq += p->vq_ptr[a + 1] - p->vq_ptr[a];
      K.vq_ptr.push_back(K.n_vq);
      // own-side face points + coupling items
      for (int64_t t = adj.fptr[a]; t < adj.fptr[a + 1]; ++t)
        {
          const int f = adj.flist[t], other = adj.other_side(a, f);
          const int brank = blocks.rank_of(other);
          const int pos = other >= 0 ? RowBlocks::pos_of(brank, C.colnum(other), ocol, p->diag_first, n) : 0;
          const bool other_owned = other >= 0 && C.owned(other);
          if (C.ghost && other >= 0 && !other_owned && p->face_in[f] != a)
            { // owned by the other rank: its M21 and M22 arrive through the exchange
              r21_face.push_back(f);
              K.r21_dst.push_back(K.row_base[slot] + pos);
              K.r21_rlen.push_back((int32_t)rl);
              continue;
            }
          const int64_t at = K.n_ap; // first packed point of the run
          append_face_run(p, K, a, f);
          K.run_ap.push_back(at);
          K.run_fq.push_back(K.pk_fq.back());
          K.run_cnt.push_back(K.pk_cnt.back());
          K.run_bdry.push_back(other < 0 ? 1 : 0);
          K.run_slot.push_back(slot);
          K.run_nbr.push_back(other);
          K.run_blk.push_back(brank);
          K.run_sig.push_back(K.pk_sig.back());
          // one item per interior face: the owned side with the lower polytope id computes A[P,Q]
          // and also writes A[Q,P] = A[P,Q]^T when Q's rows are owned here too
          if (other >= 0 && (!other_owned || a < other))
            {
              K.it_own.push_back(slot);
              K.it_nbr.push_back(other);
              K.it_pbeg.push_back(at);
              K.it_pcnt.push_back(K.pk_cnt.back());
              K.it_pos.push_back(pos);
              // polytope id for now (resolve_item_targets); ghost mode: -2 - f marks "M21 of face f goes to the send region"
              K.it_nbr_slot.push_back(other_owned ? other : (C.ghost ? -2 - f : -1));
              K.it_pos_t.push_back(0);
            }
        }
      K.ap_ptr.push_back(K.n_ap);
    }
  if ((int64_t)K.own_agg.size() * n != (int64_t)(C.row_end - C.row_begin))
    return fail(err, PDH_EINVAL, "dof_offset values do not tile the owned row range");
  K.n_owned = (int)K.own_agg.size();
  return PDH_OK;
}

// pseudo slots: the M22 sums for remote polytopes (side 1 of cut faces owned here), computed by the diagonal-block kernel
// from the points of those faces seen from side 1 and written as plain n x n blocks into the send region
void append_pseudo_slots(const PackCtx &C, const FaceAdjacency &adj, const PeerBlocks &send, Packed &K)
{
  for (const PeerBlocks::M22 &m : send.m22)
    {
      const int q = m.polytope;
      K.own_agg.push_back(q);
      K.own_row.push_back(0);
      K.row_base.push_back(K.n_values + m.block * (int64_t)C.n * C.n);
      K.row_len.push_back(C.n);
      K.diag_L.push_back(0);
      K.vq_ptr.push_back(K.n_vq);
      for (int64_t t = adj.fptr[q]; t < adj.fptr[q + 1]; ++t)
        {
          const int f = adj.flist[t];
          if (C.p->face_out[f] == q && C.owned(C.p->face_in[f]))
            append_face_run(C.p, K, q, f);
        }
      K.ap_ptr.push_back(K.n_ap);
    }
}

// resolve, for every coupling item, the neighbour's owned slot and the position of P's block inside Q's rows
void resolve_item_targets(const PackCtx &C, const FaceAdjacency &adj, const PeerBlocks &send, const std::vector<int32_t> &slot_of, Packed &K)
{
  RowBlocks blocks;
  for (size_t it = 0; it < K.it_own.size(); ++it)
    {
      const int q = K.it_nbr_slot[it];
      if (q == -1)
        continue;
      if (q <= -2)
        { // ghost mode: plain n x n block of the send region, addressed like a row range through a pseudo entry
          K.it_nbr_slot[it] = (int32_t)K.row_base.size();
          K.row_base.push_back(K.n_values + send.block_of_face[-2 - q] * (int64_t)C.n * C.n);
          K.row_len.push_back(C.n);
          continue;
        }
      const int pa = K.own_agg[K.it_own[it]];
      blocks.assign(C, adj, q);
      K.it_pos_t[it] = RowBlocks::pos_of(blocks.rank_of(pa), C.colnum(pa), C.colnum(q), C.p->diag_first, C.n);
      K.it_nbr_slot[it] = slot_of[q];
    }
}

// receive side of the exchange: where the incoming blocks go
void place_received_blocks(const PackCtx &C, PeerBlocks &recv, const std::vector<int32_t> &slot_of, const std::vector<int32_t> &r21_face,
                           Packed &K)
{
  const int64_t nn = (int64_t)C.n * C.n;
  for (int32_t f : r21_face)
    K.r21_src.push_back(recv.block_of_face[f] * nn);
  // M22: grouped by destination polytope so that one wave adds all contributions of a polytope, in a fixed order
  std::sort(recv.m22.begin(), recv.m22.end(), [](const PeerBlocks::M22 &x, const PeerBlocks::M22 &y) {
    return x.polytope != y.polytope ? x.polytope < y.polytope : x.peer < y.peer;
  });
  for (size_t k = 0; k < recv.m22.size(); ++k)
    {
      if (k == 0 || recv.m22[k - 1].polytope != recv.m22[k].polytope)
        {
          K.r22_ptr.push_back((int64_t)K.r22_src.size());
          K.r22_slot.push_back(slot_of[recv.m22[k].polytope]);
        }
      K.r22_src.push_back(recv.m22[k].block * nn);
    }
  K.r22_ptr.push_back((int64_t)K.r22_src.size());
}

// volume points of the owned slots: the caller's arrays where the slots are its polytopes in its order, else a copy in SoA with
// the final strides - disjoint ranges, all host threads
void bind_volume_points(const pdh_problem *p, Packed &K)
{
  const int64_t nq_tot = p->vq_ptr[p->n_agg], nvq = K.n_vq;
  bool vq_identity = nvq == nq_tot;
  for (int sl = 0; sl < K.n_owned && vq_identity; ++sl)
    vq_identity = K.vq_ptr[sl] == p->vq_ptr[K.own_agg[sl]];
  if (K.cart)
    K.vqx_h = K.vqw_h = nullptr, K.vq_stride_h = nvq; // (generated on the device, slot by slot)
  else if (vq_identity)
    K.vqx_h = p->vq_x, K.vqw_h = p->vq_w, K.vq_stride_h = nq_tot;
  else
    {
      K.vq_w.resize((size_t)nvq);
      K.vq_x.resize((size_t)p->dim * nvq);
      K.vqx_h = K.vq_x.data(), K.vqw_h = K.vq_w.data(), K.vq_stride_h = nvq;
      host_parallel_for((size_t)K.n_owned, [&](size_t sl) {
        const int a = K.own_agg[sl];
        int64_t vq = K.vq_ptr[sl];
        for (int64_t q = p->vq_ptr[a]; q < p->vq_ptr[a + 1]; ++q, ++vq)
          {
            K.vq_w[vq] = p->vq_w[q];
            for (int c = 0; c < p->dim; ++c)
              K.vq_x[c * nvq + vq] = p->vq_x[c * nq_tot + q];
          }
      });
    }
}
} // namespace

int pack_problem(std::string &err, const pdh_problem *p, int32_t row_begin, int32_t row_end, Packed &K, int exchange_mode,
                 const pdh_cartesian_points *cart)
{
  PDH_TRY(validate_description(err, p, row_begin, row_end, cart, K));
  fill_basis_tables(p, K);
  const PackCtx C{p, row_begin, row_end, K.n, exchange_mode == PDH_EXCHANGE_GHOST, p->local ? (int64_t)row_begin : 0};
  K.ghost = C.ghost;
  K.src = p;
  K.nqf_src = p->n_faces ? p->fq_ptr[p->n_faces] : 0;
  K.n_values = p->rowptr[row_end - C.rp_shift] - p->rowptr[row_begin - C.rp_shift];
  const FaceAdjacency adj(p);
  PeerBlocks send, recv;
  PDH_TRY(plan_exchange(err, C, K, send, recv));
  std::vector<int32_t> slot_of(p->n_agg, -1), r21_face;
  PDH_TRY(pack_owned_slots(err, C, adj, K, slot_of, r21_face));
  append_pseudo_slots(C, adj, send, K);
  resolve_item_targets(C, adj, send, slot_of, K);
  if (C.ghost)
    place_received_blocks(C, recv, slot_of, r21_face, K);
  bind_volume_points(p, K);
  return PDH_OK;
}

// Are the volume points of every owned polytope tensor-product rules of n^dim points on axis-aligned boxes (pdh_problem::
// vq_tensor_n)?  Checked on the packed points to a few ulp; dim = 3.
// Relative accuracy to expect of JxW (and of unit normals) that a caller computed from vertex coordinates of size |x| on
// cells of size h: eps |x| / h per factor (differences of rounded coordinates), taken from the polytope's box; between
// 1e-13 and 1e-12 (beyond that a deviation is treated as structure, not rounding).
double geometry_rounding(const pdh_problem *p, int a)
{
  double t = 1e-13;
  for (int d = 0; d < p->dim; ++d)
    {
      const double lo_d = p->bbox[(size_t)a * 2 * p->dim + d], hi_d = p->bbox[(size_t)a * 2 * p->dim + p->dim + d];
      t = std::max(t, 64.0 * 2.2e-16 * std::max(std::fabs(lo_d), std::fabs(hi_d)) / (hi_d - lo_d));
    }
  return std::min(t, 1e-12);
}

static bool volume_rules_are_tensor(const pdh_problem *p, const Packed &K, int n)
{
  if (n <= 0 || n > 8 || p->dim != 3)
    return false;
  const int64_t m = (int64_t)n * n * n, nvq = K.vq_stride_h;
  const double *vq_x = K.vqx_h, *vq_w = K.vqw_h;
  return host_parallel_all((size_t)K.n_owned, [&](size_t sl) {
    const int64_t b0 = K.vq_ptr[sl], e0 = K.vq_ptr[sl + 1];
    if ((e0 - b0) % m)
      return false;
    const int a = K.own_agg[sl];
    const double wtol = geometry_rounding(p, a);
    for (int64_t b = b0; b < e0; b += m)
      {
        const double w000 = vq_w[b];
        if (!(w000 > 0.0))
          return false;
        for (int k = 0; k < n; ++k)
          for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i)
              {
                const int64_t q = b + i + (int64_t)n * (j + (int64_t)n * k);
                const int idx[3] = {i, j, k};
                const int64_t step[3] = {1, n, (int64_t)n * n};
                double wf = w000;
                for (int d = 0; d < 3; ++d)
                  {
                    const double X = vq_x[d * nvq + b + idx[d] * step[d]];
                    const double h = box_side(p, a, d);
                    if (std::fabs(vq_x[d * nvq + q] - X) > 3e-15 * (std::fabs(X) + h))
                      return false;
                    wf *= vq_w[b + idx[d] * step[d]] / w000;
                  }
                if (std::fabs(vq_w[q] - wf) > wtol * wf)
                  return false;
              }
      }
    return true;
  });
}

// Sub-face rules: groups of n^2 points of a run, tensor in the two tangential axes (ti < tj); returns for every run whether
// tj runs fastest (flag) - or false if some group is not a tensor rule.  dim = 3; axis[r] = normal axis of the run's plane(s)
// is not needed: the tangential axes are found per group from the first point's normal.
static bool face_rules_are_tensor(const pdh_problem *p, const Packed &K, int n, std::vector<signed char> &fast_j)
{
  if (n <= 0 || n > 8 || p->dim != 3)
    return false;
  const int m = n * n;
  const size_t nruns = K.run_ap.size();
  fast_j.assign(3 * nruns, -1); // per run and normal axis: does t_j run fastest? (-1: no group with that axis)
  return host_parallel_all(nruns, [&](size_t r) {
    const int cnt = K.run_cnt[r];
    if (cnt % m)
      return false;
    const int a = K.own_agg[K.run_slot[r]];
    const double wtol = geometry_rounding(p, a);
    for (int64_t b = 0; b < cnt; b += m) // b: first point of the group inside run r
      {
        int c = 0;
        for (int d = 0; d < 3; ++d)
          if (std::fabs(K.ap_n(d, r, b)) > 0.5)
            c = d;
        const int ti = c == 0 ? 1 : 0, tj = c == 2 ? 1 : 2;
        // which tangential coordinate changes between the first two points?
        const double h_i = box_side(p, a, ti);
        const bool i_moves = n > 1 && std::fabs(K.ap_x(ti, r, b + 1) - K.ap_x(ti, r, b)) > 1e-9 * h_i;
        const int f = (n == 1 || i_moves) ? 0 : 1;
        signed char &fast = fast_j[3 * r + c];
        if (fast < 0)
          fast = (signed char)f;
        else if (fast != f)
          return false; // the kernel takes one orientation per plane of a run
        const int64_t st_i = f == 0 ? 1 : n, st_j = f == 0 ? n : 1;
        for (int which = 0; which < 2; ++which)
          {
            auto w = [&](int64_t q) { return which ? K.ap_wcross(r, q) : K.ap_wself(r, q); };
            const double w00 = w(b);
            if (which && K.run_nbr[r] < 0)
              continue;
            if (!(w00 > 0.0))
              return false;
            for (int be = 0; be < n; ++be)
              for (int al = 0; al < n; ++al)
                {
                  const int64_t q = b + al * st_i + be * st_j;
                  const double Xi = K.ap_x(ti, r, b + al * st_i), Xj = K.ap_x(tj, r, b + be * st_j);
                  const double h_j = box_side(p, a, tj);
                  if (std::fabs(K.ap_x(ti, r, q) - Xi) > 3e-15 * (std::fabs(Xi) + h_i) ||
                      std::fabs(K.ap_x(tj, r, q) - Xj) > 3e-15 * (std::fabs(Xj) + h_j))
                    return false;
                  const double wf = w(b + al * st_i) * (w(b + be * st_j) / w00);
                  if (std::fabs(w(q) - wf) > wtol * wf)
                    return false;
                }
          }
      }
    return true;
  });
}

// pdh_problem::vq_tensor_n / fq_tensor_n: > 0 a claim to verify, 0 find out (2 .. 8 points per direction are tried, largest
// first: a wrong candidate fails on the first group of points), < 0 do not look
template <class Check>
static int resolve_tensor_hint(int hint, Check &&holds)
{
  if (hint > 0)
    return holds(hint) ? hint : 0;
  if (hint < 0)
    return 0;
  for (int n = 8; n >= 2; --n)
    if (holds(n))
      return n;
  return 0;
}


int resolve_volume_rules(const pdh_problem *p, const Packed &K)
{
  return resolve_tensor_hint(p->vq_tensor_n, [&](int n) { return volume_rules_are_tensor(p, K, n); });
}

// runs are stored slot by slot; the faces of a slot in record order: boundary first, then ascending block rank
void order_runs_of_slots(const Packed &K, FaceAnalysis &A)
{
  const size_t nruns = K.run_ap.size();
  A.order.assign((size_t)K.n_owned, {});
  size_t r = 0;
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      auto &idx = A.order[(size_t)sl];
      for (; r < nruns && K.run_slot[r] == sl; ++r)
        idx.push_back(r);
      std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return K.run_blk[x] < K.run_blk[y]; });
    }
  A.n_ordered = r;
}

// Planes of run r.  An interior face must lie in one plane - or in several, one entry each (whether the element's kernel can take
// that is decided by the table builders).  The boundary "face" of a polytope collects ALL its domain-boundary sub-faces (reference
// source/agglomeration_handler.cc:1575-1613), up to three planes at a corner: it becomes one entry per plane over the same point
// range, and the kernel masks the points of the other planes.  Returns the reason if the run is not a union of axis-aligned planes.
static const char *planes_of_run(const pdh_problem *p, const Packed &K, size_t r, std::vector<Plane> &planes)
{
  const int cnt = K.run_cnt[r];
  if (cnt <= 0)
    return "empty face";
  const int a = K.own_agg[K.run_slot[r]];
  // (tangential components of a computed unit normal: of the order of the rounding of the geometry)
  const double ntol = geometry_rounding(p, a);
  std::vector<double> sum;
  std::vector<int> num;
  for (int q = 0; q < cnt; ++q)
    {
      int c = -1;
      for (int d = 0; d < 3; ++d)
        if (std::fabs(K.ap_n(d, r, q)) > 0.5)
          c = d;
      if (c < 0)
        return "normal not axis-aligned";
      const double sg = K.ap_n(c, r, q) > 0 ? 1.0 : -1.0;
      for (int d = 0; d < 3; ++d)
        {
          const double nd = K.ap_n(d, r, q);
          if (d == c ? std::fabs(nd - sg) > ntol : std::fabs(nd) > ntol)
            return "normal not axis-aligned";
        }
      const double x = K.ap_x(c, r, q);
      const double h = box_side(p, a, c);
      size_t k = 0;
      for (; k < planes.size(); ++k)
        if (planes[k].axis == c && planes[k].sign == sg && std::fabs(planes[k].coord - x) <= 1e-9 * h)
          break;
      if (k == planes.size())
        {
          planes.push_back({c, sg, x});
          sum.push_back(0.0);
          num.push_back(0);
        }
      sum[k] += x;
      num[k] += 1;
    }
  // the kernel evaluates the bases at ONE coordinate per plane (the mean): the points must agree with it to a few ulp
  for (size_t k = 0; k < planes.size(); ++k)
    planes[k].coord = sum[k] / num[k];
  for (int q = 0; q < cnt; ++q)
    for (const Plane &pl : planes)
      if (in_plane(K, r, q, pl, box_side(p, a, pl.axis)) &&
          std::fabs(K.ap_x(pl.axis, r, q) - pl.coord) > 2e-15 * (std::fabs(pl.coord) + box_side(p, a, pl.axis)))
        return "face not planar";
  return nullptr;
}

// The face analysis of the row kernels (pdh_rows.h, term kernels).  Eligible: 3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3, no exchange
// variant, and every polytopal face of every owned polytope a union of pieces of axis-aligned planes (agglomerates of Cartesian
// cells).  The test is made on the packed points themselves, so any description qualifies that has the geometry - there is no
// mesh-type flag.  Planarity is required to a few ulp: the kernels evaluate the bases at ONE plane coordinate per entry (the mean).
bool analyse_faces(const pdh_problem *p, const Packed &K, RowsHost &R, FaceAnalysis &A, std::string *why)
{
  R.fq_tensor_n = resolve_tensor_hint(p->fq_tensor_n, [&](int n) { return face_rules_are_tensor(p, K, n, R.fast_j); });
  if (R.fq_tensor_n == 0)
    R.fast_j.clear();
  if (p->dim != 3 || p->degree < 1 || p->degree > 3 || K.n != pdhr::rows_n_functions(p->degree + 1, p->basis == PDH_BASIS_AGGLODGP ? 1 : 0))
    return refuse(why, "not 3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3");
  if ((int)K.own_agg.size() != K.n_owned) // pseudo slots of the exchange variant
    return refuse(why, "exchange variant");
  const size_t nruns = K.run_ap.size();
  A.planes.assign(nruns, {});
  std::vector<const char *> why_run(nruns, nullptr);
  host_parallel_for(nruns, [&](size_t r) { why_run[r] = planes_of_run(p, K, r, A.planes[r]); });
  for (size_t r = 0; r < nruns; ++r)
    if (why_run[r])
      return refuse(why, why_run[r]);
  R.planar_ok = true;
  order_runs_of_slots(K, A);
  return true;
}

// A run that lies in several planes (the boundary run of a corner polytope; a staircase face towards one neighbour) gives one
// entry per plane, and the kernel skips the sub-faces (groups of a tensor rule, else single points) whose first point is not in the
// entry's plane.  The entry covers only the span [sp_b, sp_e) from the first to the last group of ITS plane - a run of s groups in
// k planes costs the sum of the spans, not k s, in lane tasks and moment sums - and is flagged for masking (returned) only if a
// foreign group lies inside that span.
static bool span_of_plane(const pdh_problem *p, const Packed &K, size_t t, const Plane &pl, int64_t gsz, int64_t &sp_b, int64_t &sp_e)
{
  const double h = box_side(p, K.own_agg[K.run_slot[t]], pl.axis);
  int64_t g_first = -1, g_last = -1;
  const int64_t ng = K.run_cnt[t] / gsz;
  for (int64_t g = 0; g < ng; ++g)
    if (in_plane(K, t, g * gsz, pl, h))
      {
        if (g_first < 0)
          g_first = g;
        g_last = g;
      }
  // (a plane seen only on points that are not the first of their group would be a group straddling planes: not a
  // tensor rule on a rectangle, such runs fail face_rules_are_tensor; with gsz = 1 every point is its own group.
  // Should it happen all the same: the whole run, masked, as before)
  if (g_first < 0)
    g_first = 0, g_last = ng - 1;
  bool foreign_inside = false;
  for (int64_t g = g_first; g <= g_last; ++g)
    foreign_inside = foreign_inside || !in_plane(K, t, g * gsz, pl, h);
  sp_b = g_first * gsz, sp_e = (g_last + 1) * gsz;
  if (sp_e > K.run_cnt[t] || K.run_cnt[t] % gsz) // (a run that is not whole groups: keep all of it)
    sp_b = 0, sp_e = K.run_cnt[t], foreign_inside = true;
  return foreign_inside;
}

// fr_*: one entry per run and plane of every owned slot, in record order; the limits the entries put on the kernel
static void build_face_entries(const pdh_problem *p, const Packed &K, const FaceAnalysis &A, RowsHost &R)
{
  const int64_t gsz = R.fq_tensor_n > 0 ? (int64_t)R.fq_tensor_n * R.fq_tensor_n : 1;
  R.fr_ptr.assign(1, 0);
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      int nf = 0;
      for (size_t t : A.order[(size_t)sl])
        for (const Plane &pl : A.planes[t])
          {
            int64_t sp_b = 0, sp_e = K.run_cnt[t];
            const bool foreign_inside = A.planes[t].size() > 1 && span_of_plane(p, K, t, pl, gsz, sp_b, sp_e);
            // A boundary run with tensor sub-face rules is cut into pieces of at most 32 sub-faces: the kernel forms the moments
            // of a piece in one batch of 64 lane tasks (2 per sub-face), and a corner polytope of 4^3 cells already has 48
            // boundary sub-faces in its run.  Boundary pieces only add to the diagonal block's face tensors, so the cut
            // changes nothing but the order of summation.  (An interior face is one entry: its coupling moments are one set.)
            for (int64_t pc0 = sp_b, pcs = (K.run_nbr[t] < 0 && R.fq_tensor_n > 0) ? 32 * gsz : sp_e - sp_b; pc0 < sp_e; pc0 += pcs)
              {
                R.fr_pbeg.push_back(K.run_ap[t] + pc0);
                R.fr_pcnt.push_back((int32_t)std::min<int64_t>(pcs, sp_e - pc0));
                R.fr_nbr.push_back(K.run_nbr[t]);
                R.fr_axis.push_back(pl.axis);
                R.fr_blk.push_back(K.run_blk[t]);
                R.fr_flags.push_back((foreign_inside ? 1 : 0) | ((R.fq_tensor_n > 0 && R.fast_j[3 * t + pl.axis] == 1) ? 2 : 0));
                R.fr_coord.push_back(pl.coord);
                R.fr_sigma.push_back(K.run_sig[t]);
                R.fr_nsign.push_back(pl.sign);
                if (K.run_nbr[t] >= 0)
                  {
                    ++nf; // the LDS layout of the kernel limits the INTERIOR entries (coupling moments kept per entry)
                    if (A.planes[t].size() > 1)
                      R.multi = true;
                  }
              }
          }
      const int ne = (int)R.fr_pbeg.size() - R.fr_ptr.back();
      if (R.fq_tensor_n > 0)
        {
          int64_t nsub = 0;
          for (size_t f = (size_t)R.fr_ptr.back(); f < R.fr_pbeg.size(); ++f)
            if (R.fr_nbr[f] >= 0)
              nsub += R.fr_pcnt[f] / gsz;
          R.maxs = std::max<int>(R.maxs, (int)nsub);
        }
      R.maxf = std::max(R.maxf, nf);
      R.maxe = std::max(R.maxe, ne);
      R.fr_ptr.push_back((int32_t)R.fr_pbeg.size());
    }
}

// Face tables of the row kernel (pdh_rows.h), from the analysed faces.  Block-shaped polytopes meet every neighbour along ONE plane;
// METIS-like agglomerates meet some along several ("staircase" faces): FE_DGQ(3) has an instantiation for those (RowsHost::multi),
// the other elements need one plane per neighbour and at most pdhr::MAXF neighbours.
bool build_rows_tables(const pdh_problem *p, const Packed &K, const FaceAnalysis &A, const PlanSwitches &sw, RowsHost &R, std::string *why)
{
  const size_t nruns = K.run_ap.size();
  build_face_entries(p, K, A, R);
  if (A.n_ordered != nruns)
    return refuse(why, "run bookkeeping");
  if (sw.rows_verbose)
    {
      int64_t covered = 0, points = 0, masked = 0;
      for (size_t f = 0; f < R.fr_pcnt.size(); ++f)
        covered += R.fr_pcnt[f], masked += (R.fr_flags[f] & 1) ? 1 : 0;
      for (size_t t = 0; t < nruns; ++t)
        points += K.run_cnt[t];
      fprintf(stderr, "row kernel tables: %zu runs, %zu plane entries (%lld masked), %lld face points, %lld covered by the entries (%.2fx)\n",
              nruns, R.fr_pcnt.size(), (long long)masked, (long long)points, (long long)covered, (double)covered / (double)points);
    }
  if (R.maxf > pdhr::MAXF || R.maxe > 16)
    R.multi = true;
  if (R.multi)
    {
      // the MULTI instantiation exists for FE_DGQ(3); its records hold up to 48 entries (the face table of a polytope lives in
      // the lanes of the wave, twelve of which carry the header) and LDS provides one 512-byte slot per interior entry
      if (!(K.n1d == 4 && p->basis != PDH_BASIS_AGGLODGP))
        return refuse(why, "a neighbour is met along several planes, or a polytope has more than 6 interior / 16 face entries: FE_DGQ(3) only");
      if (R.maxe > 48 || R.maxf > 40)
        return refuse(why, "too many face entries on a polytope (48 plane entries, 40 of them interior)");
      R.maxe = (R.maxe + 3) / 4 * 4;
    }
  else
    R.maxe = 16, R.maxf = pdhr::MAXF;
  // per-slot records: header (number of entries, own box as lo / 1/h, row base / length / position of the own block,
  // volume point range) + one entry per face with the neighbour's box - everything the kernel needs about a polytope in
  // one contiguous block
  constexpr int HDR = pdhr::ROWS_HDR, ENT = pdhr::ROWS_ENT;
  const int MAXE = R.maxe, REC = HDR + MAXE * ENT;
  R.meta.assign((size_t)K.n_owned * REC, 0.0);
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      const int f0 = R.fr_ptr[sl], nf = R.fr_ptr[sl + 1] - f0;
      if (nf > MAXE)
        return refuse(why, "too many face entries on a polytope");
      double *rec = R.meta.data() + (size_t)sl * REC;
      rec[0] = as_d(nf);
      write_slot_header(rec, p, K, (size_t)sl);
      rec[10] = as_d(K.vq_ptr[sl]), rec[11] = as_d(K.vq_ptr[sl + 1]);
      for (int e = 0; e < nf; ++e)
        {
          double *en = rec + HDR + e * ENT;
          const int f = f0 + e, nb = R.fr_nbr[f];
          en[0] = as_d(R.fr_pbeg[f]);
          // (nb and fr_blk are -1 on the boundary: into the upper word by a product, a shift of a negative value is undefined)
          en[1] = as_d((long long)(uint32_t)R.fr_pcnt[f] | ((long long)nb * (1LL << 32)));
          en[2] = as_d((long long)(R.fr_axis[f] & 0xff) | ((long long)(R.fr_flags[f] & 0xff) << 8) | ((long long)R.fr_blk[f] * (1LL << 32)));
          en[3] = R.fr_coord[f];
          en[4] = R.fr_sigma[f];
          en[5] = R.fr_nsign[f];
          write_box(en + 6, en + 9, p, nb);
        }
    }
  return true;
}

// Second half of the eligibility test: structure of the volume rules (vq_n), and - every kind but FE_DGQ(3) has no
// general-point paths - tensor rules everywhere and no face entry with more sub-faces than the 64 lane tasks of a batch
// hold (pdh_rows.h, P2).
bool rows_kind_applies(const pdh_problem *p, const Packed &K, const RowsHost &RH, int &vq_n, bool &tensor_only, std::string *why)
{
  vq_n = resolve_volume_rules(p, K);
  bool ok = vq_n > 0 && RH.fq_tensor_n > 0;
  const int64_t m = (int64_t)RH.fq_tensor_n * RH.fq_tensor_n;
  for (size_t f = 0; ok && f < RH.fr_pcnt.size(); ++f)
    ok = RH.fr_pcnt[f] / m <= 32;
  tensor_only = ok;
  if (K.n1d == 4) // degree 3 has the general-point paths (pdh_rows.h: GENERAL)
    return true;
  if (!ok && why)
    *why = "this element takes the row kernel only with tensor-product rules on every sub-cell and sub-face";
  return ok;
}

// ---- merged cells and sub-faces of the term kernels --------------------------------------------------------------------------------
// A term is a product of three 1-D matrices, one per direction; the kernels sum the terms of all cells (sub-faces) of a polytope.
// Where cells form a TENSOR GRID - cell (i, j, k) has the i-th interval of the 1-D rules along x, the j-th along y, the k-th along z,
// and its weight factorises - the sum over a sub-grid of products is the product of the sums over the intervals:
//   sum_ijk A_i (x) B_j (x) C_k = (sum_i A_i) (x) (sum_j B_j) (x) (sum_k C_k),
// i.e. the sub-grid is ONE cell with composite 1-D rules of several intervals.  Block agglomerates (what an R-tree gives on a structured
// grid) are such grids as a whole; so are the sub-faces a polytope shares with one neighbour in one plane; METIS-like agglomerates
// contain pairs and quads of cells that are.  The cells (the sub-faces of a plane) are covered greedily by boxes (rectangles) of
// occupied grid slots - found on the data (first points of the rules, compared to rounding; weights checked for the factorisation),
// never assumed; what fits no larger box stays a box of one.  A composite rule has at most 8 points and TERMS_MI intervals (register
// slots of a lane task).
namespace
{
struct TermsMerged
{
  struct Cell { int32_t ivl[3][TERMS_MI]; };
  struct Sf { int64_t pb; int c, pos, fj, ni, nj; int32_t ivl[2][TERMS_MI]; };
  std::vector<Cell> cells;
  std::vector<Sf> sfs;      // run by run, in the order of the record's runs
  std::vector<int> run_off; // [runs + 1] into sfs
  int nsf = 0, nsi = 0, ivl_c = 1, ivl_f = 1; // sub-faces, interior sub-faces, most intervals of a cell / sub-face rule
  int64_t n_in = 0;                           // cells + sub-faces as given
  size_t run_size(size_t e) const { return (size_t)(run_off[e + 1] - run_off[e]); }
  const Sf *run_begin(size_t e) const { return sfs.data() + run_off[e]; }
};
// a sub-face as the merge sees it: normal axis, side, orientation of its rule, plane and first tangential coordinates
struct TermsSfGeom { int c, pos, fj; double z, xi, xj; };
// indices of the values of v in the sorted list of its distinct values (equal within tol); returns the number of distinct values
int cluster_1d(const std::vector<double> &v, double tol, std::vector<int> &idx)
{
  static thread_local std::vector<size_t> o; // (scratch: this runs once per polytope and plane on every host thread)
  o.resize(v.size());
  for (size_t i = 0; i < o.size(); ++i)
    o[i] = i;
  std::sort(o.begin(), o.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
  idx.assign(v.size(), 0);
  int n = 0;
  for (size_t k = 0; k < o.size(); ++k)
    {
      if (k > 0 && v[o[k]] - v[o[k - 1]] > tol)
        ++n;
      idx[o[k]] = n;
    }
  return v.empty() ? 0 : n + 1;
}

// Greedy cover of the occupied slots of a grid of nd[0] x nd[1] x nd[2] by boxes of at most mx[d] slots along d (rectangles: nd[2] =
// mx[2] = 1).  at(i, j, k): the member on a slot or -1; from every member not yet taken, origins in k, j, i order, the largest box of
// taken-free, occupied slots whose members all fit the box's origin (fits(member, origin)) is emitted (volume; ties: the first found,
// sizes descending with the last axis outermost).
template <class At, class Fits, class Emit>
void cover_grid(const int *nd, const int *mx, std::vector<char> &taken, At &&at, Fits &&fits, Emit &&emit)
{
  auto all_in_box = [&](const int *o, const int *sz, auto &&pred) {
    for (int k = 0; k < sz[2]; ++k)
      for (int j = 0; j < sz[1]; ++j)
        for (int i = 0; i < sz[0]; ++i)
          if (!pred(at(o[0] + i, o[1] + j, o[2] + k)))
            return false;
    return true;
  };
  auto box_ok = [&](const int *o, const int *sz) { // inside the grid, all slots occupied and free, then: all members fit
    return o[0] + sz[0] <= nd[0] && o[1] + sz[1] <= nd[1] && o[2] + sz[2] <= nd[2] &&
           all_in_box(o, sz, [&](int u) { return u >= 0 && !taken[(size_t)u]; }) && all_in_box(o, sz, [&](int u) { return fits(u, o); });
  };
  for (int k0 = 0; k0 < nd[2]; ++k0)
    for (int j0 = 0; j0 < nd[1]; ++j0)
      for (int i0 = 0; i0 < nd[0]; ++i0)
        {
          const int u0 = at(i0, j0, k0);
          if (u0 < 0 || taken[(size_t)u0])
            continue;
          const int o[3] = {i0, j0, k0};
          int best[3] = {1, 1, 1}, bestv = 1;
          for (int c = mx[2]; c >= 1; --c)
            for (int b = mx[1]; b >= 1; --b)
              for (int a = mx[0]; a >= 1; --a)
                {
                  const int sz[3] = {a, b, c};
                  if (a * b * c > bestv && box_ok(o, sz))
                    best[0] = a, best[1] = b, best[2] = c, bestv = a * b * c;
                }
          all_in_box(o, best, [&](int u) { return taken[(size_t)u] = 1; });
          emit(o, best);
        }
}

// ---- where the merge looks: the packed points, or the cells' boxes of the cartesian description -------------------------------------
struct SlotGeom // the polytope of owned slot sl
{
  const pdh_problem *p;
  const Packed &K;
  size_t sl;
  int a, tn, fn; // polytope, points per direction of the volume / sub-face rules
  int64_t m3, gsz;
  double hbox[3], wtol;
  SlotGeom(const pdh_problem *p_, const Packed &K_, size_t sl_, int tn_, int fn_)
    : p(p_), K(K_), sl(sl_), a(K_.own_agg[sl_]), tn(tn_), fn(fn_), m3((int64_t)tn_ * tn_ * tn_), gsz((int64_t)fn_ * fn_)
  {
    for (int d = 0; d < 3; ++d)
      hbox[d] = box_side(p, a, d);
    wtol = 8.0 * geometry_rounding(p, a);
  }
};
struct FromPoints : SlotGeom
{
  using SlotGeom::SlotGeom;
  double cell_key(int d, int u) const { return K.vqx_h[d * K.vq_stride_h + K.vq_ptr[sl] + u * m3]; }
  // does cell u carry, along every direction d, the 1-D rule of cell ref[d], and does its weight factorise (origin cell uo)?
  bool cell_fits(int u, const int *ref, int uo) const
  {
    const int64_t b0 = K.vq_ptr[sl], st = K.vq_stride_h, bu = b0 + u * m3;
    const int64_t step[3] = {1, tn, (int64_t)tn * tn};
    const double wu = K.vqw_h[bu], w0 = K.vqw_h[b0 + uo * m3];
    double wf = 1.0;
    for (int d = 0; d < 3; ++d)
      {
        const int64_t br = b0 + ref[d] * m3;
        const double wr = K.vqw_h[br];
        wf *= wr / w0;
        for (int i = 0; i < tn; ++i)
          {
            const double X = K.vqx_h[d * st + br + i * step[d]];
            if (!(std::fabs(K.vqx_h[d * st + bu + i * step[d]] - X) <= 3e-15 * (std::fabs(X) + hbox[d]) &&
                  std::fabs(K.vqw_h[bu + i * step[d]] / wu - K.vqw_h[br + i * step[d]] / wr) <= wtol * (K.vqw_h[br + i * step[d]] / wr)))
              return false;
          }
      }
    return std::fabs(wu - w0 * wf) <= wtol * wu;
  }
  void sf_geom(size_t t, int g, TermsSfGeom &s) const
  {
    s.c = 0;
    for (int d = 0; d < 3; ++d)
      if (std::fabs(K.ap_n(d, t, g * gsz)) > 0.5)
        s.c = d;
    s.pos = K.ap_n(s.c, t, g * gsz) > 0 ? 1 : 0;
    const int ti = s.c == 0 ? 1 : 0, tj = s.c == 2 ? 1 : 2;
    s.z = K.ap_x(s.c, t, g * gsz);
    s.xi = K.ap_x(ti, t, g * gsz), s.xj = K.ap_x(tj, t, g * gsz);
  }
  // does sub-face g of run t carry the tangential rules of gi (along ti) and gj (along tj), and do its weights factorise (origin go)?
  bool sf_fits(size_t t, int g, int gi, int gj, int go, int ti, int tj, int fj) const
  {
    const int64_t st_i = fj ? fn : 1, st_j = fj ? 1 : fn;
    for (int which = 0; which < 2; ++which)
      { // own-side and cross weights (the latter zero on the boundary)
        auto W = [&](int gq, int64_t q) { return which ? K.ap_wcross(t, gq * gsz + q) : K.ap_wself(t, gq * gsz + q); };
        const double wu = W(g, 0), wi = W(gi, 0), wj = W(gj, 0), wo = W(go, 0);
        if (which && wu == 0.0 && wo == 0.0)
          continue;
        if (!(wu > 0.0 && wo > 0.0 && std::fabs(wu - wi * wj / wo) <= wtol * wu))
          return false;
        for (int al = 0; al < fn; ++al)
          {
            const double Xi = K.ap_x(ti, t, gi * gsz + al * st_i), Xj = K.ap_x(tj, t, gj * gsz + al * st_j);
            if (!(std::fabs(K.ap_x(ti, t, g * gsz + al * st_i) - Xi) <= 3e-15 * (std::fabs(Xi) + hbox[ti]) &&
                  std::fabs(K.ap_x(tj, t, g * gsz + al * st_j) - Xj) <= 3e-15 * (std::fabs(Xj) + hbox[tj]) &&
                  std::fabs(W(g, al * st_i) / wu - W(gi, al * st_i) / wi) <= wtol * (W(gi, al * st_i) / wi) &&
                  std::fabs(W(g, al * st_j) / wu - W(gj, al * st_j) / wj) <= wtol * (W(gj, al * st_j) / wj)))
              return false;
          }
      }
    return true;
  }
};
struct FromBoxes : SlotGeom // same interval = same extent along the direction
{
  using SlotGeom::SlotGeom;
  const double *cell_box(int u) const { return K.cart->cell_box + (size_t)K.cart->vq_cell[p->vq_ptr[a] / m3 + u] * 6; }
  // (the side-0 cell's box carries the sub-face)
  const double *sf_box(size_t t, int g) const { return K.cart->cell_box + (size_t)K.cart->fq_cell[K.pk_fq[t] / gsz + g] * 6; }
  bool same_extent(const double *x, const double *y, int d) const
  {
    return std::fabs(x[d] - y[d]) <= 1e-12 * hbox[d] && std::fabs(x[3 + d] - y[3 + d]) <= 1e-12 * hbox[d];
  }
  double cell_key(int d, int u) const { return cell_box(u)[d]; }
  bool cell_fits(int u, const int *ref, int) const
  {
    for (int d = 0; d < 3; ++d)
      if (!same_extent(cell_box(u), cell_box(ref[d]), d))
        return false;
    return true;
  }
  void sf_geom(size_t t, int g, TermsSfGeom &s) const
  {
    const int lf = K.cart->fq_face[K.pk_fq[t] / gsz + g];
    const double *bx = sf_box(t, g);
    s.c = lf >> 1;
    s.pos = ((lf & 1) != 0) == ((K.pk_flags[t] & 1) != 0) ? 1 : 0;
    s.z = bx[(lf & 1) ? 3 + s.c : s.c];
    const int ti = s.c == 0 ? 1 : 0, tj = s.c == 2 ? 1 : 2;
    s.xi = bx[ti], s.xj = bx[tj];
  }
  bool sf_fits(size_t t, int g, int gi, int gj, int, int ti, int tj, int) const
  {
    return same_extent(sf_box(t, g), sf_box(t, gi), ti) && same_extent(sf_box(t, g), sf_box(t, gj), tj);
  }
};

// ---------------- cells: a greedy cover by boxes of at most mc intervals per direction.  The cells are placed on the tensor grid of
// their clustered first points; a box of cells that share their 1-D rules per interval (and whose weights factorise) becomes one cell
// with composite rules.  A polytope that is a full grid is cut into sub-grids of mc intervals exactly as a chunking would; METIS-like
// agglomerates keep what pairs and quads they have.  False: the cells are on no grid (nothing emitted).
template <class Src>
bool merge_cells(const Src &S, int ncell, int mc, std::vector<TermsMerged::Cell> &cells)
{
  static thread_local std::vector<double> key[3];
  static thread_local std::vector<int> idx[3], grid;
  static thread_local std::vector<char> taken;
  int nd[3];
  for (int d = 0; d < 3; ++d)
    {
      key[d].resize((size_t)ncell);
      for (int u = 0; u < ncell; ++u)
        key[d][(size_t)u] = S.cell_key(d, u);
      nd[d] = cluster_1d(key[d], 1e-9 * S.hbox[d], idx[d]);
    }
  const int64_t nslot = (int64_t)nd[0] * nd[1] * nd[2];
  if (nslot > 4096)
    return false;
  grid.assign((size_t)nslot, -1);
  for (int u = 0; u < ncell; ++u)
    {
      int &g = grid[(size_t)(idx[0][u] + nd[0] * (idx[1][u] + nd[1] * idx[2][u]))];
      if (g >= 0) // (two cells on one slot: no grid)
        return false;
      g = u;
    }
  auto at = [&](int i, int j, int k) { return grid[(size_t)(i + nd[0] * (j + nd[1] * k))]; };
  // the cell of the box at origin o that shares the interval of cell u along d
  auto ref_cell = [&](int u, const int *o, int d) {
    int r[3] = {o[0], o[1], o[2]};
    r[d] = idx[d][u];
    return at(r[0], r[1], r[2]);
  };
  const int mx[3] = {mc, mc, mc};
  taken.assign((size_t)ncell, 0);
  cover_grid(
    nd, mx, taken, at,
    [&](int u, const int *o) {
      const int ref[3] = {ref_cell(u, o, 0), ref_cell(u, o, 1), ref_cell(u, o, 2)};
      return S.cell_fits(u, ref, at(o[0], o[1], o[2]));
    },
    [&](const int *o, const int *best) {
      TermsMerged::Cell cm;
      for (int d = 0; d < 3; ++d)
        for (int t = 0; t < TERMS_MI; ++t)
          {
            int r[3] = {o[0], o[1], o[2]};
            r[d] = o[d] + t;
            cm.ivl[d][t] = t < best[d] ? at(r[0], r[1], r[2]) : -1;
          }
      cells.push_back(cm);
    });
  return true;
}

// ---------------- sub-faces of run t: plane by plane (axis, side, orientation, coordinate), a greedy cover of the plane's sub-faces by
// rectangles of at most mf x mf intervals (as for the cells above); mf <= 1: as given
template <class Src>
void merge_sub_faces(const Src &S, size_t t, const RowsHost &RH, int mf, std::vector<TermsMerged::Sf> &out)
{
  const Packed &K = S.K;
  const int64_t gsz = S.gsz;
  const int ns = (int)(K.run_cnt[t] / gsz);
  static thread_local std::vector<TermsSfGeom> gs;
  gs.resize((size_t)ns);
  for (int g = 0; g < ns; ++g)
    {
      S.sf_geom(t, g, gs[(size_t)g]);
      gs[(size_t)g].fj = RH.fast_j[3 * t + gs[(size_t)g].c] == 1 ? 1 : 0;
    }
  auto single = [&](int g) {
    TermsMerged::Sf f{}; // (ivl: zeros)
    f.pb = K.run_ap[t] + g * gsz;
    f.c = gs[(size_t)g].c, f.pos = gs[(size_t)g].pos, f.fj = gs[(size_t)g].fj, f.ni = f.nj = 1;
    out.push_back(f);
  };
  if (mf <= 1 || ns <= 1)
    {
      for (int g = 0; g < ns; ++g)
        single(g);
      return;
    }
  static thread_local std::vector<char> used, ftaken;
  static thread_local std::vector<int> mem, ii, jj, fgrid;
  static thread_local std::vector<double> ki, kj;
  used.assign((size_t)ns, 0);
  for (int g0 = 0; g0 < ns; ++g0)
    {
      if (used[(size_t)g0])
        continue;
      const TermsSfGeom r0 = gs[(size_t)g0];
      mem.clear();
      for (int g = g0; g < ns; ++g)
        if (!used[(size_t)g] && gs[(size_t)g].c == r0.c && gs[(size_t)g].pos == r0.pos && gs[(size_t)g].fj == r0.fj &&
            std::fabs(gs[(size_t)g].z - r0.z) <= 1e-9 * S.hbox[r0.c])
          {
            mem.push_back(g);
            used[(size_t)g] = 1;
          }
      const int c = r0.c, ti = c == 0 ? 1 : 0, tj = c == 2 ? 1 : 2;
      int nd[3] = {0, 0, 1};
      bool ok = mem.size() > 1; // (a plane with one sub-face: nothing to merge)
      if (ok)
        {
          ki.resize(mem.size()), kj.resize(mem.size());
          for (size_t m = 0; m < mem.size(); ++m)
            ki[m] = gs[(size_t)mem[m]].xi, kj[m] = gs[(size_t)mem[m]].xj;
          nd[0] = cluster_1d(ki, 1e-9 * S.hbox[ti], ii), nd[1] = cluster_1d(kj, 1e-9 * S.hbox[tj], jj);
          ok = (int64_t)nd[0] * nd[1] <= 4096;
        }
      if (ok)
        {
          fgrid.assign((size_t)nd[0] * nd[1], -1);
          for (size_t m = 0; m < mem.size() && ok; ++m)
            {
              int &gg = fgrid[(size_t)(ii[m] + nd[0] * jj[m])];
              ok = gg < 0;
              gg = (int)m;
            }
        }
      if (!ok)
        {
          for (int g : mem)
            single(g);
          continue;
        }
      auto atm = [&](int i, int j, int = 0) { return fgrid[(size_t)(i + nd[0] * j)]; }; // member index or -1
      auto at = [&](int i, int j) { return mem[(size_t)atm(i, j)]; };                    // sub-face of the run
      const int mx[3] = {mf, mf, 1};
      ftaken.assign(mem.size(), 0);
      cover_grid(
        nd, mx, ftaken, atm,
        [&](int m, const int *o) {
          return S.sf_fits(t, mem[(size_t)m], at(ii[(size_t)m], o[1]), at(o[0], jj[(size_t)m]), at(o[0], o[1]), ti, tj, r0.fj);
        },
        [&](const int *o, const int *best) {
          TermsMerged::Sf f;
          const int go = at(o[0], o[1]);
          f.pb = K.run_ap[t] + go * gsz;
          f.c = c, f.pos = r0.pos, f.fj = r0.fj;
          f.ni = best[0], f.nj = best[1];
          for (int q = 0; q < TERMS_MI; ++q)
            {
              f.ivl[0][q] = q < best[0] ? (int32_t)((at(o[0] + q, o[1]) - go) * gsz) : 0;
              f.ivl[1][q] = q < best[1] ? (int32_t)((at(o[0], o[1] + q) - go) * gsz) : 0;
            }
          out.push_back(f);
        });
    }
}

// the cells and sub-faces slot sl is summed over (order: its runs in record order); enabled = false: as given
template <class Src>
void merge_terms_of_slot(const Src &S, const RowsHost &RH, const std::vector<size_t> &order, bool enabled, TermsMerged &M)
{
  const Packed &K = S.K;
  const int tn = S.tn, fn = S.fn;
  const int ncell = (int)((K.vq_ptr[S.sl + 1] - K.vq_ptr[S.sl]) / S.m3);
  const int mc = tn >= 1 && tn <= 4 ? std::min(TERMS_MI, 8 / tn) : 1;
  if (!(enabled && mc > 1 && ncell > 1 && merge_cells(S, ncell, mc, M.cells)))
    {
      M.cells.resize((size_t)ncell);
      for (int u = 0; u < ncell; ++u)
        for (int d = 0; d < 3; ++d)
          for (int i = 0; i < TERMS_MI; ++i)
            M.cells[(size_t)u].ivl[d][i] = i == 0 ? u : -1;
    }
  const int mf = enabled && fn >= 1 && fn <= 4 ? std::min(TERMS_MI, 8 / fn) : 1;
  M.run_off.assign(order.size() + 1, 0);
  size_t tot = 0;
  for (size_t t : order)
    tot += (size_t)(K.run_cnt[t] / S.gsz);
  M.sfs.reserve(tot);
  // summary (build_terms_tables reduces these instead of walking the lists again)
  M.n_in = ncell + (int64_t)tot;
  for (size_t e = 0; e < order.size(); ++e)
    {
      merge_sub_faces(S, order[e], RH, mf, M.sfs);
      M.run_off[e + 1] = (int)M.sfs.size();
      M.nsf += (int)M.run_size(e);
      if (K.run_nbr[order[e]] >= 0)
        M.nsi += (int)M.run_size(e);
    }
  for (const auto &f : M.sfs)
    M.ivl_f = std::max(M.ivl_f, std::max(f.ni, f.nj));
  for (const auto &c : M.cells)
    for (int d = 0; d < 3; ++d)
      {
        int k = 0;
        for (int i = 0; i < TERMS_MI; ++i)
          k += c.ivl[d][i] >= 0 ? 1 : 0;
        M.ivl_c = std::max(M.ivl_c, k);
      }
}

void merge_terms(const pdh_problem *p, const Packed &K, const RowsHost &RH, const FaceAnalysis &A, int tn, bool enabled,
                 std::vector<TermsMerged> &MG)
{
  MG.assign((size_t)K.n_owned, TermsMerged());
  host_parallel_for((size_t)K.n_owned, [&](size_t sl) {
    if (K.cart)
      merge_terms_of_slot(FromBoxes(p, K, sl, tn, RH.fq_tensor_n), RH, A.order[sl], enabled, MG[sl]);
    else
      merge_terms_of_slot(FromPoints(p, K, sl, tn, RH.fq_tensor_n), RH, A.order[sl], enabled, MG[sl]);
  });
}

constexpr int PDH_TERMS_LDS_CAP = 40 * 1024; // bytes per workgroup: four resident waves per CU at least

// the limits of the kernels on the runs and cells of a polytope; T.maxruns
bool check_runs_of_slots(const Packed &K, const FaceAnalysis &A, int64_t gsz, int64_t m3, TermsHost &T, std::string *why)
{
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      const auto &idx = A.order[(size_t)sl];
      int nb = 0;
      for (size_t t : idx)
        {
          if (K.run_cnt[t] % gsz)
            return refuse(why, "term kernel: a face is not made of whole sub-face rules");
          if (K.run_nbr[t] < 0)
            ++nb;
        }
      if (nb > 1)
        return refuse(why, "term kernel: more than one boundary run on a polytope");
      const int64_t nq = K.vq_ptr[sl + 1] - K.vq_ptr[sl];
      if (nq % m3 || nq / m3 > 65535 || idx.size() > 250)
        return refuse(why, "term kernel: too many cells or faces on a polytope");
      T.maxruns = std::max<int>(T.maxruns, (int)idx.size());
    }
  if (A.n_ordered != K.run_ap.size())
    return refuse(why, "run bookkeeping");
  T.maxruns = std::max(T.maxruns, 1);
  return true;
}

// record, sub-face list and cell list of slot sl; false: the boundary run is not run 0 (the kernel takes it to be)
bool write_terms_of_slot(const pdh_problem *p, const Packed &K, const std::vector<size_t> &idx, const TermsMerged &M, size_t sl, TermsHost &T)
{
  constexpr int HDR = pdht::TERMS_HDR, ENT = pdht::TERMS_ENT;
  double *rec = T.meta.data() + sl * (HDR + T.maxruns * ENT);
  const int64_t at0 = (int64_t)sl * T.maxsf;
  int64_t at = at0;
  int nsfb = 0, e = 0;
  bool ok = true;
  for (size_t t : idx)
    {
      const TermsMerged::Sf *fs = M.run_begin((size_t)e);
      const int ns = (int)M.run_size((size_t)e);
      double *en = rec + HDR + e * ENT;
      en[0] = as_d((long long)(uint32_t)(at - at0) | ((long long)ns << 32));
      en[1] = as_d((long long)K.run_blk[t]);
      en[2] = K.run_sig[t];
      write_box(en + 3, en + 6, p, K.run_nbr[t]);
      if (K.run_nbr[t] < 0)
        {
          nsfb += ns;
          ok = ok && e == 0;
        }
      for (int q = 0; q < ns; ++q, ++at)
        {
          const TermsMerged::Sf &f = fs[q];
          T.sf_pt[(size_t)at] = f.pb;
          T.sf_info[(size_t)at] = e | (f.c << 8) | (f.pos << 10) | (f.fj << 11) | (f.ni << 12) | (f.nj << 15);
          for (int d = 0; d < 2; ++d)
            for (int i = 0; i < TERMS_MI; ++i)
              T.sf_ivl[((size_t)at * 2 + d) * TERMS_MI + i] = f.ivl[d][i];
        }
      ++e;
    }
  for (size_t u = 0; u < M.cells.size(); ++u)
    for (int d = 0; d < 3; ++d)
      for (int i = 0; i < TERMS_MI; ++i)
        T.cell_ivl[((sl * T.maxcell + u) * 3 + d) * TERMS_MI + i] = M.cells[u].ivl[d][i];
  rec[0] = as_d((long long)idx.size() | ((long long)M.cells.size() << 16) | ((long long)nsfb << 32));
  write_slot_header(rec, p, K, sl);
  rec[10] = as_d(K.vq_ptr[sl]), rec[11] = as_d((long long)(at - at0));
  return ok;
}
} // namespace

// Tables of the term kernels: per owned polytope one record and the lists of its sub-faces and cells (TermsHost, pdh_plan.h).
bool build_terms_tables(const pdh_problem *p, const Packed &K, const RowsHost &RH, const FaceAnalysis &A, int vq_n, const PlanSwitches &sw,
                        TermsHost &T, std::string *why)
{
  const int basis = p->basis == PDH_BASIS_AGGLODGP ? 1 : 0;
  if (p->dim != 3 || !pdht::terms_has_kind(K.n1d, basis))
    return refuse(why, "term kernel: 3-D FE_DGQ(1,2) / FE_AggloDGP(1..3) only");
  // (which condition failed: origins far from zero leave the rules tensor-product only to more than geometry_rounding allows)
  if (!RH.planar_ok)
    return refuse(why, "term kernel: needs faces that are unions of axis-aligned planes");
  if (RH.fq_tensor_n <= 0)
    return refuse(why, "term kernel: needs tensor-product rules on every sub-face (the face points are not, to the rounding bound of the geometry)");
  if (vq_n <= 0)
    return refuse(why, "term kernel: needs tensor-product rules on every sub-cell (the volume points are not, to the rounding bound of the geometry)");
  if ((int)K.own_agg.size() != K.n_owned)
    return refuse(why, "term kernel: exchange variant");
  const int fn = RH.fq_tensor_n;
  const int64_t m3 = (int64_t)vq_n * vq_n * vq_n;
  if (!check_runs_of_slots(K, A, (int64_t)fn * fn, m3, T, why))
    return false;
  auto tnow = [] { return std::chrono::steady_clock::now(); };
  auto t_prev = tnow();
  auto tlap = [&](const char *what) {
    if (sw.trace)
      fprintf(stderr, "[build_terms_tables] %-28s %6.1f ms\n", what, std::chrono::duration<double, std::milli>(tnow() - t_prev).count());
    t_prev = tnow();
  };
  tlap("run order");
  // cells and sub-faces the kernel sums over: merged where they form tensor grids; PDH_TERMS_MERGE=0: as given
  std::vector<TermsMerged> MG;
  merge_terms(p, K, RH, A, vq_n, sw.terms_merge != 0, MG);
  if (sw.terms_merge == 1)
    { // composite rules cost every lane task of the problem 8 instead of 4 register slots: taken when they remove at least a third of
      // what is summed over - block agglomerates lose 7 / 8 of their cells and 3 / 4 of their sub-faces, METIS-like ones 44 % of their
      // cells but only 17 % of their sub-faces (23 % together) and ran 2-10 % slower merged (profiles/r04_terms_merge.txt).
      // PDH_TERMS_MERGE=2 merges whatever can be merged.
      int64_t n_in = 0, n_out = 0;
      for (const auto &m : MG)
        n_in += m.n_in, n_out += (int64_t)m.cells.size() + m.nsf;
      if (3 * n_out > 2 * n_in)
        merge_terms(p, K, RH, A, vq_n, false, MG);
    }
  tlap("merge");
  int ivl_c = 1, ivl_f = 1;
  for (int sl = 0; sl < K.n_owned; ++sl)
    {
      const TermsMerged &M = MG[(size_t)sl];
      ivl_c = std::max(ivl_c, M.ivl_c), ivl_f = std::max(ivl_f, M.ivl_f);
      T.n_sf_out += M.nsf;
      T.n_sf_in += M.n_in - (K.vq_ptr[sl + 1] - K.vq_ptr[sl]) / m3;
      T.n_cells_in += (K.vq_ptr[sl + 1] - K.vq_ptr[sl]) / m3;
      T.n_cells_out += (int64_t)M.cells.size();
      if (M.nsf > 65535)
        return refuse(why, "term kernel: too many sub-faces on a polytope");
      T.maxsf = std::max(T.maxsf, M.nsf);
      T.maxsi = std::max(T.maxsi, M.nsi);
      T.maxcell = std::max<int>(T.maxcell, (int)M.cells.size());
    }
  T.task_pts = std::max(vq_n * ivl_c, fn * ivl_f);
  tlap("maxima");
  {
    // one pass or two (pdh_terms.h: SPLIT): whichever lets more single-wave workgroups stay resident on a CU - by LDS (160 KB in
    // granules of 1280 bytes), capped by the 12 waves the kernels' registers allow; a tie goes to the single pass (fewer
    // instructions), and so does FE_DGQ(2): with 27 functions its phases are bound by VALU issue rather than by latency, and the
    // second evaluation of the bases costs more than three more waves give (grown agglomerates of the bench cells: 0.79 ms in one
    // pass at 6 waves, 0.83 in two at 9; FE_AggloDGP(3) 0.71 -> 0.59, FE_AggloDGP(2) 0.29 -> 0.24: profiles/r04_terms_split.txt)
    const int one = pdht::terms_lds_bytes(K.n1d, basis, T.maxruns, T.maxsf, T.maxsi, T.maxcell, 0);
    const int two = pdht::terms_lds_bytes(K.n1d, basis, T.maxruns, T.maxsf, T.maxsi, T.maxcell, 1);
    auto waves = [](int bytes) { return bytes <= 0 ? 0 : std::min(12, (int)(160 * 1024 / (((int64_t)bytes + 1279) / 1280 * 1280))); };
    // (diagnostics: PDH_TERMS_SPLIT = 0 / 1 forces the form)
    T.split = sw.terms_split >= 0 ? sw.terms_split : ((waves(two) > waves(one) && K.n <= 20) ? 1 : 0);
    if (pdht::terms_has_kind(K.n1d, basis) == 2)
      T.split = 0; // (workgroup kernel: no such form)
    T.lds_bytes = T.split ? two : one;
  }
  if (T.lds_bytes <= 0 || T.lds_bytes > PDH_TERMS_LDS_CAP)
    return refuse(why, "term kernel: the tables of the largest polytope do not fit its LDS budget (moment-based kinds take over)");
  // the sub-faces (cells) of a polytope stand at a fixed stride (maxsf, maxcell): the kernel requests them together with the record
  T.maxsf = std::max(T.maxsf, 1);
  T.maxcell = std::max(T.maxcell, 1);
  T.sf_pt.assign((size_t)K.n_owned * T.maxsf, 0);
  T.sf_info.assign((size_t)K.n_owned * T.maxsf, 0);
  T.sf_ivl.assign((size_t)K.n_owned * T.maxsf * 2 * TERMS_MI, 0);
  T.cell_ivl.assign((size_t)K.n_owned * T.maxcell * 3 * TERMS_MI, -1);
  T.meta.assign((size_t)K.n_owned * (pdht::TERMS_HDR + T.maxruns * pdht::TERMS_ENT), 0.0);
  const bool ok = host_parallel_all((size_t)K.n_owned, [&](size_t sl) { return write_terms_of_slot(p, K, A.order[sl], MG[sl], sl, T); });
  tlap("tables");
  return ok || refuse(why, "term kernel: run order");
}

PlanSwitches read_plan_switches()
{
  PlanSwitches s;
  auto first = [](const char *name) { return getenv(name) ? getenv(name)[0] : '\0'; };
  s.terms_merge = first("PDH_TERMS_MERGE") == '0' ? 0 : (first("PDH_TERMS_MERGE") == '2' ? 2 : 1);
  s.terms_split = getenv("PDH_TERMS_SPLIT") ? (first("PDH_TERMS_SPLIT") == '1' ? 1 : 0) : -1;
  s.trace = getenv("PDH_TRACE_SETUP") != nullptr;
  s.rows_verbose = getenv("PDH_ROWS_VERBOSE") != nullptr;
  s.terms_off = first("PDH_TERMS") == '0';
  s.terms_dgq3_off = first("PDH_TERMS_DGQ3") == '0';
  s.rows_waves_per_cu = getenv("PDH_ROWS_WAVES_PER_CU") ? atoi(getenv("PDH_ROWS_WAVES_PER_CU")) : 0;
  s.rows_lds_pad = getenv("PDH_ROWS_LDS_PAD") ? (size_t)atol(getenv("PDH_ROWS_LDS_PAD")) : 0;
  s.terms_wg_waves = getenv("PDH_TERMS_WG_WAVES") && atoi(getenv("PDH_TERMS_WG_WAVES")) == 4 ? 4 : 8;
  s.terms_wg_batch = getenv("PDH_TERMS_WG_BATCH") ? atoi(getenv("PDH_TERMS_WG_BATCH")) : 0;
  return s;
}

// sw.terms_off keeps the kinds of pdh_rows.h, sw.terms_dgq3_off keeps them for FE_DGQ(3) only.  (FE_DGQ(3) has the
// workgroup-per-polytope form of the term kernel, pdh_terms_wg.h: the default where it applies since the records of 1-D rules and
// the merged cells - 1.28-1.35 ms on the bench mesh where pdh_rows.h takes 1.59-1.66, never slower on the other shapes tried,
// profiles/r04_wg_forms.txt.)  The cartesian description has no other kernel and ignores them.
KernelPlan plan_kernels(const pdh_problem *p, const Packed &K, const PlanSwitches &sw)
{
  KernelPlan P;
  RowsHost &RH = P.rows;
  FaceAnalysis A;
  if (p->dim != 3 || K.n1d < 2 || K.n1d > 4 || K.ghost)
    {
      P.why_rows = P.why_terms = K.ghost ? "exchange variant" : "not 3-D FE_DGQ / FE_AggloDGP of degree 1 .. 3";
      return P;
    }
  if (K.cart)
    { // planar axis-aligned faces and tensor rules hold by construction - and there are no host copies of the points to look at:
      // the kinds of pdh_rows.h, whose tables are made from the points, are not offered
      RH.planar_ok = true;
      RH.fq_tensor_n = K.cart->nqf;
      RH.fast_j.assign(3 * K.run_ap.size(), 0); // (the generator runs the lower tangential axis fastest)
      order_runs_of_slots(K, A);
      P.vq_n = K.cart->nq;
      P.why_rows = "cartesian description: the kinds of pdh_rows.h need the points";
    }
  else if (analyse_faces(p, K, RH, A, &P.why_rows) && build_rows_tables(p, K, A, sw, RH, &P.why_rows) &&
           rows_kind_applies(p, K, RH, P.vq_n, P.tensor_only, &P.why_rows))
    P.kernel = RowKernel::rows;
  const int terms_kind = pdht::terms_has_kind(K.n1d, p->basis == PDH_BASIS_AGGLODGP ? 1 : 0);
  if (!RH.planar_ok)
    P.why_terms = P.why_rows;
  else if (!K.cart && (sw.terms_off || (terms_kind == 2 && sw.terms_dgq3_off)))
    P.why_terms = "term kernel: switched off (PDH_TERMS / PDH_TERMS_DGQ3)";
  else
    {
      if (P.vq_n < 0 && RH.fq_tensor_n > 0)
        P.vq_n = resolve_volume_rules(p, K);
      if (build_terms_tables(p, K, RH, A, std::max(P.vq_n, 0), sw, P.terms, &P.why_terms))
        P.kernel = RowKernel::terms;
    }
  return P;
}

// the plan as pdh_set_problem makes it, but for PDH_TERMS / PDH_TERMS_DGQ3: the checks say what applies, not what was switched off
static int check_plan(const pdh_problem *p, int32_t row_begin, int32_t row_end, KernelPlan &plan)
{
  Packed K;
  g_err_noctx.clear();
  PDH_TRY(pack_problem(g_err_noctx, p, row_begin, row_end, K));
  PlanSwitches sw = read_plan_switches();
  sw.terms_off = sw.terms_dgq3_off = false;
  plan = plan_kernels(p, K, sw);
  return PDH_OK;
}

// Host-only: 1 if a row kernel (PDH_ALG_ROWS: pdh_rows.h or the term kernels) applies to this description and row range, 0 if not
// (pdh_last_error(NULL) says why), < 0 on an invalid description.
extern "C" int pdh_check_rows(const pdh_problem *p, int32_t row_begin, int32_t row_end)
{
  KernelPlan plan;
  PDH_TRY(check_plan(p, row_begin, row_end, plan));
  if (plan.kernel != RowKernel::none)
    return 1;
  g_err_noctx = plan.why_rows;
  if (plan.rows.planar_ok && plan.rows.fq_tensor_n > 0 && plan.vq_n > 0) // (the term kernels' own tests ran)
    g_err_noctx += "; " + plan.why_terms;
  return 0;
}

// Host-only: 1 if the term kernels (pdh_terms.h / pdh_terms_wg.h) apply to this description and row range, 0 if not
// (pdh_last_error(NULL) says why), < 0 on an invalid description.  stats5 (may be NULL; left alone where the faces are not unions
// of axis-aligned planes): most runs / sub-faces / interior sub-faces / cells of one owned polytope, LDS bytes of a workgroup.
extern "C" int pdh_check_terms(const pdh_problem *p, int32_t row_begin, int32_t row_end, int64_t *stats5)
{
  KernelPlan plan;
  PDH_TRY(check_plan(p, row_begin, row_end, plan));
  const TermsHost &TH = plan.terms;
  if (stats5 && plan.rows.planar_ok)
    {
      stats5[0] = TH.maxruns, stats5[1] = TH.maxsf, stats5[2] = TH.maxsi, stats5[3] = TH.maxcell, stats5[4] = TH.lds_bytes;
    }
  if (plan.kernel == RowKernel::terms)
    return 1;
  g_err_noctx = plan.why_terms;
  return 0;
}

// Host-only validation (no GPU needed): runs exactly the checks of pdh_set_problem.
extern "C" int pdh_check_problem(const pdh_problem *p, int32_t row_begin, int32_t row_end, int64_t *stats)
{
  Packed K;
  g_err_noctx.clear();
  const int rc = pack_problem(g_err_noctx, p, row_begin, row_end, K);
  if (rc == PDH_OK && stats)
    {
      stats[0] = (int64_t)K.n_owned;
      stats[1] = (int64_t)K.it_own.size();
      stats[2] = K.n_vq;
      stats[3] = K.n_ap;
      stats[4] = K.n_values;
      stats[5] = K.n;
      stats[6] = (int64_t)pdh::lds_bytes_diag(p->dim, K.n1d, K.NT);
      stats[7] = (int64_t)pdh::lds_bytes_offdiag(p->dim, K.n1d, K.NT);
    }
  return rc;
}

// Host-only: per-peer sizes of the ghost-block exchange of a description (what pdh_exchange_layout reports after
// pdh_set_problem_local in PDH_EXCHANGE_GHOST mode) - lets the multi-rank logic be checked on machines without a GPU.
extern "C" int pdh_check_exchange(const pdh_problem *p, int32_t row_begin, int32_t row_end, int n_ranks, int64_t *send_count,
                                  int64_t *recv_count)
{
  Packed K;
  g_err_noctx.clear();
  const int rc = pack_problem(g_err_noctx, p, row_begin, row_end, K, PDH_EXCHANGE_GHOST);
  if (rc != PDH_OK)
    return rc;
  if (n_ranks < (int)K.send_count.size() || !send_count || !recv_count)
    return fail(g_err_noctx, PDH_EINVAL, "n_ranks is smaller than the number of ranks in agg_rank, or an output is NULL");
  for (int r = 0; r < n_ranks; ++r)
    {
      send_count[r] = r < (int)K.send_count.size() ? K.send_count[r] : 0;
      recv_count[r] = r < (int)K.recv_count.size() ? K.recv_count[r] : 0;
    }
  return PDH_OK;
}

// Host-only: extreme eigenvalues of a symmetric tridiagonal matrix (the Lanczos matrix of pdh_setup_chebyshev's CG steps).  Bisection
// on the Sturm count of T - x I (number of negative pivots q_i = d_i - x - e_(i-1)^2 / q_(i-1) = number of eigenvalues below x),
// started from the Gershgorin interval and run until the interval holds no further double.
extern "C" int pdh_tridiagonal_eigenvalues(int k, const double *diag, const double *offdiag, double *lo, double *hi)
{
  g_err_noctx.clear();
  if (k < 1 || k > 256 || !diag || (k > 1 && !offdiag) || !lo || !hi)
    return fail(g_err_noctx, PDH_EINVAL, "pdh_tridiagonal_eigenvalues: 1 <= k <= 256, diag, offdiag (k > 1), lo and hi are required");
  double gl = diag[0], gu = diag[0], emax = 0.0;
  for (int i = 0; i < k; ++i)
    {
      const double el = i > 0 ? std::fabs(offdiag[i - 1]) : 0.0, er = i + 1 < k ? std::fabs(offdiag[i]) : 0.0;
      if (!std::isfinite(diag[i]) || !std::isfinite(el) || !std::isfinite(er))
        return fail(g_err_noctx, PDH_EINVAL, "pdh_tridiagonal_eigenvalues: entry " + std::to_string(i) + " is not finite");
      gl = std::min(gl, diag[i] - el - er);
      gu = std::max(gu, diag[i] + el + er);
      emax = std::max(emax, er);
    }
  if (k == 1)
    {
      *lo = *hi = diag[0];
      return PDH_OK;
    }
  const double norm = std::max(std::fabs(gl), std::fabs(gu));
  const double pivmin = std::max(2.2250738585072014e-308, 2.2250738585072014e-308 * emax * emax);
  const double pad = 2.0 * 2.220446049250313e-16 * norm * k + 2.0 * pivmin;
  gl -= pad;
  gu += pad;
  auto below = [&](double x) { // number of eigenvalues < x
    int c = 0;
    double q = diag[0] - x;
    if (std::fabs(q) < pivmin)
      q = -pivmin;
    c += q < 0.0;
    for (int i = 1; i < k; ++i)
      {
        q = diag[i] - x - offdiag[i - 1] * offdiag[i - 1] / q;
        if (std::fabs(q) < pivmin)
          q = -pivmin;
        c += q < 0.0;
      }
    return c;
  };
  auto kth = [&](int want) { // eigenvalue number `want` (0 = smallest): below(a) <= want < below(b) throughout
    double a = gl, b = gu;
    for (int it = 0; it < 2200; ++it)
      {
        const double m = a + 0.5 * (b - a);
        if (!(m > a && m < b))
          break;
        if (below(m) <= want)
          a = m;
        else
          b = m;
      }
    return a + 0.5 * (b - a);
  };
  *lo = kth(0);
  *hi = kth(k - 1);
  return PDH_OK;
}

void pdh_lanczos_tridiagonal(const std::vector<double> &alpha, const std::vector<double> &beta, std::vector<double> &diag,
                             std::vector<double> &offdiag)
{
  const int m = (int)alpha.size();
  diag.assign((size_t)m, 0.0);
  offdiag.assign((size_t)std::max(m - 1, 1), 0.0);
  for (int j = 0; j < m; ++j)
    {
      diag[j] = j == 0 ? 1.0 / alpha[j] : 1.0 / alpha[j] + beta[j - 1] / alpha[j - 1];
      if (j + 1 < m)
        offdiag[j] = std::sqrt(beta[j]) / alpha[j];
    }
}

void pdh_chebyshev_coefficients(int degree, double estimate, double smoothing_range, double *lambda_lo, double *lambda_hi,
                                std::vector<double> &c1, std::vector<double> &c2)
{
  const double hi = 1.2 * estimate, lo = hi / smoothing_range;
  const double theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta;
  c1.assign((size_t)degree, 0.0);
  c2.assign((size_t)degree, 0.0);
  c2[0] = 1 / theta;
  double rho_old = 1 / sigma;
  for (int k = 1; k < degree; ++k)
    {
      const double rho = 1 / (2 * sigma - rho_old);
      c1[k] = rho * rho_old;
      c2[k] = 2 * rho / delta;
      rho_old = rho;
    }
  *lambda_lo = lo;
  *lambda_hi = hi;
}
