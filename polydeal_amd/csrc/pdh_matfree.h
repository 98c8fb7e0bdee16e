// pdh_matfree.h — the SIP operator applied from the term tables instead of the stored values (3-D FE_DGQ(1..3), FE_AggloDGP(1..3) on
// agglomerates of Cartesian cells; C ABI: pdh_setup_matrix_free, pdh_matrix_free_vmult*, pdh_set_smoother_operator).
//
// Every block the term kernels write is a short sum of Kronecker products of three 1-D matrices per merged cell or sub-face
// (pdh_terms.h, header comment), and a Kronecker product is applied to a vector by sum factorisation: three passes of N1D multiply-adds
// per entry.  So with the 1-D matrices of a polytope resident in HBM - a few hundred doubles where its rows are a few tens of
// thousands - y = A x needs no stored value:
//   y_P = sum_cells     (K0' (x) M1 (x) M2 + M0 (x) K1 (x) M2 + M0 (x) M1 (x) K2) x_P
//       + sum_sub-faces (D0 (x) D1 (x) D2) x_P
//       + sum_interior runs r  sum_sub-faces of r  (X0 (x) X1 (x) X2) x_Q(r)
// k_mf_tables (set-up, once per problem): the lane tasks of phase A of the term kernels (pdht::TermTasks, unchanged) write the tables
//   of a polytope straight into its record (layout: pdht::matfree_rec_doubles); no table passes through LDS, so no polytope is too
//   large for it.  The one thing it hands them differently is the plane of a sub-face that lies on a box face (see there).
// k_mf_vmult: one wave per owned polytope, lane = entry (k0, k1, k2) of the full N1D^3 tensor.  FE_AggloDGP (k0 + k1 + k2 <= p) is
//   embedded with zeros and the rows of the set are kept.  A pass along axis d: the lane gathers the N1D entries of its line from
//   the other lanes (ds_bpermute: the LDS crossbar, no LDS memory) and forms one N1D-term sum with its row of the 1-D matrix; the
//   tables are staged from the record to LDS in chunks of a fixed size.  The gathered line of x along axis 2 serves every term of
//   the same x; the three cell terms share their passes (a = M2 x, b = K2 x, c = M1 a, d = K1 a + M1 b, y += K0' c + M0 d).
//   y is one register per lane, the terms are added in a fixed order, no atomics: the same call gives the same bits.
#pragma once
#include "pdh_solve.h"
#include "pdh_terms.h"

namespace pdht
{
// ---- set-up: the finished tables of every owned polytope into HBM -------------------------------------------------------------------
// PAIR: the records of 1-D rules have 8 slots per task (PdhTerms::tpm), worked on by pairs of lanes; else 4
template <int N1D, int BASIS, bool PAIR>
__global__ void __launch_bounds__(PDH_WAVE) k_mf_tables(const PdhDev P, const PdhTerms T, double *__restrict__ out, const int n_owned)
{
  constexpr int PL = 4, TS = PAIR ? 2 : 1, TPM = PL * TS; // slots per lane, lanes per task, slots per rule in the record
  using TT = TermTasks<N1D, BASIS, PL, PAIR>;
  const int lane = threadIdx.x, slot = blockIdx.x;
  if (slot >= n_owned)
    return;
  // header and run entries are read where they lie (TermTasks::rec: the record from its header on)
  const double *g = T.meta + (int64_t)slot * (TERMS_HDR + T.maxruns * TERMS_ENT);
  const long long h0 = __double_as_longlong(g[0]);
  const int ncell = (int)((h0 >> 16) & 0xffff), nsfb = (int)(h0 >> 32);
  const int nsf = (int)__double_as_longlong(g[11]);
  double *rec = out + (int64_t)slot * matfree_rec_doubles(N1D, T.maxsf, T.maxsi, T.maxcell);
  const double *gr = T.tdata + (int64_t)slot * T.tstride;
  const double *gr_info = gr + (2 * T.maxsf + 3 * T.maxcell) * (3 * TPM) + T.maxsf;
  double *Xa = rec, *Da = rec + matfree_off_d(N1D, T.maxsi), *Ca = rec + matfree_off_c(N1D, T.maxsf, T.maxsi);
  const TT tt{P, g, Xa, Da, Ca, g[1], g[2], g[3], g[4], g[5], g[6], nsfb, T.fq_tensor_n, T.vq_tensor_n, gr, T.maxsf, T.maxcell};
  // lane tasks as in k_terms: (sub-face, tangential direction[, half]); the normal-direction tasks, then - from an even lane on,
  // pairs must be neighbours - (cell, direction[, half])
  const int n1 = 2 * nsf * TS, ncs = PAIR ? (nsf + 1) & ~1 : nsf, n2 = ncs + 3 * ncell * TS;
  for (int tid = lane; tid < n1; tid += PDH_WAVE)
    {
      const int task = tid / TS, half = tid - task * TS, sf = task >> 1, dir = task & 1;
      const int info = (int)__double_as_longlong(gr_info[sf]);
      tt.tang_compute(tt.tang_load(info, sf, dir, half), sf, dir, info, half);
    }
  // The record carries the plane coordinate of a sub-face as ONE face point of the description has it, and a caller's mapped points
  // carry it with an ulp or two of rounding (|x| eps, far from the origin many times eps of the box).  Where the plane is a face of
  // the box, nodal bases are exactly 0 or 1 there and the penalty table sigma B_k B_l has exact zeros: the rounding of the coordinate
  // would put sigma B'_k |x| eps / h into them.  A plane within 1e-10 of the box side of a face of the own box, or of the lower face of
  // the neighbour's, IS that face - no cell is thinner - and the boxes are the description's own numbers: take theirs.
  const double *own_hi = P.bbox + ((int64_t)P.own_agg[slot] * 2 + 1) * 3;
  auto plane = [&](int sf, int info) {
    const double z = tt.zeta_load(sf);
    const int c = (info >> 8) & 3;
    const double *re = g + TERMS_HDR + (info & 0xff) * TERMS_ENT;
    const double lo = g[1 + c], hi = own_hi[c], tol = 1e-10 / g[4 + c];
    if (fabs(z - lo) <= tol)
      return lo;
    if (fabs(z - hi) <= tol)
      return hi;
    const bool interior = (int)__double_as_longlong(re[1]) >= 0;
    return interior && fabs(z - re[3 + c]) <= tol ? re[3 + c] : z;
  };
  for (int tid = lane; tid < n2; tid += PDH_WAVE)
    {
      if (tid < nsf)
        {
          const int info = (int)__double_as_longlong(gr_info[tid]);
          tt.norm_compute(plane(tid, info), tid, info);
        }
      else if (tid >= ncs)
        {
          const int ct = (tid - ncs) / TS, half = (tid - ncs) - ct * TS;
          tt.cell_compute(tt.cell_load(ct, half), ct, half);
        }
    }
}

// ---- the product ------------------------------------------------------------------------------------------------------------------------
// tables of one staged chunk, doubles: 8 coupling terms (24 full 1-D matrices) - 3.3 KB for N1D = 4, whatever the problem's maxima
template <int N1D>
constexpr int MF_CHUNK = 8 * 3 * ((N1D * N1D) | 1);

template <int N1D, int BASIS>
__global__ void __launch_bounds__(PDH_WAVE) k_mf_vmult(const PdhSolveArgs A, const PdhTerms T, const double *__restrict__ tables,
                                                        const double *__restrict__ x, double *__restrict__ y, double *__restrict__ part)
{
  using K = Kind<N1D, BASIS>;
  constexpr int N = N1D, NT = N * N * N, NF = K::NF, SYMS = K::SYMS, FULLS = K::FULLS, CH = MF_CHUNK<N1D>;
  constexpr int XCH = CH / (3 * FULLS), DCH = CH / (3 * SYMS), CCH = CH / (6 * SYMS); // terms per chunk: coupling, sub-face, cell
  __shared__ double tab[CH];
  const int lane = threadIdx.x, s = blockIdx.x;
  // ---- the lane's entry of the tensor and its row R of the element (in_set: the entry belongs to the index set)
  const int tl = lane < NT ? lane : 0; // (lanes behind the tensor follow entry 0 and store nothing)
  const int k0 = tl % N, k1 = (tl / N) % N, k2 = tl / (N * N);
  bool in_set = lane < NT;
  int R = tl;
  if constexpr (BASIS != 0)
    { // Kind::dig: x fastest over k0 + k1 + k2 < N1D
      in_set = in_set && k0 + k1 + k2 < N;
      R = k0;
      for (int iz = 0; iz < k2; ++iz)
        R += (N - iz) * (N - iz + 1) / 2;
      for (int iy = 0; iy < k1; ++iy)
        R += N - iy - k2;
    }
  const int b0 = tl - k0, b1 = tl - k1 * N, b2 = tl - k2 * N * N; // first lane of the lane's line along every axis
  int o0[N], o1[N], o2[N];                                        // packed positions of row k_d of a symmetric table
  for (int l = 0; l < N; ++l)
    o0[l] = K::sym(k0, l), o1[l] = K::sym(k1, l), o2[l] = K::sym(k2, l);
  // ---- header of the polytope (uniform addresses: scalar loads)
  const double *g = T.meta + (int64_t)s * (TERMS_HDR + T.maxruns * TERMS_ENT);
  const long long h0 = __double_as_longlong(g[0]);
  const int nruns = (int)(h0 & 0xffff), ncell = (int)((h0 >> 16) & 0xffff), nsfb = (int)(h0 >> 32);
  const int nsf = (int)__double_as_longlong(g[11]);
  const int m0 = A.diag_L[s] / NF;        // place of the own block among the row's blocks
  const int first_int = nsfb > 0 ? 1 : 0; // the boundary run, if any, is run 0
  const int64_t blk0 = A.blk_ptr[s];
  const double *rec = tables + (int64_t)s * matfree_rec_doubles(N1D, T.maxsf, T.maxsi, T.maxcell);
  // x of block t of the row, embedded in the tensor
  auto load_x = [&](int t) { return in_set ? x[(int64_t)A.blk_dof[blk0 + t] + R] : 0.0; };
  // the entries of v along the lane's line: g[l] = v of the lane at first + l * stride
  auto line = [&](double v, int first, int stride, double(&gl)[N]) {
    static_for<0, N>([&](auto l_) { gl[l_] = __shfl(v, first + l_ * stride, PDH_WAVE); });
  };
  auto dot_sym = [&](const double *m, const int(&o)[N], const double(&gl)[N]) {
    double v = 0.0;
    static_for<0, N>([&](auto l_) { v += m[o[l_]] * gl[l_]; });
    return v;
  };
  auto dot_full = [&](const double *m, int k, const double(&gl)[N]) { // entry (k, l) at l * N1D + k
    double v = 0.0;
    static_for<0, N>([&](auto l_) { v += m[l_ * N + k] * gl[l_]; });
    return v;
  };
  // `count` doubles of the record from `src` on into LDS (the reads of the chunk before are issued: one wave, in order)
  auto stage = [&](const double *src, int count) {
    PDH_WAVE_SYNC();
    for (int i = lane; i < count; i += PDH_WAVE)
      tab[i] = src[i];
    PDH_WAVE_SYNC();
  };
  const double xp = load_x(m0);
  double xl[N], gl[N], hl[N];
  line(xp, b2, N * N, xl);
  double yv = 0.0;
  // ---- cells: M | K per axis
  for (int c0 = 0; c0 < ncell; c0 += CCH)
    {
      const int c1 = c0 + CCH < ncell ? c0 + CCH : ncell;
      stage(rec + matfree_off_c(N1D, T.maxsf, T.maxsi) + c0 * 6 * SYMS, (c1 - c0) * 6 * SYMS);
      for (int u = 0; u < c1 - c0; ++u)
        {
          const double *m = tab + u * 6 * SYMS;
          const double a = dot_sym(m + 4 * SYMS, o2, xl), b = dot_sym(m + 5 * SYMS, o2, xl);
          line(a, b1, N, gl);
          line(b, b1, N, hl);
          const double c = dot_sym(m + 2 * SYMS, o1, gl), d = dot_sym(m + 3 * SYMS, o1, gl) + dot_sym(m + 2 * SYMS, o1, hl);
          line(c, b0, 1, gl);
          line(d, b0, 1, hl);
          yv += dot_sym(m + SYMS, o0, gl) + dot_sym(m, o0, hl);
        }
    }
  // ---- sub-faces, own side
  for (int c0 = 0; c0 < nsf; c0 += DCH)
    {
      const int c1 = c0 + DCH < nsf ? c0 + DCH : nsf;
      stage(rec + matfree_off_d(N1D, T.maxsi) + c0 * 3 * SYMS, (c1 - c0) * 3 * SYMS);
      for (int u = 0; u < c1 - c0; ++u)
        {
          const double *m = tab + u * 3 * SYMS;
          line(dot_sym(m + 2 * SYMS, o2, xl), b1, N, gl);
          line(dot_sym(m + SYMS, o1, gl), b0, 1, hl);
          yv += dot_sym(m, o0, hl);
        }
    }
  // ---- coupling: the interior sub-faces' tables stand run by run; interior run ri is block ri of the row, behind the own block ri + 1
  const int nsi = nsf - nsfb;
  for (int c0 = 0; c0 < nsi; c0 += XCH)
    {
      const int c1 = c0 + XCH < nsi ? c0 + XCH : nsi;
      stage(rec + c0 * 3 * FULLS, (c1 - c0) * 3 * FULLS);
      for (int ri = 0; ri + first_int < nruns; ++ri)
        {
          const long long e0 = __double_as_longlong(g[TERMS_HDR + (first_int + ri) * TERMS_ENT]);
          const int f = (int)(uint32_t)e0 - nsfb, ns = (int)(e0 >> 32);
          const int lo = f > c0 ? f : c0, hi = f + ns < c1 ? f + ns : c1;
          if (lo >= hi)
            continue;
          double ql[N];
          line(load_x(ri < m0 ? ri : ri + 1), b2, N * N, ql);
          for (int i = lo; i < hi; ++i)
            {
              const double *m = tab + (i - c0) * 3 * FULLS;
              line(dot_full(m + 2 * FULLS, k2, ql), b1, N, gl);
              line(dot_full(m + FULLS, k1, gl), b0, 1, hl);
              yv += dot_full(m, k0, hl);
            }
        }
    }
  if (in_set)
    y[A.own_row[s] + R] = yv;
  if (part)
    { // the slot's sum_i y_i x_i, added by the butterfly of pdh_solve.hip
      double acc = in_set ? yv * xp : 0.0;
      for (int mk = PDH_WAVE / 2; mk > 0; mk >>= 1)
        acc += __shfl_xor(acc, mk, PDH_WAVE);
      if (lane == 0)
        part[s] = acc;
    }
}
} // namespace pdht
