// pdh_terms_wg.h — FE_DGQ(3) (n = 64) on agglomerates of Cartesian cells with tensor rules: a whole CU on ONE polytope at a time.
//
// Same sums as pdh_rows.h / pdh_terms.h (reference include/poly_utils.h:2040-2084, 1870-1926), same owner-computes-rows formulation,
// same stores (whole aligned 512-byte pieces of a row through one buffer resource per polytope) - what changes is who works on a
// polytope.  The launch writes 7.3 GB and reads 0.1 GB on the bench mesh; what its stores reach depends on how many waves of a CU
// fill the SAME polytope's region and on the ORDER in which the device takes the polytopes (tools/probes/rows_store_probe.hip,
// profiles/r13_probe_team.txt): eight waves that are the only writers of their CU, polytopes handed out one by one by a device-wide
// counter: 1.15 ms (6.5 TB/s); four waves a polytope, four such workgroups per CU (the form before this one): 1.28; eight waves alone
// on their CU but each workgroup on a FIXED share of the polytopes, consecutive or interleaved: 1.31-1.40 - the CUs drift apart and the
// window of regions the device writes at a time is no longer dense.  So:
//   - one workgroup per CU (by its LDS request: the resolver of pdh_terms.hip checks it) of W WRITER waves and 4 BUILDER waves;
//   - the workgroup's first two polytopes are blockIdx.x and blockIdx.x + gridDim.x, the following come from PdhTerms::sched[0] (one
//     returning atomic add per polytope, by a builder lane, two polytopes ahead of its use; the ring `seq` in LDS passes them on).  The
//     workgroup that leaves last (sched[1] counts leavers) puts both words back to zero - launches of a context are stream-ordered;
//   - two table buffers in LDS, each laid out as the planner sized it (rec | digits | Xa | Da | Ca, PdhTerms::lds_bytes);
//   - step k: the writers compute and store polytope k from buffer k & 1 while the builders make the tables of polytope k + 1 in buffer
//     (k + 1) & 1, whose data they requested a step earlier, and request the data of polytope k + 2.  ONE __syncthreads() ends the step:
//     the writers last read buffer (k + 1) & 1 in step k - 1, before its barrier.  Every wave passes (polytopes of the workgroup) + 1
//     barriers.  Loads and stores are separated BY WAVE: a writer makes no load from global memory (vmcnt retires in issue order - a load
//     behind a burst of row stores waits for all of them), a builder no store;
//   - the row stores are sc1|nt, and a writer waits for its own (vmcnt(0)) before the step's barrier: against nt stores left in flight
//     over the barrier, timed in turn on the SAME resident problem (tools/paired_bench.py), -2.6 % to -3.3 % on each of eight contexts
//     with the baseline 0.2 % apart from itself, and -1.5 % to -5 % from an eighth of the bench mesh to its grown agglomerates
//     (profiles/r14_paired_variants.txt).  The ORDER of a wave's stores (its 8 rows of one piece, 3.5 KB apart, then the next piece) was
//     set against whole rows in ascending address order in the store-only twin and is not what holds the stream back: row-major is 2-3 %
//     slower than piece-major at their better policies (profiles/r14_probe_row_major.txt).
// Builders (phase A: the lane tasks of pdh_terms.h, TermTasks): waves 0, 1 the (sub-face, tangential direction[, half]) tasks in
// alternating chunks of 64, wave 2 the normal-direction tasks, wave 3 the (cell, direction[, half]) tasks - a lane's task, and with it
// every address of a request, depends on the slot alone, so a request waits for nothing, not even the header (one round trip to HBM).
// Every builder wave copies the record (header | run entries) into the buffer itself (the same values to the same places; the entries a
// wave reads are its own copy, ordered by the LDS unit): the writers take rbase, row length, L and the counts from the header there.
// A builder's load INSTRUCTION takes its turn among the writers' stores in the CU's memory pipeline (about 540 cycles each, stamps in
// profiles/r13_wg_team_stamps.txt), so a request is few instructions: the record in two pieces per lane, the task's points in 16-byte
// loads, the first-point weights by a lane exchange; the ticket is drawn by the wave with the least to do, and the builders run at
// priority 3.  With that the last writer waits 2-3 % of a step at the barrier and the builders idle for half of it.
// Writers (phase B): wave w owns rows [64 w / W, 64 (w + 1) / W) of every block: lane = column.  A value is a short sum of products of
// three 1-D matrix entries (pdh_terms.h), so a wave accumulates its 64 / W rows of a block in registers straight from the LDS tables -
// no moments, no contraction stages, no MFMA - and stores each row piece as 512 contiguous bytes.  Diagonal-first rows: piece m <= m0
// holds [carry | columns 0 .. 62]: lane l computes column l - 1 (its own table offsets), lane 0 the last column of the block before
// (another run's tables) or, in piece 0, receives the diagonal entry; the own block is computed in natural order and stored with lanes
// 0 .. R rotated by one position (lane R, whose diagonal entry belongs to position 0 of the ROW, carries the last column of the block
// before).
// The planner's DEFAULT for FE_DGQ(3) wherever the term tables can be built (plan_kernels in pdh_plan.cpp; PDH_TERMS_DGQ3=0 or
// PDH_TERMS=0 keeps pdh_rows.h).  W = 8 by default, PDH_TERMS_WG_WAVES=4: four writers of 16 rows each.  Against the form before (four
// waves a polytope, four workgroups per CU) in one process, four runs: medians 1.21-1.31 against 1.32-1.37 ms (-3 % to -12 %), the
// per-context ranges OVERLAPPING in every run - a shift of the median, not a gain by the rule "slowest new context below the fastest old
// one"; 5 % slower at 32 polytopes per CU (profiles/r13_wg_team_ab.txt).  168 VGPRs, no scratch with 4-slot rules, 24 bytes with 8-slot rules.
#pragma once
#include "pdh_terms.h"

// -DPDHT_STAMP (diagnostic builds): cycle counter -> stamps[slot][..]: the first writer wave at 0 .. 2, the last at 3 .. 5 (start of the
// step, last store issued - and, where the writers drain, retired -, barrier left: 2 - 1 is the wait at the barrier alone); the first builder wave at 6 .. 8, the last at 9 .. 11 (loads of the NEXT polytope issued, tables
// of this one done, barrier left)
#ifdef PDHT_STAMP
#define PDHW_MARK(s, base, k)                                                                                         \
  do                                                                                                                  \
    {                                                                                                                 \
      const long long tm_ = (long long)__builtin_readcyclecounter();                                                  \
      if ((base) >= 0 && lane == 0 && T.stamps)                                                                       \
        T.stamps[(int64_t)(s) * 16 + (base) + (k)] = tm_;                                                              \
    }                                                                                                                 \
  while (0)
#else
#define PDHW_MARK(s, base, k)
#endif

namespace pdht
{
constexpr int WG_BUILDERS = 4; // builder waves of a workgroup
constexpr int WG_TICKET = 2;   // the one that draws the tickets (normal-direction tasks: the least loads and arithmetic)

// The kernel's body.  AUX: cache-policy bits of the row stores (gfx940+: 1 = sc0, 2 = nt, 16 = sc1); DRAIN: a writer waits for its
// stores (vmcnt(0)) before the barrier that ends a step.  k_terms_wg below is the body with the defaults of pdh_terms_tables.h (sc1|nt,
// drained) and all the library instantiates; -DPDHT_VARIANTS builds add k_terms_wg_base, the policy before (nt, in flight), and
// tools/paired_bench.py times the two in turn on one resident problem.  (The policy is an argument of the body, not of the kernels: a
// kernel's symbol keeps its three arguments, by which tools/device_code_diff.py and tests/test_isa_lint.py find the instantiations.)
template <int W, bool SHIFTED, int PMAX, int AUX, bool DRAIN>
__device__ __forceinline__ void terms_wg(const PdhDev &P, const PdhTerms &T, const int n_owned)
{
  constexpr int N1D = 4, BASIS = 0;
  using K = Kind<N1D, BASIS>;
  constexpr int NF = K::NF, SYMS = K::SYMS, FULLS = K::FULLS;
  constexpr int RPW = 64 / W, NK1 = RPW / 4; // rows per writer wave; values of k1 among them (k2 is fixed per wave)
  static_assert(NF == 64 && (W == 4 || W == 8), "FE_DGQ(3), four or eight writer waves");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int seq[4]; // seq[i & 3]: the workgroup's i-th polytope, i >= 2 (>= n_owned: there is none)
  const int lane = threadIdx.x & (PDH_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s0 = blockIdx.x, s1 = s0 + (int)gridDim.x;
  const int NENT = T.maxruns * TERMS_ENT, REC = TERMS_HDR + NENT;
  const int stride = T.lds_bytes >> 3; // doubles of one table buffer
  const int XA_OFF = terms_rec_doubles(T.maxruns) + ((NF + 1) / 2 + ((NF + 1) / 2 & 1));
  const int DA_OFF = XA_OFF + (T.maxsi * 3 * FULLS + ((T.maxsi * 3 * FULLS) & 1));
  // entry i of a record header held one entry per lane (uniform)
  auto hdr = [](double hv, int i) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(hv), i), __builtin_amdgcn_readlane(__double2loint(hv), i));
  };
  // PMAX = slots per 1-D rule in the records (PdhTerms::tpm); rules of more than four slots are worked on by pairs of lanes (TermTasks)
  constexpr bool PAIR = PMAX > 4;
  constexpr int PL = PAIR ? PMAX / 2 : PMAX, TS = PAIR ? 2 : 1; // slots per lane, lanes per task
  using TT = TermTasks<N1D, BASIS, PL, PAIR>;

  if (wave >= W)
    {
      // ================= builders ====================================================================================
      const int bw = wave - W;
      __builtin_amdgcn_s_setprio(3); // (a step is as long as its slower side: the builders' short chains go first on their SIMD)
#ifdef PDHT_STAMP
      const int sbase = bw == 0 ? 6 : (bw == WG_BUILDERS - 1 ? 9 : -1);
#endif
      // the lane's task of the first round, from the slot-independent numbering (later rounds: + 128 / + 64, loaded when they are worked on)
      const int tid0 = (bw < 2 ? bw * PDH_WAVE : 0) + lane;
      const int task0 = tid0 / TS, half0 = tid0 - task0 * TS;
      const int sf0 = bw < 2 ? task0 >> 1 : tid0, dir0 = task0 & 1; // (bw 3: task0 = (cell, direction))
      const int sf0c = sf0 < T.maxsf ? sf0 : 0, ct0c = task0 < 3 * T.maxcell ? task0 : 0;
      const int info_off = (2 * T.maxsf + 3 * T.maxcell) * (3 * PMAX) + T.maxsf;
      constexpr int NC = 2; // (records of up to 11 runs; the rest is copied when the tables are built)
      struct Req // what a lane holds of a polytope between request and use
      {
        typename TT::Pts p; // bw 0, 1: the tangential task; bw 3: the cell task; bw 2: x[0] = plane coordinate
        int info;           // descriptor of the task's sub-face
        double c[NC];       // entries lane + 64 i of the record (header | run entries); c[0] holds the header
      };
      auto request = [&](int s) __attribute__((always_inline)) {
        Req r;
        const int sc = s < n_owned ? s : n_owned - 1; // (behind the last polytope: a request nobody uses)
        const double *g = T.meta + (int64_t)sc * REC;
        const double *gr = T.tdata + (int64_t)sc * T.tstride;
        static_for<0, NC>([&](auto i_) {
          const int k = lane + PDH_WAVE * i_;
          r.c[i_] = 0.0;
          if (PDH_WAVE * i_ < REC) // (uniform: a load instruction of a builder takes its turn among the writers' stores)
            r.c[i_] = g[k < REC ? k : 0];
        });
        r.info = reinterpret_cast<const int *>(gr + info_off + sf0c)[0]; // (low half of the integer bits stored as a double)
        if (bw < 2)
          r.p = TT::template task_request<true>(gr + (2 * sf0c + dir0) * (3 * PMAX), half0);
        else if (bw == 3)
          r.p = TT::template task_request<false>(gr + (2 * T.maxsf + ct0c) * (3 * PMAX), half0);
        else
          {
            r.p = typename TT::Pts{};
            r.p.x[0] = gr[(2 * T.maxsf + 3 * T.maxcell) * (3 * PMAX) + sf0c];
          }
        return r;
      };
      auto build = [&](const Req &r, int s, double *buf) __attribute__((always_inline)) {
        double *rec = buf, *Xa = buf + XA_OFF, *Da = buf + DA_OFF;
        const double hv = r.c[0];
        const long long h0 = __double_as_longlong(hdr(hv, 0));
        const int ncell = (int)((h0 >> 16) & 0xffff), nsfb = (int)(h0 >> 32);
        const int nsf = (int)__double_as_longlong(hdr(hv, 11));
        const double lo0 = hdr(hv, 1), lo1 = hdr(hv, 2), lo2 = hdr(hv, 3);
        const double ih0 = hdr(hv, 4), ih1 = hdr(hv, 5), ih2 = hdr(hv, 6);
        const int fn = T.fq_tensor_n, tn = T.vq_tensor_n;
        const double *g = T.meta + (int64_t)s * REC;
        const double *gr = T.tdata + (int64_t)s * T.tstride;
        double *Ca = Da + nsf * 3 * SYMS;
        // header and run entries (this wave's own copy)
        static_for<0, NC>([&](auto i_) {
          const int k = lane + PDH_WAVE * i_;
          if (k < REC)
            rec[k] = r.c[i_];
        });
        for (int k = NC * PDH_WAVE + lane; k < REC; k += PDH_WAVE)
          rec[k] = g[k];
        PDH_WAVE_SYNC();
        const TT tt{P, rec, Xa, Da, Ca, lo0, lo1, lo2, ih0, ih1, ih2, nsfb, fn, tn, gr, T.maxsf, T.maxcell};
        auto desc = [&](int sf) { return (int)__double_as_longlong(gr[info_off + (sf < T.maxsf ? sf : 0)]); };
        const int info0 = r.info;
        typename TT::Pts p = r.p;
        TT::task_first_weights(p);
        if (bw < 2)
          {
            const int n1 = 2 * nsf * TS;
            if (tid0 < n1)
              {
                p.npts = TT::tang_npts(info0, dir0, fn, half0);
                tt.tang_compute(p, sf0, dir0, info0, half0);
              }
            for (int tid = tid0 + 2 * PDH_WAVE; tid < n1; tid += 2 * PDH_WAVE)
              {
                const int task = tid / TS, half = tid - task * TS, sf = task >> 1, dir = task & 1;
                const int info = desc(sf);
                const typename TT::TPts tp = tt.tang_load(info, sf, dir, half);
                tt.tang_compute(tp, sf, dir, info, half);
              }
          }
        else if (bw == 2)
          {
            if (tid0 < nsf)
              tt.norm_compute(r.p.x[0], tid0, info0);
            for (int tid = tid0 + PDH_WAVE; tid < nsf; tid += PDH_WAVE)
              tt.norm_compute(tt.zeta_load(tid), tid, desc(tid));
          }
        else
          {
            const int n3 = 3 * ncell * TS;
            if (tid0 < n3)
              {
                p.npts = TT::cell_npts(p);
                tt.cell_compute(p, task0, half0);
              }
            for (int tid = tid0 + PDH_WAVE; tid < n3; tid += PDH_WAVE)
              {
                const int ct = tid / TS, half = tid - ct * TS;
                const typename TT::CPts cp = tt.cell_load(ct, half);
                tt.cell_compute(cp, ct, half);
              }
          }
      };
      int s_cur = s0, s_nxt = s1;
      Req rq = request(s_cur);
      for (int j = 0;; ++j)
        {
          // s_cur, s_nxt: polytopes j and j + 1 of the workgroup.  Ask for polytope j + 2, request the data of j + 1, build j
          const bool fetch = bw == WG_TICKET && s_nxt < n_owned;
          unsigned tick = 0;
          if (fetch && lane == 0)
            tick = __hip_atomic_fetch_add(T.sched, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const Req rn = request(s_nxt);
          PDHW_MARK(s_cur < n_owned ? s_cur : 0, s_cur < n_owned ? sbase : -1, 0);
          if (s_cur < n_owned)
            build(rq, s_cur, lds + (j & 1) * stride);
          if (bw == WG_TICKET && lane == 0)
            seq[(j + 2) & 3] = fetch ? 2 * (int)gridDim.x + (int)tick : n_owned;
          PDHW_MARK(s_cur < n_owned ? s_cur : 0, s_cur < n_owned ? sbase : -1, 1);
          __syncthreads();
          PDHW_MARK(s_cur < n_owned ? s_cur : 0, s_cur < n_owned ? sbase : -1, 2);
          if (s_cur >= n_owned)
            break;
          s_cur = s_nxt;
          rq = rn;
          s_nxt = __builtin_amdgcn_readfirstlane(seq[(j + 2) & 3]);
        }
      // (the workgroup has made its last request to sched[0] before it counts itself out: the last one out may reset both)
      if (bw == WG_TICKET && lane == 0)
        if (__hip_atomic_fetch_add(T.sched + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1)
          {
            __hip_atomic_store(T.sched, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(T.sched + 1, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          }
      return;
    }

  // ================= writers: this wave's rows of every block ==========================================================
#ifdef PDHT_STAMP
  const int sbase = wave == 0 ? 0 : (wave == W - 1 ? 3 : -1);
#endif
  const int R0 = RPW * wave;                      // first row of the wave
  const int k2 = RPW == 16 ? wave : wave >> 1;    // third digit of all its rows
  const int K1B = RPW == 16 ? 0 : 2 * (wave & 1); // first value of the second digit (NK1 values)
  // rows r = k0 + 4 i (i-th value of k1):  acc[r] += f0[k0] * (f1[i] * f2)
  auto add_term = [&](double (&acc)[RPW], const double (&f0)[4], const double (&f1)[NK1], double f2) __attribute__((always_inline)) {
    double yz[NK1];
    static_for<0, NK1>([&](auto i_) { yz[i_] = f1[i_] * f2; });
    static_for<0, RPW>([&](auto r_) {
      constexpr int r = r_;
      acc[r] += f0[r & 3] * yz[r >> 2];
    });
  };
  int s = s0;
  __syncthreads(); // the tables of the workgroup's first polytope
  for (int step = 0;; ++step)
    {
      if (step > 0)
        s = step == 1 ? s1 : __builtin_amdgcn_readfirstlane(seq[step & 3]);
      if (s >= n_owned)
        break;
      PDHW_MARK(s, sbase, 0);
      const double *rec = lds + (step & 1) * stride, *Xa = rec + XA_OFF, *Da = rec + DA_OFF;
      const double hv = rec[lane < TERMS_HDR ? lane : 0];
      const long long h0 = __double_as_longlong(hdr(hv, 0));
      const int ncell = (int)((h0 >> 16) & 0xffff), nsfb = (int)(h0 >> 32);
      const int nsf = (int)__double_as_longlong(hdr(hv, 11));
      const int64_t rbase = __double_as_longlong(hdr(hv, 7));
      const int rlen = (int)__double_as_longlong(hdr(hv, 8));
      const int L = (int)__double_as_longlong(hdr(hv, 9));
      const double *Ca = Da + nsf * 3 * SYMS;
      const int m0 = L >> 6, nblk = rlen >> 6;
      const int first_int = nsfb > 0 ? 1 : 0; // the boundary run, if any, is run 0
      const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(P.values + rbase, 0, NF * rlen * 8, 0x00020000);
      auto row_store = [&](double v, uint32_t lane_bytes, uint32_t row_bytes) {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2_t, v), vrs, (int)lane_bytes, (int)row_bytes, AUX);
      };
      const uint32_t row0_bytes = (uint32_t)R0 * (uint32_t)rlen * 8u, rstep = (uint32_t)rlen * 8u;
      // coupling column `col` (0 .. 63) of the block of interior run `fl` (ascending block order without the own block), per lane
      // (always inlined: called from three places, and an out-of-line call would put the accumulators into scratch memory)
      auto coupling = [&](double (&acc)[RPW], int fl, int col, bool on) __attribute__((always_inline)) {
        const long long e0 = __double_as_longlong(rec[TERMS_HDR + (first_int + fl) * TERMS_ENT]);
        const int ns = on ? (int)(e0 >> 32) : 0;
        const double *xb = Xa + ((int)(uint32_t)e0 - nsfb) * 3 * FULLS;
        const int q0 = (col & 3) * 4, q1 = ((col >> 2) & 3) * 4 + FULLS + K1B, q2 = (col >> 4) * 4 + 2 * FULLS + k2;
        for (int st = 0; __any(st < ns); ++st)
          {
            if (st < ns)
              {
                double f0[4], f1[NK1];
                for (int k = 0; k < 4; ++k)
                  f0[k] = xb[q0 + k];
                for (int i = 0; i < NK1; ++i)
                  f1[i] = xb[q1 + i];
                add_term(acc, f0, f1, xb[q2]);
              }
            xb += 3 * FULLS;
          }
      };
      // ---- the own block, natural order (lane = column)
      double own[RPW];
      static_for<0, RPW>([&](auto r_) { own[r_] = 0.0; });
      {
        const int l0 = lane & 3, l1 = (lane >> 2) & 3, l2 = lane >> 4;
        int o0[4], o1[NK1];
        for (int k = 0; k < 4; ++k)
          o0[k] = K::sym(k, l0);
        for (int i = 0; i < NK1; ++i)
          o1[i] = K::sym(K1B + i, l1) + SYMS;
        const int o2 = K::sym(k2, l2) + 2 * SYMS;
        for (int u = 0; u < ncell; ++u)
          { // (K0' M1 M2 + M0 (K1 M2 + M1 K2))[k, l]
            const double *b = Ca + u * 6 * SYMS;
            double M0[4], K0[4], mm[NK1], km[NK1];
            const double M2 = b[o2 + 2 * SYMS], K2 = b[o2 + 3 * SYMS];
            for (int k = 0; k < 4; ++k)
              M0[k] = b[o0[k]], K0[k] = b[o0[k] + SYMS];
            for (int i = 0; i < NK1; ++i)
              {
                const double M1 = b[o1[i] + SYMS], K1 = b[o1[i] + 2 * SYMS];
                mm[i] = M1 * M2;
                km[i] = K1 * M2 + M1 * K2;
              }
            static_for<0, RPW>([&](auto r_) {
              constexpr int r = r_;
              own[r] += K0[r & 3] * mm[r >> 2] + M0[r & 3] * km[r >> 2];
            });
          }
        for (int u = 0; u < nsf; ++u)
          { // (D0 D1 D2)[k, l]
            const double *b = Da + u * 3 * SYMS;
            double f0[4], f1[NK1];
            for (int k = 0; k < 4; ++k)
              f0[k] = b[o0[k]];
            for (int i = 0; i < NK1; ++i)
              f1[i] = b[o1[i]];
            add_term(own, f0, f1, b[o2]);
          }
      }
      if constexpr (!SHIFTED)
        {
          // ascending rows: every piece is a block, the own block among them
          for (int b = 0; b < nblk; ++b)
            {
              double acc[RPW];
              if (b == m0)
                static_for<0, RPW>([&](auto r_) { acc[r_] = own[r_]; });
              else
                {
                  static_for<0, RPW>([&](auto r_) { acc[r_] = 0.0; });
                  coupling(acc, b < m0 ? b : b - 1, lane, true);
                }
              uint32_t rowrun = row0_bytes + (uint32_t)b * 512u;
              static_for<0, RPW>([&](auto r_) {
                row_store(acc[r_], (uint32_t)lane * 8u, rowrun);
                rowrun += rstep;
              });
            }
        }
      else
        {
          // ---- the own block's piece m0: lanes 0 .. R rotated by one position; lane R stores position 0 of the piece - the diagonal
          // entry itself if the own block is the first of the row, else the last column of the block before, which every lane
          // computes for the wave's rows (one column: the terms of that run once)
          double dg[RPW]; // diagonal entries of the wave's rows (uniform), for position 0 of piece 0
          {
            double left63[RPW];
            static_for<0, RPW>([&](auto r_) { left63[r_] = 0.0; });
            if (m0 > 0)
              coupling(left63, m0 - 1, 63, true);
            uint32_t rowrun = row0_bytes + (uint32_t)m0 * 512u;
            static_for<0, RPW>([&](auto r_) {
              constexpr int r = r_;
              const int R = R0 + r; // uniform
              dg[r] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(own[r]), R), __builtin_amdgcn_readlane(__double2loint(own[r]), R));
              const bool diag = lane == R;
              // (an opaque copy: `c ? a[r] : b[r]` of two register arrays is turned into ONE load from a selected address, which
              // puts both arrays into scratch memory)
              double lv = left63[r];
              asm volatile("" : "+v"(lv));
              const double v = (diag && m0 > 0) ? lv : own[r];
              const uint32_t off = diag ? 0u : (lane < R ? (uint32_t)(lane + 1) * 8u : (uint32_t)lane * 8u);
              row_store(v, off, rowrun);
              rowrun += rstep;
            });
          }
          // ---- pieces left of the own block: [carry | columns 0 .. 62 of block m]
          for (int m = 0; m < m0; ++m)
            {
              double acc[RPW];
              static_for<0, RPW>([&](auto r_) { acc[r_] = 0.0; });
              const bool l0_ = lane == 0;
              // lane 0: last column of block m - 1 (piece 0: the diagonal entry, set below); the others: column lane - 1 of block m
              coupling(acc, l0_ ? (m > 0 ? m - 1 : 0) : m, l0_ ? 63 : lane - 1, !(l0_ && m == 0));
              if (m == 0)
                static_for<0, RPW>([&](auto r_) {
                  double dv = dg[r_];
                  asm volatile("" : "+v"(dv));
                  acc[r_] = l0_ ? dv : acc[r_];
                });
              uint32_t rowrun = row0_bytes + (uint32_t)m * 512u;
              static_for<0, RPW>([&](auto r_) {
                row_store(acc[r_], (uint32_t)lane * 8u, rowrun);
                rowrun += rstep;
              });
            }
          // ---- pieces right of it: aligned blocks
          for (int b = m0 + 1; b < nblk; ++b)
            {
              double acc[RPW];
              static_for<0, RPW>([&](auto r_) { acc[r_] = 0.0; });
              coupling(acc, b - 1, lane, true);
              uint32_t rowrun = row0_bytes + (uint32_t)b * 512u;
              static_for<0, RPW>([&](auto r_) {
                row_store(acc[r_], (uint32_t)lane * 8u, rowrun);
                rowrun += rstep;
              });
            }
        }
      if constexpr (DRAIN)
        __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0) alone (gfx9 encoding: expcnt 7 and lgkmcnt 15 wait for nothing)
      PDHW_MARK(s, sbase, 1);
      __syncthreads(); // tables of the next polytope in the other buffer; this one may be overwritten
      PDHW_MARK(s, sbase, 2);
    }
}

template <int W, bool SHIFTED, int PMAX>
__global__ void __launch_bounds__(PDH_WAVE *(W + WG_BUILDERS), 1) k_terms_wg(const PdhDev P, const PdhTerms T, const int n_owned)
{
  terms_wg<W, SHIFTED, PMAX, WG_STORE_AUX, WG_DRAIN>(P, T, n_owned);
}
#ifdef PDHT_VARIANTS
template <int W, bool SHIFTED, int PMAX>
__global__ void __launch_bounds__(PDH_WAVE *(W + WG_BUILDERS), 1) k_terms_wg_base(const PdhDev P, const PdhTerms T, const int n_owned)
{
  terms_wg<W, SHIFTED, PMAX, WG_BASE_STORE_AUX, WG_BASE_DRAIN>(P, T, n_owned);
}
#endif
} // namespace pdht
