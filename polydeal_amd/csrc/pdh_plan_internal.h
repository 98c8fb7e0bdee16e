// pdh_plan_internal.h — small helpers of the planner (pdh_plan.cpp) that nothing else includes: refusals, the writers of the record
// fields the two kinds of slot record have in common, and what the face analysis hands to the builders of the tables.
#pragma once
#include "pdh_plan.h"

#include <cmath>
#include <cstring>

inline int fail(std::string &err, int code, const std::string &msg) { return err = msg, code; }
#define PDH_TRY(call) do { const int rc_ = (call); if (rc_ != PDH_OK) return rc_; } while (0)

// a builder's refusal: leaves the reason (if asked for) and returns false
inline bool refuse(std::string *why, const char *m) { return why ? (*why = m, false) : false; }

// fn(i) for all i < n on all host threads: did every call return true?
template <class F>
bool host_parallel_all(size_t n, F &&fn)
{
  std::vector<char> bad(n, 0);
  host_parallel_for(n, [&](size_t i) { bad[i] = !fn(i); });
  return std::find(bad.begin(), bad.end(), 1) == bad.end();
}

// side of the box of polytope a along d (3-D)
inline double box_side(const pdh_problem *p, int a, int d) { return p->bbox[(size_t)a * 6 + 3 + d] - p->bbox[(size_t)a * 6 + d]; }

// ---- record fields (the kernels read integers through the bits of a double) ----------------------------------------------------------
inline double as_d(long long v)
{
  double d;
  std::memcpy(&d, &v, sizeof(d));
  return d;
}
// box of polytope a as lower corner and 1 / side; a < 0 (boundary): 0 and 1
inline void write_box(double *dst_lo, double *dst_inv_h, const pdh_problem *p, int a)
{
  for (int c = 0; c < 3; ++c)
    dst_lo[c] = a >= 0 ? p->bbox[(size_t)a * 6 + c] : 0.0, dst_inv_h[c] = a >= 0 ? 1.0 / box_side(p, a, c) : 1.0;
}
// fields 1 .. 9 of a slot record of either family: own box, row base, row length, position of the own block
inline void write_slot_header(double *rec, const pdh_problem *p, const Packed &K, size_t sl)
{
  write_box(rec + 1, rec + 4, p, K.own_agg[sl]);
  rec[7] = as_d(K.row_base[sl]), rec[8] = as_d(K.row_len[sl]), rec[9] = as_d(K.diag_L[sl]);
}

// ---- face analysis ------------------------------------------------------------------------------------------------------------------
struct Plane { int axis; double sign, coord; };
struct FaceAnalysis
{
  std::vector<std::vector<Plane>> planes; // of every run (owned slots)
  std::vector<std::vector<size_t>> order; // runs of every owned slot in record order: boundary first, then ascending block rank
  size_t n_ordered = 0;                   // runs in `order` (all of them, or the bookkeeping of the runs is broken)
};
void order_runs_of_slots(const Packed &K, FaceAnalysis &A);
// does point q of run r lie in plane pl (h: side of the owner's box along the plane's axis)?
inline bool in_plane(const Packed &K, size_t r, int64_t q, const Plane &pl, double h)
{
  return K.ap_n(pl.axis, r, q) * pl.sign > 0.5 && std::fabs(K.ap_x(pl.axis, r, q) - pl.coord) <= 1e-9 * h;
}
double geometry_rounding(const pdh_problem *p, int a);
// points per direction of the verified tensor volume rules (pdh_problem::vq_tensor_n resolved), 0: none
int resolve_volume_rules(const pdh_problem *p, const Packed &K);
// RowsHost::fq_tensor_n / fast_j / planar_ok and A; false (with the reason) if the faces are not unions of axis-aligned planes
bool analyse_faces(const pdh_problem *p, const Packed &K, RowsHost &R, FaceAnalysis &A, std::string *why);
bool build_rows_tables(const pdh_problem *p, const Packed &K, const FaceAnalysis &A, const PlanSwitches &sw, RowsHost &R, std::string *why);
bool rows_kind_applies(const pdh_problem *p, const Packed &K, const RowsHost &RH, int &vq_n, bool &tensor_only, std::string *why);
bool build_terms_tables(const pdh_problem *p, const Packed &K, const RowsHost &RH, const FaceAnalysis &A, int vq_n, const PlanSwitches &sw,
                        TermsHost &T, std::string *why);
