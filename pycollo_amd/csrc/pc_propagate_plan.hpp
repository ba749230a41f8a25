// Forward propagation of an NLP point: the host-side index arithmetic of pc_sol_propagate (compiles without HIP;
// tests/c/propagate_plan_sanitize.cpp runs it under AddressSanitizer + UBSan).  The checks of the segment list and of
// the tolerances, the first section of every segment and the grid.  The sections are the fit kernel's
// (pc_solution_plan.hpp).  For pc_sol_propagate_dense also the check of integral_atol and the queries: their
// checks, their stable sort and the slot of every query (tests/c/propagate_dense_plan_sanitize.cpp).  For
// pc_sol_propagate_stiff the check of its options and the lane's LDS indexing
// (tests/c/propagate_stiff_plan_sanitize.cpp).  The three kernels share one plan, one set of staged lists and the
// argument prefix PcSolPropCommon (pc_solution_host.hpp: solution_stage_propagate); the step control of a node interval
// is host-testable too, in a header of its own (pc_step_control.hpp, tests/c/step_control_sanitize.cpp).
#ifndef PC_PROPAGATE_PLAN_HPP
#define PC_PROPAGATE_PLAN_HPP

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "pc_solution_plan.hpp"

namespace pcs {

struct PropagatePlan {
  int TB = PC_SOL_PROP_TB;
  int32_t n_seg = 0;
  std::vector<int32_t> seg_node;   // [n_seg+1] strictly ascending, 0 .. N - 1
  std::vector<int32_t> seg_sec;    // [n_seg] section k of every segment's first interval: sec_s[k] <= seg_node[i] < sec_s[k+1]
  int64_t blocks = 0;              // workgroups of TB lanes, one lane per segment
};

// substeps >= 1: fixed steps per node interval; 0: adaptive (then rtol counts).  atol: one entry per state.
inline void check_propagate_tolerances(int64_t substeps, double rtol, const double* atol, int NY, int64_t max_steps) {
  if (substeps < 0) throw std::runtime_error("propagate: negative substeps");
  if (substeps > PC_SOL_PROP_MAX_STEPS) throw std::runtime_error("propagate: substeps above 2^20");
  if (substeps == 0 && !(std::isfinite(rtol) && rtol > 0.0)) throw std::runtime_error("propagate: rtol must be finite and positive");
  if (NY < 0 || (NY > 0 && !atol)) throw std::runtime_error("propagate: null atol");
  for (int a = 0; a < NY; ++a)
    if (!(std::isfinite(atol[a]) && atol[a] > 0.0)) throw std::runtime_error("propagate: every atol must be finite and positive");
  if (max_steps < 1 || max_steps > PC_SOL_PROP_MAX_STEPS) throw std::runtime_error("propagate: max_steps outside [1, 2^20]");
}

// The options of the implicit method (pc_sol_propagate_stiff): the checks above, except that rtol counts in
// both modes (the Newton iteration stops by it), and newton_max in 1 .. PC_SOL_STIFF_MAX_NEWTON.  NY above
// PC_SOL_STIFF_MAX_NY is refused: the lane's factors would not fit a workgroup's LDS.
inline void check_propagate_stiff_options(int64_t substeps, double rtol, const double* atol, int NY, int64_t max_steps,
                                          int64_t newton_max) {
  if (NY > PC_SOL_STIFF_MAX_NY)
    throw std::runtime_error("propagate: the implicit method takes phases of at most " + std::to_string(PC_SOL_STIFF_MAX_NY) +
                             " states (PC_SOL_STIFF_MAX_NY), this one has " + std::to_string(NY));
  if (!(std::isfinite(rtol) && rtol > 0.0)) throw std::runtime_error("propagate: rtol must be finite and positive");
  check_propagate_tolerances(substeps, rtol, atol, NY, max_steps);
  if (newton_max < 1 || newton_max > PC_SOL_STIFF_MAX_NEWTON)
    throw std::runtime_error("propagate: newton_max outside [1, " + std::to_string(PC_SOL_STIFF_MAX_NEWTON) + "]");
}

// Where element e (row-major in the NY x NY block, e < NY^2) of lane l's factors and row swap k (k < NY) lie in the
// workgroup's two LDS arrays of pc_sol_propagate_stiff: the kernel's own expressions, restated for the host tests.
inline int64_t stiff_lu_index(int e, int lane, int TB = PC_SOL_PROP_TB) { return (int64_t)e * TB + lane; }
inline int64_t stiff_piv_index(int k, int lane, int TB = PC_SOL_PROP_TB) { return (int64_t)k * TB + lane; }
inline int64_t stiff_lds_bytes(int NY, int TB = PC_SOL_PROP_TB) {
  const int64_t n = NY > 0 ? NY : 1;
  return n * n * TB * (int64_t)sizeof(double) + n * TB * (int64_t)sizeof(int32_t);
}

inline PropagatePlan build_propagate_plan(const FitPlan& F, int64_t n_seg, const int32_t* seg_nodes, int TB = PC_SOL_PROP_TB) {
  if (n_seg < 1 || !seg_nodes) throw std::runtime_error("propagate: at least one segment is needed");
  if (n_seg > (int64_t)F.N - 1) throw std::runtime_error("propagate: more segments than node intervals");
  if (TB < 1 || TB > 1024) throw std::runtime_error("propagate: workgroup size outside [1, 1024]");
  if (seg_nodes[0] != 0) throw std::runtime_error("propagate: the first segment must start at node 0");
  if (seg_nodes[n_seg] != F.N - 1) throw std::runtime_error("propagate: the last segment must end at the last node");
  PropagatePlan P;
  P.TB = TB;
  P.n_seg = (int32_t)n_seg;
  P.seg_node.assign(seg_nodes, seg_nodes + n_seg + 1);
  P.seg_sec.assign((size_t)n_seg, 0);
  int k = 0;
  for (int64_t i = 0; i < n_seg; ++i) {
    const int32_t j = seg_nodes[i];
    if (!(seg_nodes[i + 1] > j)) throw std::runtime_error("propagate: the segment list must be strictly ascending");
    while (k < F.K - 1 && j >= F.sec_s[(size_t)k + 1]) ++k;   // (ascending starts: the walk never goes back)
    P.seg_sec[(size_t)i] = k;
  }
  P.blocks = (n_seg + TB - 1) / TB;
  return P;
}

// ---- integrals and dense output (pc_sol_propagate_dense) ----
// integral_atol: null (the integrals take no part in the error norm), or one finite positive entry per integral
inline void check_integral_atol(const double* integral_atol, int NQ) {
  if (NQ < 0) throw std::runtime_error("propagate: negative integral count");
  if (!integral_atol) return;
  for (int m = 0; m < NQ; ++m)
    if (!(std::isfinite(integral_atol[m]) && integral_atol[m] > 0.0))
      throw std::runtime_error("propagate: every integral_atol must be finite and positive");
}

// The queries of a dense propagation, sorted.  Slot 0 holds the queries at tau_0; slot j >= 1 those in (tau_{j-1},
// tau_j]: a query on a node belongs to the interval that ends there.  Slot j is the sorted queries node_q0[j] ..
// node_q0[j+1]; sorted query k is the caller's query q_order[k] (a stable sort: equal queries keep the caller's order).
struct DenseQueryPlan {
  int64_t Q = 0;
  std::vector<int32_t> q_order;    // [Q]
  std::vector<int32_t> node_q0;    // [N+1] ascending, node_q0[0] = 0, node_q0[N] = Q
  std::vector<double> tau_sorted;  // [Q] ascending
};

// node_tau [N] strictly ascending.  Refused: a query that is NaN, infinite or outside [tau_0, tau_{N-1}] (a propagated
// path is not extrapolated), Q < 0, Q >= 2^31, a null array with Q > 0.
inline DenseQueryPlan build_dense_query_plan(int N, const double* node_tau, int64_t Q, const double* tau_q) {
  if (N < 2 || !node_tau) throw std::runtime_error("propagate: the phase has no node interval");
  if (Q < 0 || Q > (int64_t)INT32_MAX) throw std::runtime_error("propagate: the number of queries must be in [0, 2^31)");
  if (Q > 0 && !tau_q) throw std::runtime_error("propagate: null queries");
  for (int64_t q = 0; q < Q; ++q) {
    if (!std::isfinite(tau_q[q])) throw std::runtime_error("propagate: a query is not finite");
    if (!(tau_q[q] >= node_tau[0] && tau_q[q] <= node_tau[N - 1])) throw std::runtime_error("propagate: a query lies outside the phase");
  }
  DenseQueryPlan D;
  D.Q = Q;
  D.q_order.resize((size_t)Q);
  for (int64_t q = 0; q < Q; ++q) D.q_order[(size_t)q] = (int32_t)q;
  std::stable_sort(D.q_order.begin(), D.q_order.end(), [&](int32_t a, int32_t b) { return tau_q[a] < tau_q[b]; });
  D.tau_sorted.resize((size_t)Q);
  D.node_q0.assign((size_t)N + 1, 0);
  for (int64_t k = 0; k < Q; ++k) {
    const double t = tau_q[D.q_order[(size_t)k]];
    D.tau_sorted[(size_t)k] = t;
    int lo = 0, hi = N - 1;   // the first node j with t <= tau_j (t <= tau_{N-1} was checked)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t <= node_tau[mid]) hi = mid; else lo = mid + 1;
    }
    ++D.node_q0[(size_t)lo + 1];
  }
  for (int j = 0; j < N; ++j) D.node_q0[(size_t)j + 1] += D.node_q0[(size_t)j];
  return D;
}

}  // namespace pcs

#endif  // PC_PROPAGATE_PLAN_HPP
