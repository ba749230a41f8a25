// Forward propagation of an NLP point: the host-side index arithmetic of pc_sol_propagate (compiles without HIP;
// tests/c/propagate_plan_sanitize.cpp runs it under AddressSanitizer + UBSan).  The checks of the segment list and of
// the tolerances, the first section of every segment and the grid.  The sections are the fit kernel's
// (pc_solution_plan.hpp).
#ifndef PC_PROPAGATE_PLAN_HPP
#define PC_PROPAGATE_PLAN_HPP

#include <cmath>

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

}  // namespace pcs

#endif  // PC_PROPAGATE_PLAN_HPP
