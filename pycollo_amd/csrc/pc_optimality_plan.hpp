// Path and bound multipliers of an NLP point: the host-side index arithmetic of pc_sol_multipliers and
// pc_sol_sample_optimality (compiles without HIP; tests/c/optimality_plan_sanitize.cpp runs it under AddressSanitizer +
// UBSan).  The path rows and x columns of a phase, the offsets of the node-weight rows by order, the LDS the kernel asks
// for and the argument checks of pc_solution_set_bound_multipliers (pc_solution_sample_optimality's are check_sample_args
// of pc_solution_plan.hpp: phase in range, Q >= 0).  The tiles, lanes
// and n x n table offsets are the fit kernel's (pc_solution_plan.hpp).
#ifndef PC_OPTIMALITY_PLAN_HPP
#define PC_OPTIMALITY_PLAN_HPP

#include "pc_costate_plan.hpp"

namespace pcs {

struct OptimalityPlan {
  int32_t offW[PC_MAX_ORDER + 1];          // start of order n's n node weights (the last row of A(n)), -1: none
  int32_t w_total = 0;                     // doubles in the concatenated weight rows
  // The next two restate what the kernel computes itself from c_path_off, x_off and N (as CostatePlan::lam_off does): the
  // host only checks that they fit the vectors; the sanitizer walk reads them, the launch does not.
  std::vector<int64_t> path_off;           // [NP] first multiplier of every path row: c_path_off + i N
  std::vector<int64_t> x_col;              // [NY + NU] first x entry of every node variable: x_off + b N
  size_t lds_bytes = 0;
};

// offsets of the per-order weight rows, in the order the caller lists them
inline int32_t w_table_offsets(int n_orders, const int32_t* orders, int32_t* offW) {
  for (int i = 0; i <= PC_MAX_ORDER; ++i) offW[i] = -1;
  if (n_orders < 0 || (n_orders > 0 && !orders)) throw std::runtime_error("optimality tables: bad list of orders");
  int32_t o = 0;
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (n < 2 || n > PC_MAX_ORDER) throw std::runtime_error("optimality tables: order outside [2, " + std::to_string(PC_MAX_ORDER) + "]");
    if (offW[n] >= 0) throw std::runtime_error("optimality tables: an order is listed twice");
    offW[n] = o;
    o += n;
  }
  return o;
}

// the last rows of the (n - 1) x n integration tables (at offA[n] of tabA), packed by offW
inline std::vector<double> pack_weight_rows(int n_orders, const int32_t* orders, const double* tabA, const int32_t* offA,
                                            const int32_t* offW, int32_t w_total) {
  if (!tabA) throw std::runtime_error("optimality tables: null integration tables");
  std::vector<double> w((size_t)w_total, 0.0);
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (offA[n] < 0 || offW[n] < 0) throw std::runtime_error("optimality tables: an order has no table");
    for (int j = 0; j < n; ++j) w[(size_t)offW[n] + j] = tabA[(size_t)offA[n] + (size_t)(n - 2) * n + j];
  }
  return w;
}

// rho: the weight the NLP's integral rows give a node (the rule's weights qw, order n's at qw_off[n]) over the node weight
// of the costates (the last row of A(n)).  One number for the whole mesh: 1 under Lobatto, 2 under Radau, whose rule
// weights sum to 2.  Refused when the two are not proportional (an entry without node weight must have no rule weight).
inline double integral_weight_scale(int n_orders, const int32_t* orders, const double* tabA, const int32_t* offA,
                                    const double* qw, const int32_t* qw_off) {
  if (!tabA || !qw) throw std::runtime_error("optimality tables: null weight tables");
  double rho = 0.0;
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (offA[n] < 0 || qw_off[n] < 0) throw std::runtime_error("optimality tables: an order has no table");
    double sa = 0.0, sq = 0.0;
    for (int j = 0; j < n; ++j) {
      sa += tabA[(size_t)offA[n] + (size_t)(n - 2) * n + j];
      sq += qw[(size_t)qw_off[n] + j];
    }
    if (!(sa > 0.0)) throw std::runtime_error("optimality tables: an integration table has no weight");
    const double r = sq / sa;
    if (i == 0) rho = r;
    for (int j = 0; j < n; ++j) {
      const double a = tabA[(size_t)offA[n] + (size_t)(n - 2) * n + j], q = qw[(size_t)qw_off[n] + j];
      const double d = q - rho * a;
      if (!((d < 0 ? -d : d) <= 1e-12 * (rho * sa))) throw std::runtime_error("optimality tables: the integral rows' weights are not a multiple of the node weights");
    }
  }
  return n_orders > 0 ? rho : 1.0;
}

// C_u and ydot tables, the weight rows, one staged value per lane and multiplier, the lane tags
inline size_t optimality_lds_bytes(int tab_total, int w_total, int TB, int NP, int NZ) {
  const size_t nm = NP + NZ > 0 ? NP + NZ : 1;
  return 8 * (2 * (size_t)tab_total + (size_t)w_total + nm * (size_t)TB) + 4 * (size_t)TB;
}

// the plan on top of a phase's fit plan; c_path_off / c_int_off: the phase's first path row and first integral row (the
// path rows end there); x_off: the phase's first x entry; num_c / num_x: the lengths of the two multiplier vectors
inline OptimalityPlan build_optimality_plan(const FitPlan& F, int n_orders, const int32_t* orders, int NY, int NU, int NP,
                                            int64_t c_path_off, int64_t c_int_off, int64_t num_c, int64_t x_off, int64_t num_x,
                                            int lds_limit) {
  OptimalityPlan P;
  P.w_total = w_table_offsets(n_orders, orders, P.offW);
  if (NY < 0 || NU < 0 || NP < 0 || c_path_off < 0 || x_off < 0) throw std::runtime_error("optimality: negative size or offset");
  if (c_path_off + (int64_t)NP * F.N > c_int_off || c_int_off > num_c)
    throw std::runtime_error("optimality: the phase's path rows do not fit the multiplier vector");
  if (x_off + (int64_t)(NY + NU) * F.N > num_x) throw std::runtime_error("optimality: the phase's node variables do not fit x");
  for (int i = 0; i < NP; ++i) P.path_off.push_back(c_path_off + (int64_t)i * F.N);
  for (int b = 0; b < NY + NU; ++b) P.x_col.push_back(x_off + (int64_t)b * F.N);
  for (int k = 0; k < F.K; ++k)
    if (P.offW[F.sec_s[(size_t)k + 1] - F.sec_s[(size_t)k] + 1] < 0)
      throw std::runtime_error("optimality tables: an order in use has no table");
  P.lds_bytes = optimality_lds_bytes(F.tab_total, P.w_total, F.TB, NP, NY + NU);
  if (lds_limit > 0 && P.lds_bytes > (size_t)lds_limit) throw std::runtime_error("multiplier kernel: tables do not fit in LDS");
  return P;
}

// pc_solution_set_bound_multipliers: the constraint multipliers must have been set; z may be null (n_z is then ignored)
inline void check_bound_multiplier_args(bool has_multipliers, const void* z, int64_t n_z, int64_t num_x) {
  if (!has_multipliers) throw std::runtime_error("optimality: no multipliers were set");
  if (z && n_z != num_x) throw std::runtime_error("optimality: the bound multiplier vector must have " + std::to_string(num_x) + " entries");
}

}  // namespace pcs

#endif  // PC_OPTIMALITY_PLAN_HPP
