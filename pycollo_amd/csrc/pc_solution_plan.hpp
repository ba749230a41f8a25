// The kernels that read a finished NLP point: the host-side index arithmetic (compiles without HIP;
// tests/c/solution_plan_sanitize.cpp runs it under AddressSanitizer + UBSan).  The section-to-tile table of pc_sol_fit
// and pc_mesh_err, the coefficient offsets, the table offsets by order, the LDS the two kernels ask for and the argument
// checks of the exported calls.
#ifndef PC_SOLUTION_PLAN_HPP
#define PC_SOLUTION_PLAN_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "pc_args.h"

namespace pcs {

struct FitPlan {
  int TB = 256;
  int32_t K = 0, N = 0, NC = 0;            // sections, nodes, coefficients per variable (N + K - 1)
  std::vector<int32_t> sec_s;              // [K+1] first node of every section
  std::vector<int32_t> tile_k0;            // [n_tiles+1]
  std::vector<int32_t> lane0;              // [K]
  std::vector<int32_t> coef_off;           // [K+1] first coefficient of every section: sec_s[k] + k
  int32_t offC[PC_MAX_ORDER + 1];          // start of order n's n x n table, -1: no table
  int32_t tab_total = 0;                   // doubles in one concatenated table
  size_t lds_bytes = 0;
  int n_tiles() const { return (int)tile_k0.size() - 1; }
};

// offsets of the per-order n x n tables, in the order the caller lists them
inline int32_t table_offsets(int n_orders, const int32_t* orders, int32_t* offC) {
  for (int i = 0; i <= PC_MAX_ORDER; ++i) offC[i] = -1;
  if (n_orders < 0 || (n_orders > 0 && !orders)) throw std::runtime_error("solution tables: bad list of orders");
  int64_t o = 0;
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (n < 2 || n > PC_MAX_ORDER) throw std::runtime_error("solution tables: order outside [2, " + std::to_string(PC_MAX_ORDER) + "]");
    if (offC[n] >= 0) throw std::runtime_error("solution tables: an order is listed twice");
    offC[n] = (int32_t)o;
    o += (int64_t)n * n;
  }
  return (int32_t)o;
}

inline size_t fit_lds_bytes(int tab_total, int TB, int NY, int NU) {
  return 8 * (2 * (size_t)tab_total + (size_t)TB * ((NY > 0 ? NY : 1) + (NU > 0 ? NU : 1))) + 4 * (size_t)TB;
}

// tiles of a kernel in which section k owns n_k + extra_lanes consecutive lanes of a workgroup of TB: consecutive
// sections while their lanes fit.  tile_k0 [n_tiles+1]: first section of every tile; lane0 [K]: first lane of every
// section inside its tile.  (The device side is pc::sol_lane_map.)
inline void section_tiles(int K, const int32_t* n_k, int extra_lanes, int TB, std::vector<int32_t>& tile_k0,
                          std::vector<int32_t>& lane0) {
  tile_k0.assign(1, 0);
  lane0.assign((size_t)K, 0);
  int lanes = 0;
  for (int k = 0; k < K; ++k) {
    const int need = n_k[k] + extra_lanes;
    if (lanes + need > TB) {
      tile_k0.push_back(k);
      lanes = 0;
    }
    lane0[k] = lanes;
    lanes += need;
  }
  tile_k0.push_back(K);
}

// the fit kernel: section k owns n_k lanes = its nodes
inline FitPlan build_fit_plan(int K, const int32_t* n_k, int n_orders, const int32_t* orders, int NY, int NU, int TB,
                              int lds_limit) {
  if (K < 1 || !n_k) throw std::runtime_error("solution: a phase needs at least one section");
  if (TB < PC_MAX_ORDER || TB > 1024) throw std::runtime_error("solution: workgroup size outside [20, 1024]");
  FitPlan P;
  P.TB = TB;
  P.K = K;
  P.tab_total = table_offsets(n_orders, orders, P.offC);
  P.sec_s.assign((size_t)K + 1, 0);
  P.coef_off.assign((size_t)K + 1, 0);
  int64_t s = 0;
  for (int k = 0; k < K; ++k) {
    const int n = n_k[k];
    if (n < 2 || n > PC_MAX_ORDER) throw std::runtime_error("solution: section order outside [2, " + std::to_string(PC_MAX_ORDER) + "]");
    if (P.offC[n] < 0) throw std::runtime_error("solution tables: an order in use has no table");
    P.sec_s[k] = (int32_t)s;
    P.coef_off[k] = (int32_t)(s + k);
    s += n - 1;
    if (s + K > INT32_MAX) throw std::runtime_error("solution: the phase has too many nodes for 32-bit node indices");
  }
  section_tiles(K, n_k, 0, TB, P.tile_k0, P.lane0);
  P.sec_s[K] = (int32_t)s;
  P.coef_off[K] = (int32_t)(s + K);          // one past the last section's coefficients
  P.N = (int32_t)s + 1;
  P.NC = P.N + K - 1;
  P.lds_bytes = fit_lds_bytes(P.tab_total, TB, NY, NU);
  if (lds_limit > 0 && P.lds_bytes > (size_t)lds_limit) throw std::runtime_error("solution fit kernel: tables do not fit in LDS");
  return P;
}

// the mesh-error kernel: section k owns n_k + 1 lanes = its nodes on the ph mesh.  Per listed order n (2 .. 19: the ph
// mesh has n + 1 <= 20 nodes) the B and E tables are (n - 1) x n at offBE[n], the A table n x (n + 1) at offA[n].
// Refused beyond what a handle can ask for (it has K >= 1 sections of orders 2 .. 20 and a positive LDS limit): no
// section, and a section order that cannot index the offsets; lds_limit <= 0 means no limit, as in build_fit_plan.
struct MeshErrorPlan {
  int TB = 256;
  std::vector<int32_t> tile_k0;            // [n_tiles+1]
  std::vector<int32_t> lane0;              // [K]
  int32_t offBE[PC_MAX_ORDER + 1];         // -1: no table
  int32_t offA[PC_MAX_ORDER + 1];
  int32_t tab_total_BE = 0, tab_total_A = 0;
  size_t lds_bytes = 0;
  int n_tiles() const { return (int)tile_k0.size() - 1; }
};

inline MeshErrorPlan build_mesh_error_plan(int K, const int32_t* n_k, int n_orders, const int32_t* orders, int NY, int NU,
                                           int TB, int lds_limit) {
  if (K < 1 || !n_k) throw std::runtime_error("mesh-error kernel: a phase needs at least one section");
  MeshErrorPlan P;
  P.TB = TB;
  for (int i = 0; i <= PC_MAX_ORDER; ++i) P.offBE[i] = P.offA[i] = -1;
  size_t oBE = 0, oA = 0;
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (n < 2 || n >= PC_MAX_ORDER) throw std::runtime_error("mesh-error tables: order outside [2, 19]");
    P.offBE[n] = (int32_t)oBE;
    P.offA[n] = (int32_t)oA;
    oBE += (size_t)(n - 1) * n;
    oA += (size_t)n * (n + 1);
  }
  for (int k = 0; k < K; ++k)
    if (n_k[k] < 0 || n_k[k] > PC_MAX_ORDER || P.offBE[n_k[k]] < 0)
      throw std::runtime_error("mesh-error tables: an order in use has no table");
  section_tiles(K, n_k, 1, TB, P.tile_k0, P.lane0);
  P.tab_total_BE = (int32_t)oBE;
  P.tab_total_A = (int32_t)oA;
  P.lds_bytes = 8 * (2 * oBE + oA + (size_t)TB * (5 * (size_t)NY + (NU > 0 ? NU : 1) + 1)) + 4 * (size_t)TB;
  if (lds_limit > 0 && P.lds_bytes > (size_t)lds_limit) throw std::runtime_error("mesh-error kernel: tables do not fit in LDS");
  return P;
}

// section boundaries in tau from the node abscissae; they must increase
inline std::vector<double> section_edges(const FitPlan& P, const double* tau) {
  if (!tau) throw std::runtime_error("solution: null node abscissae");
  std::vector<double> e((size_t)P.K + 1);
  for (int k = 0; k <= P.K; ++k) e[k] = tau[P.sec_s[k]];
  for (int k = 0; k < P.K; ++k)
    if (!(e[k + 1] > e[k])) throw std::runtime_error("solution: section boundaries do not increase");
  return e;
}

inline void check_sample_args(int n_phases, int phase, const void* t, int64_t n_t, int flags) {
  if (phase < 0 || phase >= n_phases) throw std::runtime_error("solution: phase out of range");
  if (n_t < 0) throw std::runtime_error("solution: negative number of queries");
  if (n_t > 0 && !t) throw std::runtime_error("solution: null queries");
  if (flags & ~(PC_SOL_TAU | PC_SOL_EXTRAPOLATE)) throw std::runtime_error("solution: unknown flag");
  if ((n_t + 255) / 256 > INT32_MAX) throw std::runtime_error("solution: too many queries for one launch");
}

inline int64_t sample_blocks(int64_t n_t, int TB) { return (n_t + TB - 1) / TB; }

}  // namespace pcs

#endif  // PC_SOLUTION_PLAN_HPP
