// Costates of an NLP point: the host-side index arithmetic of pc_sol_costate (compiles without HIP;
// tests/c/costate_plan_sanitize.cpp runs it under AddressSanitizer + UBSan).  The offsets of the (n - 1) x n
// integration tables by order, the multiplier rows of a phase and of a tile, the LDS the kernel asks for and the
// argument checks of pc_solution_set_multipliers.  The tiles and lanes are the fit kernel's (pc_solution_plan.hpp).
#ifndef PC_COSTATE_PLAN_HPP
#define PC_COSTATE_PLAN_HPP

#include "pc_solution_plan.hpp"

namespace pcs {

// staged multiplier rows of one state in a workgroup of TB lanes (pc_solution.hpp, PC_SOL_LAM_ROWS): a tile's own
// sections have at most TB - 1 rows, each neighbour section at most PC_MAX_ORDER - 1
inline int lam_rows(int TB) { return TB + 2 * PC_MAX_ORDER; }

struct CostatePlan {
  int32_t offA[PC_MAX_ORDER + 1];          // start of order n's (n - 1) x n table, -1: no table
  int32_t a_total = 0;                     // doubles in the concatenated A tables
  std::vector<int64_t> lam_off;            // [NY] first defect multiplier of every state: c_off + a (N - 1)
  int64_t lam_int_off = 0;                 // first integral multiplier
  std::vector<int32_t> row_lo, row_hi;     // [n_tiles] defect rows [row_lo, row_hi) a tile stages per state
  size_t lds_bytes = 0;
};

// offsets of the per-order (n - 1) x n tables, in the order the caller lists them
inline int32_t a_table_offsets(int n_orders, const int32_t* orders, int32_t* offA) {
  for (int i = 0; i <= PC_MAX_ORDER; ++i) offA[i] = -1;
  if (n_orders < 0 || (n_orders > 0 && !orders)) throw std::runtime_error("costate tables: bad list of orders");
  int64_t o = 0;
  for (int i = 0; i < n_orders; ++i) {
    const int n = orders[i];
    if (n < 2 || n > PC_MAX_ORDER) throw std::runtime_error("costate tables: order outside [2, " + std::to_string(PC_MAX_ORDER) + "]");
    if (offA[n] >= 0) throw std::runtime_error("costate tables: an order is listed twice");
    offA[n] = (int32_t)o;
    o += (int64_t)(n - 1) * n;
  }
  return (int32_t)o;
}

inline size_t costate_lds_bytes(int tab_total, int a_total, int TB, int NY) {
  const size_t ny = NY > 0 ? NY : 1;
  return 8 * ((size_t)tab_total + (size_t)a_total + ny * ((size_t)lam_rows(TB) + (size_t)TB)) + 4 * (size_t)TB;
}

// the costate kernel's plan on top of a phase's fit plan; c_off / c_int_off / num_c are the phase's first defect row,
// its first integral row and the length of the multiplier vector
inline CostatePlan build_costate_plan(const FitPlan& F, int n_orders, const int32_t* orders, int NY, int NQ, int64_t c_off,
                                      int64_t c_int_off, int64_t num_c, int lds_limit) {
  CostatePlan P;
  P.a_total = a_table_offsets(n_orders, orders, P.offA);
  if (NY < 0 || NQ < 0 || c_off < 0) throw std::runtime_error("costates: negative size or offset");
  if (c_off + (int64_t)NY * (F.N - 1) > c_int_off || c_int_off + NQ > num_c)
    throw std::runtime_error("costates: the phase's multiplier rows do not fit the multiplier vector");
  P.lam_off.resize((size_t)NY);
  for (int a = 0; a < NY; ++a) P.lam_off[(size_t)a] = c_off + (int64_t)a * (F.N - 1);
  P.lam_int_off = c_int_off;
  for (int t = 0; t < F.n_tiles(); ++t) {
    const int k0 = F.tile_k0[(size_t)t], k1 = F.tile_k0[(size_t)t + 1];
    const int lo = F.sec_s[(size_t)(k0 > 0 ? k0 - 1 : 0)], hi = F.sec_s[(size_t)(k1 < F.K ? k1 + 1 : F.K)];
    if (hi - lo > lam_rows(F.TB)) throw std::runtime_error("costates: a tile's multiplier rows exceed its staging buffer");
    P.row_lo.push_back(lo);
    P.row_hi.push_back(hi);
  }
  for (int k = 0; k < F.K; ++k)
    if (P.offA[F.sec_s[(size_t)k + 1] - F.sec_s[(size_t)k] + 1] < 0)
      throw std::runtime_error("costate tables: an order in use has no table");
  P.lds_bytes = costate_lds_bytes(F.tab_total, P.a_total, F.TB, NY);
  if (lds_limit > 0 && P.lds_bytes > (size_t)lds_limit) throw std::runtime_error("costate kernel: tables do not fit in LDS");
  return P;
}

inline void check_multiplier_args(const void* lam, int64_t n_lam, int64_t num_c, const void* tabA, double wJ) {
  if (!lam || !tabA) throw std::runtime_error("costates: null argument");
  if (n_lam != num_c) throw std::runtime_error("costates: the multiplier vector must have " + std::to_string(num_c) + " entries");
  if (!(wJ != 0.0) || wJ != wJ) throw std::runtime_error("costates: the objective scaling is zero or NaN");
}

}  // namespace pcs

#endif  // PC_COSTATE_PLAN_HPP
