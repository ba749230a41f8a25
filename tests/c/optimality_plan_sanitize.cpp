// CPU-only sanitizer harness for the host index arithmetic of the multiplier kernels (TEST INFRASTRUCTURE).
//
// Compiles pc_optimality_plan.hpp (path rows and x columns of a phase, weight-row offsets by order, LDS size, argument
// checks) on top of pc_solution_plan.hpp under g++ -fsanitize=address,undefined, reads meshes, builds every plan and
// walks every multiplier row, x column, table entry, staged slot and coefficient slot a lane of pc_sol_multipliers would
// touch against the array sizes the library allocates, checks that every output slot is written exactly once, and
// prints the offsets.  tests/test_optimality_plan_sanitize.py compares them with a NumPy restatement.
//
//   usage: optimality_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case:  K TB NY NU NQ NP c_off x_off lds_limit n_orders | orders... | n_k[K]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../pycollo_amd/csrc/pc_optimality_plan.hpp"

namespace {

template <class T>
void put(std::ostream& out, const char* name, const std::vector<T>& v) {
  out << name << ' ' << v.size();
  for (const auto& e : v) out << ' ' << (long long)e;
  out << '\n';
}

int expect_throw(void (*f)()) {
  try {
    f();
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}

// every slot of an output array is written exactly once
struct Once {
  std::vector<char> hit;
  const char* what;
  Once(size_t n, const char* w) : hit(n, 0), what(w) {}
  void write(size_t i) {
    if (hit.at(i)) throw std::runtime_error(std::string(what) + ": a slot is written twice");
    hit[i] = 1;
  }
  void complete() const {
    for (char h : hit)
      if (!h) throw std::runtime_error(std::string(what) + ": a slot is never written");
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <in.txt> <out.txt>\n", argv[0]);
    return 2;
  }
  try {
    std::ifstream in(argv[1]);
    if (!in) throw std::runtime_error("cannot open input");
    std::ofstream out(argv[2]);
    int n_cases = 0;
    in >> n_cases;
    for (int c = 0; c < n_cases; ++c) {
      int K = 0, TB = 0, NY = 0, NU = 0, NQ = 0, NP = 0, lds_limit = 0, n_orders = 0;
      long long c_off = 0, x_off = 0;
      in >> K >> TB >> NY >> NU >> NQ >> NP >> c_off >> x_off >> lds_limit >> n_orders;
      if (!in || K < 0 || n_orders < 0) throw std::runtime_error("bad case header");
      std::vector<int32_t> orders((size_t)n_orders), n_k((size_t)K);
      for (auto& e : orders) in >> e;
      for (auto& e : n_k) in >> e;
      if (!in) throw std::runtime_error("input truncated");
      pcs::FitPlan F;
      pcs::OptimalityPlan P;
      int64_t num_c = 0, num_x = 0;
      const int NZ = NY + NU;
      try {
        F = pcs::build_fit_plan(K, n_k.data(), n_orders, orders.data(), NY, NU, TB, 0);
        // the rows of the phase: NY (N - 1) defects, NP N path rows, NQ integrals, three endpoint rows behind them; its
        // variables: NZ N node values, NQ integrals and two times, five static parameters behind them
        const int64_t c_path_off = c_off + (int64_t)NY * (F.N - 1), c_int_off = c_path_off + (int64_t)NP * F.N;
        num_c = c_int_off + NQ + 3;
        num_x = x_off + (int64_t)NZ * F.N + NQ + 2 + 5;
        P = pcs::build_optimality_plan(F, n_orders, orders.data(), NY, NU, NP, c_path_off, c_int_off, num_c, x_off, num_x, lds_limit);
      } catch (const std::exception& e) {
        out << "case " << c << " refused\n";
        continue;
      }
      // what the library allocates and the kernel carves
      int32_t offA[PC_MAX_ORDER + 1];
      const int32_t a_total = pcs::a_table_offsets(n_orders, orders.data(), offA);
      std::vector<double> tabA((size_t)a_total, 0.0), qw((size_t)P.w_total, 0.0);
      for (int i = 0; i < n_orders; ++i)   // the last row of A(n): weights 1 / n; the rule's weights: twice that
        for (int j = 0; j < orders[i]; ++j) {
          tabA.at((size_t)offA[orders[i]] + (size_t)(orders[i] - 2) * orders[i] + j) = 1.0 / orders[i];
          qw.at((size_t)P.offW[orders[i]] + j) = 2.0 / orders[i];
        }
      const std::vector<double> tabW = pcs::pack_weight_rows(n_orders, orders.data(), tabA.data(), offA, P.offW, P.w_total);
      if ((int32_t)tabW.size() != P.w_total) throw std::runtime_error("the packed weight rows have another length");
      for (int i = 0; i < n_orders; ++i)
        for (int j = 0; j < orders[i]; ++j)
          if (tabW.at((size_t)P.offW[orders[i]] + j) != 1.0 / orders[i]) throw std::runtime_error("a weight row was packed from another place");
      const double rho = pcs::integral_weight_scale(n_orders, orders.data(), tabA.data(), offA, qw.data(), P.offW);
      if (!(rho > 1.999999 && rho < 2.000001)) throw std::runtime_error("the integral weight scale is not the tables' ratio");
      std::vector<double> lam((size_t)num_c, 0.0), z((size_t)num_x, 0.0), tabU((size_t)F.tab_total, 0.0), tabD((size_t)F.tab_total, 0.0);
      const size_t lds_doubles = (P.lds_bytes - 4 * (size_t)F.TB) / 8;
      const size_t o_val = 2 * (size_t)F.tab_total + (size_t)P.w_total;   // s_val behind s_U, s_D, s_W
      if (o_val + (size_t)(NP + NZ > 0 ? NP + NZ : 1) * F.TB != lds_doubles) throw std::runtime_error("the LDS carve does not add up");
      Once node_mu((size_t)NP * F.N, "node_mu"), node_zeta((size_t)NZ * F.N, "node_zeta"), node_Hz((size_t)NZ * F.N, "node_Hz"),
          end_z((size_t)2 * NY, "end_z"), coef_mu((size_t)NP * F.NC, "coef_mu"), coef_zeta((size_t)NZ * F.NC, "coef_zeta");
      for (int t = 0; t < F.n_tiles(); ++t) {
        const int k0 = F.tile_k0.at((size_t)t), k1 = F.tile_k0.at((size_t)t + 1);
        std::vector<char> staged((size_t)(NP + NZ) * F.TB, 0);
        for (int pass = 0; pass < 2; ++pass)   // 0: the node values and the staging; 1: the contraction behind the barrier
          for (int k = k0; k < k1; ++k) {
            const int sk = F.sec_s.at((size_t)k), n = F.sec_s.at((size_t)k + 1) - sk + 1, l0 = F.lane0.at((size_t)k);
            for (int j = 0; j < n; ++j) {
              const int node = sk + j, tid = l0 + j;
              if (tid >= F.TB) throw std::runtime_error("a lane beyond the workgroup");
              const bool owner = j < n - 1 || k == F.K - 1;
              if (pass == 0) {
                int ka = k, pa = j, kb = k;   // the sections of the node, as the kernel finds them
                if (j == 0 && k > 0) { ka = k - 1; pa = sk - F.sec_s.at((size_t)k - 1); }
                if (j == n - 1 && k < F.K - 1) kb = k + 1;
                for (int kk = ka; kk <= kb; ++kk) {
                  const int s0 = F.sec_s.at((size_t)kk), nn = F.sec_s.at((size_t)kk + 1) - s0 + 1, pos = kk == ka ? pa : 0;
                  if (s0 + pos != node) throw std::runtime_error("a section does not hold the node at the position found");
                  if (P.offW[nn] < 0) throw std::runtime_error("no weight row for an order in use");
                  (void)tabW.at((size_t)P.offW[nn] + (size_t)pos);
                }
                for (int i = 0; i < NP; ++i) {
                  (void)lam.at((size_t)(P.path_off.at((size_t)i) + node));
                  staged.at((size_t)i * F.TB + tid) = 1;
                  if (owner) node_mu.write((size_t)i * F.N + node);
                }
                for (int b = 0; b < NZ; ++b) {
                  (void)z.at((size_t)(P.x_col.at((size_t)b) + node));
                  staged.at((size_t)(NP + b) * F.TB + tid) = 1;
                  if (owner) {
                    node_zeta.write((size_t)b * F.N + node);
                    node_Hz.write((size_t)b * F.N + node);
                    if (b < NY && (node == 0 || node == F.N - 1)) end_z.write((size_t)2 * b + (node == 0 ? 0 : 1));
                  }
                }
              } else {
                const std::vector<double>& T = k == F.K - 1 ? tabD : tabU;
                const int slot = F.coef_off.at((size_t)k) + j;
                for (int i = 0; i < n; ++i) {
                  (void)T.at((size_t)F.offC[n] + (size_t)j * n + i);
                  for (int m = 0; m < NP + NZ; ++m)
                    if (!staged.at((size_t)m * F.TB + l0 + i)) throw std::runtime_error("a value is contracted that was not staged");
                }
                for (int i = 0; i < NP; ++i) coef_mu.write((size_t)i * F.NC + slot);
                for (int b = 0; b < NZ; ++b) coef_zeta.write((size_t)b * F.NC + slot);
              }
            }
          }
      }
      node_mu.complete();
      node_zeta.complete();
      node_Hz.complete();
      end_z.complete();
      coef_mu.complete();
      coef_zeta.complete();
      out << "case " << c << " ok " << F.N << ' ' << F.NC << ' ' << F.n_tiles() << ' ' << P.w_total << ' ' << P.lds_bytes << '\n';
      put(out, "offW", std::vector<int32_t>(P.offW, P.offW + PC_MAX_ORDER + 1));
      put(out, "path_off", P.path_off);
      put(out, "x_col", P.x_col);
    }
    // the argument checks of pc_solution_set_bound_multipliers and pc_solution_sample_optimality
    int refused = 0;
    static const double one = 1.0;
    refused += expect_throw([] { pcs::check_bound_multiplier_args(false, &one, 5, 5); });     // multipliers must be set
    refused += expect_throw([] { pcs::check_bound_multiplier_args(false, nullptr, 0, 5); });
    refused += expect_throw([] { pcs::check_bound_multiplier_args(true, &one, 4, 5); });      // the length must be num_x
    refused += expect_throw([] { pcs::check_bound_multiplier_args(true, &one, 6, 5); });
    refused += expect_throw([] { pcs::check_sample_args(2, 2, &one, 1, 0); });    // phase in range
    refused += expect_throw([] { pcs::check_sample_args(2, -1, &one, 1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, &one, -1, 0); });   // Q >= 0
    refused += expect_throw([] { pcs::check_sample_args(2, 0, nullptr, 1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, &one, 1, 4); });    // unknown flag
    pcs::check_bound_multiplier_args(true, &one, 5, 5);
    pcs::check_bound_multiplier_args(true, nullptr, 0, 5);
    pcs::check_sample_args(2, 1, nullptr, 0, PC_SOL_TAU | PC_SOL_EXTRAPOLATE);
    // weights that are no multiple of the node weights
    refused += expect_throw([] {
      const int32_t orders[1] = {3};
      int32_t offA[PC_MAX_ORDER + 1], offW[PC_MAX_ORDER + 1];
      (void)pcs::a_table_offsets(1, orders, offA);
      (void)pcs::w_table_offsets(1, orders, offW);
      const double A[6] = {0, 0, 0, 0.25, 0.5, 0.25}, q[3] = {0.5, 0.5, 0.5};
      (void)pcs::integral_weight_scale(1, orders, A, offA, q, offW);
    });
    out << "refused " << refused << "\nok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "optimality_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
