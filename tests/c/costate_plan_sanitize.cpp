// CPU-only sanitizer harness for the host index arithmetic of the costate kernel (TEST INFRASTRUCTURE).
//
// Compiles pc_costate_plan.hpp (A-table offsets by order, multiplier rows of a phase and of a tile, LDS size, argument
// checks) on top of pc_solution_plan.hpp under g++ -fsanitize=address,undefined, reads meshes, builds every plan and
// walks every multiplier row, A entry, staged row and coefficient slot a lane of pc_sol_costate would touch against
// the array sizes the library allocates, and prints the offsets.  tests/test_costate_plan_sanitize.py compares them
// with a NumPy restatement.
//
//   usage: costate_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case:  K TB NY NU NQ NP c_off lds_limit n_orders | orders... | n_k[K]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../pycollo_amd/csrc/pc_costate_plan.hpp"

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
      long long c_off = 0;
      in >> K >> TB >> NY >> NU >> NQ >> NP >> c_off >> lds_limit >> n_orders;
      if (!in || K < 0 || n_orders < 0) throw std::runtime_error("bad case header");
      std::vector<int32_t> orders((size_t)n_orders), n_k((size_t)K);
      for (auto& e : orders) in >> e;
      for (auto& e : n_k) in >> e;
      if (!in) throw std::runtime_error("input truncated");
      pcs::FitPlan F;
      pcs::CostatePlan P;
      int64_t num_c = 0;
      try {
        F = pcs::build_fit_plan(K, n_k.data(), n_orders, orders.data(), NY, NU, TB, 0);
        // the rows of the phase: NY (N - 1) defects, NP N path rows, NQ integrals; three endpoint rows behind them
        const int64_t c_int_off = c_off + (int64_t)NY * (F.N - 1) + (int64_t)NP * F.N;
        num_c = c_int_off + NQ + 3;
        P = pcs::build_costate_plan(F, n_orders, orders.data(), NY, NQ, c_off, c_int_off, num_c, lds_limit);
      } catch (const std::exception& e) {
        out << "case " << c << " refused\n";
        continue;
      }
      // what the library allocates and the kernel carves: lam [num_c], the A tables [a_total], the C_u tables
      // [tab_total], per state lam_rows(TB) staged rows, node arrays [N], coefficient rows [NC]
      std::vector<double> lam((size_t)num_c, 0.0), tabA((size_t)P.a_total, 0.0), tabU((size_t)F.tab_total, 0.0);
      std::vector<char> node_owned((size_t)F.N, 0), coef_written((size_t)F.NC, 0);
      for (int m = 0; m < NQ; ++m) (void)lam.at((size_t)(P.lam_int_off + m));
      for (int t = 0; t < F.n_tiles(); ++t) {
        const int k0 = F.tile_k0.at((size_t)t), k1 = F.tile_k0.at((size_t)t + 1);
        const int r_lo = P.row_lo.at((size_t)t), r_hi = P.row_hi.at((size_t)t);
        std::vector<char> staged((size_t)pcs::lam_rows(F.TB), 0);
        for (int a = 0; a < NY; ++a)
          for (int i = 0; i < r_hi - r_lo; ++i) {
            (void)lam.at((size_t)(P.lam_off.at((size_t)a) + r_lo + i));
            staged.at((size_t)i) = 1;
          }
        for (int k = k0; k < k1; ++k) {
          const int sk = F.sec_s.at((size_t)k), n = F.sec_s.at((size_t)k + 1) - sk + 1;
          for (int j = 0; j < n; ++j) {
            const int node = sk + j;
            int ka = k, pa = j, kb = k;   // the sections of the node, as the kernel finds them
            if (j == 0 && k > 0) { ka = k - 1; pa = sk - F.sec_s.at((size_t)k - 1); }
            if (j == n - 1 && k < F.K - 1) kb = k + 1;
            for (int kk = ka; kk <= kb; ++kk) {
              const int s0 = F.sec_s.at((size_t)kk), nn = F.sec_s.at((size_t)kk + 1) - s0 + 1, pos = kk == ka ? pa : 0;
              if (s0 + pos != node) throw std::runtime_error("a section does not hold the node at the position found");
              const int off = P.offA[nn];
              if (off < 0) throw std::runtime_error("no A table for an order in use");
              for (int r = 0; r < nn - 1; ++r) {
                (void)tabA.at((size_t)off + (size_t)r * nn + pos);
                if (NY > 0 && !staged.at((size_t)(s0 - r_lo + r))) throw std::runtime_error("a row is read that was not staged");
              }
            }
            if (node == F.N - 1 && NY > 0 && !staged.at((size_t)(F.N - 2 - r_lo)))
              throw std::runtime_error("the last defect row is not staged in the last node's tile");
            if (j < n - 1 || k == F.K - 1) {
              if (node_owned.at((size_t)node)) throw std::runtime_error("a node has two owners");
              node_owned[(size_t)node] = 1;
            }
            const int slot = F.coef_off.at((size_t)k) + j;
            if (coef_written.at((size_t)slot)) throw std::runtime_error("a coefficient slot is written twice");
            coef_written[(size_t)slot] = 1;
            for (int i = 0; i < n; ++i) (void)tabU.at((size_t)F.offC[n] + (size_t)j * n + i);
          }
        }
      }
      for (char o : node_owned) if (!o) throw std::runtime_error("a node has no owner");
      for (char w : coef_written) if (!w) throw std::runtime_error("a coefficient slot is never written");
      out << "case " << c << " ok " << F.N << ' ' << F.NC << ' ' << F.n_tiles() << ' ' << P.a_total << ' ' << P.lds_bytes << ' '
          << P.lam_int_off << '\n';
      put(out, "offA", std::vector<int32_t>(P.offA, P.offA + PC_MAX_ORDER + 1));
      put(out, "lam_off", P.lam_off);
      put(out, "row_lo", P.row_lo);
      put(out, "row_hi", P.row_hi);
    }
    // the argument checks of pc_solution_set_multipliers
    int refused = 0;
    static const double one = 1.0;
    refused += expect_throw([] { pcs::check_multiplier_args(nullptr, 5, 5, &one, 1.0); });
    refused += expect_throw([] { pcs::check_multiplier_args(&one, 5, 5, nullptr, 1.0); });
    refused += expect_throw([] { pcs::check_multiplier_args(&one, 4, 5, &one, 1.0); });
    refused += expect_throw([] { pcs::check_multiplier_args(&one, 6, 5, &one, 1.0); });
    refused += expect_throw([] { pcs::check_multiplier_args(&one, 5, 5, &one, 0.0); });
    refused += expect_throw([] { pcs::check_multiplier_args(&one, 5, 5, &one, __builtin_nan("")); });
    pcs::check_multiplier_args(&one, 5, 5, &one, 0.7);
    out << "refused " << refused << "\nok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "costate_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
