// CPU-only sanitizer harness for the host index arithmetic of the propagation with integrals and dense output (TEST
// INFRASTRUCTURE).
//
// Compiles pc_propagate_plan.hpp (the checks of integral_atol and of the queries, the stable sort of the queries, the
// slot of every query) under g++ -fsanitize=address,undefined, reads meshes, segment lists and queries, builds every
// plan and walks every slot a lane of pc_sol_propagate_dense would read or write against the array sizes the library
// allocates: every dense column and every arrive column must be written exactly once.  It prints the plan;
// tests/test_propagate_dense_plan_sanitize.py compares it with a NumPy restatement.
//
//   usage: propagate_dense_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case:  K n_orders n_seg NQ has_iatol Q | orders... | n_k[K] | seg_nodes[n_seg + 1] |
//           tau[N] | integral_atol[NQ] (if has_iatol) | queries[Q]         (reals may be nan or inf)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../pycollo_amd/csrc/pc_propagate_plan.hpp"

namespace {

template <class T>
void put(std::ostream& out, const char* name, const std::vector<T>& v) {
  out << name << ' ' << v.size();
  for (const auto& e : v) out << ' ' << (long long)e;
  out << '\n';
}

double real(std::istream& in) {   // (operator>> does not read "nan" / "inf")
  std::string tok;
  in >> tok;
  return std::strtod(tok.c_str(), nullptr);
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
    int n_cases = 0, refused = 0;
    in >> n_cases;
    for (int c = 0; c < n_cases; ++c) {
      int K = 0, n_orders = 0, NQ = 0, has_iatol = 0;
      long long n_seg = 0, Q = 0;
      in >> K >> n_orders >> n_seg >> NQ >> has_iatol >> Q;
      if (!in || K < 1 || n_orders < 0 || n_seg < 1 || NQ < 0 || Q < 0) throw std::runtime_error("bad case header");
      std::vector<int32_t> orders((size_t)n_orders), n_k((size_t)K), seg((size_t)n_seg + 1);
      for (auto& e : orders) in >> e;
      for (auto& e : n_k) in >> e;
      for (auto& e : seg) in >> e;
      const pcs::FitPlan F = pcs::build_fit_plan(K, n_k.data(), n_orders, orders.data(), 1, 1, 256, 0);
      std::vector<double> tau((size_t)F.N), iatol(has_iatol ? (size_t)NQ : 0), query((size_t)Q);
      for (auto& e : tau) e = real(in);
      for (auto& e : iatol) e = real(in);
      for (auto& e : query) e = real(in);
      if (!in) throw std::runtime_error("input truncated");
      pcs::PropagatePlan P;
      pcs::DenseQueryPlan D;
      try {
        pcs::check_integral_atol(has_iatol ? iatol.data() : nullptr, NQ);
        P = pcs::build_propagate_plan(F, n_seg, seg.data());
        D = pcs::build_dense_query_plan(F.N, tau.data(), Q, Q ? query.data() : nullptr);
      } catch (const std::exception& e) {
        out << "case " << c << " refused\n";
        ++refused;
        continue;
      }
      // what the library holds: the staged queries and their order [Q], the slots [N + 1], the arrive columns [N], the
      // dense columns [Q]
      if ((long long)D.q_order.size() != Q || (long long)D.tau_sorted.size() != Q || (int)D.node_q0.size() != F.N + 1 || D.Q != Q)
        throw std::runtime_error("plan sizes");
      if (D.node_q0.at(0) != 0 || D.node_q0.at((size_t)F.N) != Q) throw std::runtime_error("the slots do not cover the queries");
      std::vector<int> arrived((size_t)F.N, 0), dense((size_t)Q, 0);
      auto answer = [&](int slot, double lo, double hi, bool at_start) {
        for (int k = D.node_q0.at((size_t)slot); k < D.node_q0.at((size_t)slot + 1); ++k) {
          const double t = D.tau_sorted.at((size_t)k);
          const int32_t col = D.q_order.at((size_t)k);
          if (t != query.at((size_t)col)) throw std::runtime_error("a sorted query is not the caller's");
          if (at_start ? t != lo : !(t > lo && t <= hi)) throw std::runtime_error("a query is not inside its slot");
          if (k > 0 && D.tau_sorted.at((size_t)k - 1) > t) throw std::runtime_error("the queries are not ascending");
          if (k > 0 && D.tau_sorted.at((size_t)k - 1) == t && D.q_order.at((size_t)k - 1) > col)
            throw std::runtime_error("the sort is not stable");
          ++dense.at((size_t)col);
        }
      };
      const int64_t lanes = P.blocks * P.TB;
      for (int64_t i = 0; i < lanes; ++i) {
        if (i >= P.n_seg) continue;   // the kernel's own guard
        const int j0 = P.seg_node.at((size_t)i), j1 = P.seg_node.at((size_t)i + 1);
        if (j0 == 0) {
          ++arrived.at(0);
          answer(0, tau.at(0), tau.at(0), true);
        }
        for (int j = j0; j < j1; ++j) {
          answer(j + 1, tau.at((size_t)j), tau.at((size_t)j + 1), false);
          ++arrived.at((size_t)j + 1);
        }
      }
      for (int a : arrived) if (a != 1) throw std::runtime_error("an arrive column is not written exactly once");
      for (int d : dense) if (d != 1) throw std::runtime_error("a dense column is not written exactly once");
      out << "case " << c << " ok " << F.N << ' ' << Q << '\n';
      put(out, "q_order", D.q_order);
      put(out, "node_q0", D.node_q0);
    }
    out << "refused " << refused << "\nok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "propagate_dense_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
