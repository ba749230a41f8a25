// CPU-only sanitizer harness for the host index arithmetic of the propagation kernel (TEST INFRASTRUCTURE).
//
// Compiles pc_propagate_plan.hpp (the checks of the segment list and of the tolerances, the first section of every
// segment, the grid) on top of pc_solution_plan.hpp under g++ -fsanitize=address,undefined, reads meshes and segment
// lists, builds every plan and walks every node, section boundary, coefficient slot and output column a lane of
// pc_sol_propagate would touch against the array sizes the library allocates, and prints the plan.
// tests/test_propagate_plan_sanitize.py compares it with a NumPy restatement.
//
//   usage: propagate_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case:  K n_orders n_seg substeps rtol max_steps NY | orders... | n_k[K] |
//           seg_nodes[n_seg + 1] | atol[NY]        (n_seg = 0: no segment list follows; rtol / atol may be nan or inf)
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
      int K = 0, n_orders = 0, NY = 0;
      long long n_seg = 0, substeps = 0, max_steps = 0;
      in >> K >> n_orders >> n_seg >> substeps;
      const double rtol = real(in);
      in >> max_steps >> NY;
      if (!in || K < 0 || n_orders < 0 || n_seg < 0 || NY < 0) throw std::runtime_error("bad case header");
      std::vector<int32_t> orders((size_t)n_orders), n_k((size_t)K), seg(n_seg > 0 ? (size_t)n_seg + 1 : 0);
      std::vector<double> atol((size_t)NY);
      for (auto& e : orders) in >> e;
      for (auto& e : n_k) in >> e;
      for (auto& e : seg) in >> e;
      for (auto& e : atol) e = real(in);
      if (!in) throw std::runtime_error("input truncated");
      const pcs::FitPlan F = pcs::build_fit_plan(K, n_k.data(), n_orders, orders.data(), NY, 1, 256, 0);
      pcs::PropagatePlan P;
      try {
        pcs::check_propagate_tolerances(substeps, rtol, atol.data(), NY, max_steps);
        P = pcs::build_propagate_plan(F, n_seg, seg.empty() ? nullptr : seg.data());
      } catch (const std::exception& e) {
        out << "case " << c << " refused\n";
        ++refused;
        continue;
      }
      // what the library holds: tau [N], sec_s / sec_tau [K + 1], coefficient rows [NC], node arrays and outputs [N],
      // the staged lists [n_seg + 1] / [n_seg], status [n_seg]
      std::vector<double> tau((size_t)F.N, 0.0), sec_tau((size_t)F.K + 1, 0.0), coef((size_t)F.NC, 0.0);
      std::vector<char> arrived((size_t)F.N, 0), status((size_t)P.n_seg, 0);
      if ((int64_t)P.seg_node.size() != n_seg + 1 || (int64_t)P.seg_sec.size() != n_seg) throw std::runtime_error("plan sizes");
      const int64_t lanes = P.blocks * P.TB;
      if (lanes < n_seg || lanes - n_seg >= P.TB) throw std::runtime_error("the grid does not cover the segments exactly");
      for (int64_t i = 0; i < lanes; ++i) {
        if (i >= P.n_seg) continue;   // the kernel's own guard
        const int j0 = P.seg_node.at((size_t)i), j1 = P.seg_node.at((size_t)i + 1);
        int k = P.seg_sec.at((size_t)i);
        if (j0 == 0) {
          if (arrived.at(0)) throw std::runtime_error("column 0 is written twice");
          arrived[0] = 1;
        }
        for (int j = j0; j < j1; ++j) {
          if (j >= F.sec_s.at((size_t)k + 1) && k < F.K - 1) ++k;
          const int sk = F.sec_s.at((size_t)k), n = F.sec_s.at((size_t)k + 1) - sk + 1;
          if (!(sk <= j && j < F.sec_s.at((size_t)k + 1))) throw std::runtime_error("an interval is not inside the lane's section");
          (void)sec_tau.at((size_t)k);
          (void)sec_tau.at((size_t)k + 1);
          (void)tau.at((size_t)j);
          (void)tau.at((size_t)j + 1);
          if (F.coef_off.at((size_t)k) != sk + k) throw std::runtime_error("coefficient offset");
          for (int m = 0; m < n; ++m) (void)coef.at((size_t)sk + k + m);
          if (arrived.at((size_t)j + 1)) throw std::runtime_error("a column is written twice");
          arrived[(size_t)j + 1] = 1;
        }
        status.at((size_t)i) = 1;
      }
      for (char a : arrived) if (!a) throw std::runtime_error("a column is never written");
      for (char s : status) if (!s) throw std::runtime_error("a segment has no status");
      out << "case " << c << " ok " << F.N << ' ' << P.n_seg << ' ' << P.blocks << ' ' << P.TB << '\n';
      put(out, "seg_node", P.seg_node);
      put(out, "seg_sec", P.seg_sec);
    }
    out << "refused " << refused << "\nok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "propagate_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
