// CPU-only sanitizer harness for the host index arithmetic of the dense output and of the mesh-error estimate (TEST
// INFRASTRUCTURE).
//
// Compiles pc_solution_plan.hpp (section-to-tile tables of the fit and mesh-error kernels, coefficient offsets, table
// offsets by order, LDS sizes, argument checks) under g++ -fsanitize=address,undefined, reads meshes, builds both plans
// of every mesh, walks every lane, every coefficient slot and every table row the kernels would touch against the array
// sizes the library allocates, and prints the plans.  tests/test_solution_plan_sanitize.py compares them with a NumPy
// restatement.
//
//   usage: solution_plan_sanitize <in.txt> <out.txt>
//   in.txt: n_cases, then per case:  K TB NY NU lds_limit n_orders | orders... | n_k[K]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../../pycollo_amd/csrc/pc_solution_plan.hpp"

namespace {

template <class T>
void put(std::ostream& out, const char* name, const std::vector<T>& v) {
  out << name << ' ' << v.size();
  for (const auto& e : v) out << ' ' << (long long)e;
  out << '\n';
}

// the mesh-error plan of one mesh: "mesh_error <c> refused <why>", or the plan after every lane of it has been walked
void mesh_error_case(std::ostream& out, int c, int K, const std::vector<int32_t>& n_k, const std::vector<int32_t>& orders, int NY,
                     int NU, int TB, int lds_limit) {
  pcs::MeshErrorPlan P;
  try {
    P = pcs::build_mesh_error_plan(K, n_k.data(), (int)orders.size(), orders.data(), NY, NU, TB, lds_limit);
  } catch (const std::exception& e) {
    out << "mesh_error " << c << " refused " << e.what() << '\n';
    return;
  }
  // what the library allocates: the tables [tab_total_BE] / [tab_total_A], per-lane LDS arrays [TB], the point's node
  // rows [N], the section maxima [K]
  std::vector<int32_t> sec_s((size_t)K + 1, 0);
  for (int k = 0; k < K; ++k) sec_s[(size_t)k + 1] = sec_s[(size_t)k] + n_k[(size_t)k] - 1;
  const int N = sec_s[(size_t)K] + 1;
  std::vector<double> tabBE((size_t)P.tab_total_BE, 0.0), tabA((size_t)P.tab_total_A, 0.0), node((size_t)N, 0.0);
  std::vector<char> lane_used((size_t)P.TB), section_done((size_t)K, 0);
  for (int t = 0; t < P.n_tiles(); ++t) {
    std::fill(lane_used.begin(), lane_used.end(), 0);
    const int k0 = P.tile_k0.at((size_t)t), k1 = P.tile_k0.at((size_t)t + 1);
    if (k1 <= k0) throw std::runtime_error("mesh error: empty tile");
    for (int k = k0; k < k1; ++k) {
      const int n = n_k.at((size_t)k), oBE = P.offBE[n], oA = P.offA[n];
      if (oBE < 0 || oA < 0) throw std::runtime_error("mesh error: no table for an order in use");
      for (int j = 0; j <= n; ++j) {   // the section's n + 1 nodes on the ph mesh
        const int lane = P.lane0.at((size_t)k) + j;
        if (lane_used.at((size_t)lane)) throw std::runtime_error("mesh error: two ph nodes on one lane");
        lane_used[(size_t)lane] = 1;
        if (j < n) (void)node.at((size_t)sec_s[(size_t)k] + j);                       // the lane's solution node
        if (j >= 1 && j < n)
          for (int i = 0; i < n; ++i) (void)tabBE.at((size_t)oBE + (size_t)(j - 1) * n + i);        // row j - 1 of B and E
        if (j >= 1)
          for (int i = 0; i <= n; ++i) (void)tabA.at((size_t)oA + (size_t)(j - 1) * (n + 1) + i);   // row j - 1 of A(n + 1)
      }
      if (section_done.at((size_t)k)) throw std::runtime_error("mesh error: a section is in two tiles");
      section_done[(size_t)k] = 1;
    }
  }
  for (char d : section_done) if (!d) throw std::runtime_error("mesh error: a section is in no tile");
  out << "mesh_error " << c << " ok " << P.n_tiles() << ' ' << P.tab_total_BE << ' ' << P.tab_total_A << ' ' << P.lds_bytes << '\n';
  put(out, "tile_k0", P.tile_k0);
  put(out, "lane0", P.lane0);
  put(out, "offBE", std::vector<int32_t>(P.offBE, P.offBE + PC_MAX_ORDER + 1));
  put(out, "offA", std::vector<int32_t>(P.offA, P.offA + PC_MAX_ORDER + 1));
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
      int K = 0, TB = 0, NY = 0, NU = 0, lds_limit = 0, n_orders = 0;
      in >> K >> TB >> NY >> NU >> lds_limit >> n_orders;
      if (!in || K < 0 || n_orders < 0) throw std::runtime_error("bad case header");
      std::vector<int32_t> orders((size_t)n_orders), n_k((size_t)K);
      for (auto& e : orders) in >> e;
      for (auto& e : n_k) in >> e;
      if (!in) throw std::runtime_error("input truncated");
      pcs::FitPlan P;
      try {
        P = pcs::build_fit_plan(K, n_k.data(), n_orders, orders.data(), NY, NU, TB, lds_limit);
      } catch (const std::exception& e) {
        out << "case " << c << " refused\n";
        mesh_error_case(out, c, K, n_k, orders, NY, NU, TB, lds_limit);
        continue;
      }
      // what the library allocates: node arrays [var][N], coefficient arrays [var][NC], a section tag per lane [TB],
      // the tables [tab_total]
      std::vector<char> lane_used((size_t)P.TB), node_owned((size_t)P.N, 0), coef_written((size_t)P.NC, 0);
      std::vector<double> tab((size_t)P.tab_total, 0.0);
      for (int t = 0; t < P.n_tiles(); ++t) {
        std::fill(lane_used.begin(), lane_used.end(), 0);
        const int k0 = P.tile_k0.at((size_t)t), k1 = P.tile_k0.at((size_t)t + 1);
        if (k1 <= k0) throw std::runtime_error("empty tile");
        for (int k = k0; k < k1; ++k) {
          const int n = P.sec_s.at((size_t)k + 1) - P.sec_s.at((size_t)k) + 1;
          if (n != n_k[(size_t)k]) throw std::runtime_error("sec_s does not give the section's order back");
          const int off = P.offC[n];
          if (off < 0) throw std::runtime_error("no table for an order in use");
          for (int j = 0; j < n; ++j) {
            const int lane = P.lane0.at((size_t)k) + j;
            if (lane_used.at((size_t)lane)) throw std::runtime_error("two nodes on one lane");
            lane_used[(size_t)lane] = 1;
            const int node = P.sec_s[(size_t)k] + j;
            if (j < n - 1 || k == P.K - 1) {
              if (node_owned.at((size_t)node)) throw std::runtime_error("a node has two owners");
              node_owned[(size_t)node] = 1;
            }
            const int slot = P.coef_off.at((size_t)k) + j;
            if (coef_written.at((size_t)slot)) throw std::runtime_error("a coefficient slot is written twice");
            coef_written[(size_t)slot] = 1;
            for (int i = 0; i < n; ++i) (void)tab.at((size_t)off + (size_t)j * n + i);   // row j of the n x n table
          }
        }
      }
      for (char o : node_owned) if (!o) throw std::runtime_error("a node has no owner");
      for (char w : coef_written) if (!w) throw std::runtime_error("a coefficient slot is never written");
      if (P.coef_off.at((size_t)P.K) != P.NC) throw std::runtime_error("coefficient offsets do not end at NC");
      // section boundaries from node abscissae: tau_i = i (increasing) must pass, a repeated boundary must not
      std::vector<double> tau((size_t)P.N);
      for (int i = 0; i < P.N; ++i) tau[(size_t)i] = (double)i;
      const std::vector<double> e = pcs::section_edges(P, tau.data());
      if ((int)e.size() != P.K + 1 || e.back() != (double)(P.N - 1)) throw std::runtime_error("section edges");
      out << "case " << c << " ok " << P.N << ' ' << P.NC << ' ' << P.n_tiles() << ' ' << P.tab_total << ' ' << P.lds_bytes << '\n';
      put(out, "tile_k0", P.tile_k0);
      put(out, "lane0", P.lane0);
      put(out, "sec_s", P.sec_s);
      put(out, "coef_off", P.coef_off);
      put(out, "offC", std::vector<int32_t>(P.offC, P.offC + PC_MAX_ORDER + 1));
      mesh_error_case(out, c, K, n_k, orders, NY, NU, TB, lds_limit);
    }
    // the argument checks of the sampling calls
    int refused = 0;
    const double one = 1.0;
    static const double* q = nullptr;
    q = &one;
    refused += expect_throw([] { pcs::check_sample_args(2, 2, q, 1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, -1, q, 1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, q, -1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, nullptr, 1, 0); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, q, 1, 4); });
    refused += expect_throw([] { pcs::check_sample_args(2, 0, q, (int64_t)INT32_MAX * 256 + 1, 0); });
    pcs::check_sample_args(2, 1, q, 1, PC_SOL_TAU | PC_SOL_EXTRAPOLATE);
    pcs::check_sample_args(2, 0, nullptr, 0, 0);
    pcs::check_sample_args(2, 0, q, (int64_t)INT32_MAX * 256, 0);
    if (pcs::sample_blocks(1, 256) != 1 || pcs::sample_blocks(256, 256) != 1 || pcs::sample_blocks(257, 256) != 2 ||
        pcs::sample_blocks((int64_t)INT32_MAX * 256, 256) != INT32_MAX)
      throw std::runtime_error("sample_blocks");
    out << "refused " << refused << "\nok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "solution_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
