// CPU-only sanitizer harness for the host side of the C ABI (TEST INFRASTRUCTURE).
//
// Compiles the SAME headers the library's pc_create runs -- pc_desc.hpp (descriptor -> pcp::Problem, LDS sizing),
// pc_eval_shape.hpp (the launch shape: pce::build_shape, which cuts the tiles) and pc_pattern.hpp (mesh prefix tables, tiles,
// NLP layout, CSR patterns of G and H, producer-slot tables: ~600 lines of index arithmetic) -- with g++
// -fsanitize=address,undefined, reads a problem description as text (desc_reader.hpp), builds everything and prints the
// index arrays.  tests/test_sanitized_host.py feeds it the descriptors the library gets and compares
// its output with the library's (sanitizer builds on the CPU only; GPU ASan / XNACK are not
// available on the pool).
//
//   usage: pattern_sanitize <in.txt> <out.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "desc_reader.hpp"

namespace {

template <class T>
void put(std::ostream& out, const char* name, const std::vector<T>& v) {
  out << name << ' ' << v.size();
  for (const auto& e : v) out << ' ' << (long long)e;
  out << '\n';
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
    desc_reader::DescIn in_desc;
    desc_reader::read_desc(in, in_desc);
    const pc_problem_desc& d = in_desc.d;

    // what pc_create does on a structure-only handle
    pcp::Problem Q;
    pcp::from_desc(d, Q);
    const pce::Shape S = pce::build_shape(d, Q, in_desc.knobs);
    const int tile_nodes = S.TC, qa_total = S.qa_n, qw_total = S.qw_n;

    std::ofstream out(argv[2]);
    out << "sizes " << Q.num_x << ' ' << Q.num_c << ' ' << Q.g_row.size() << ' ' << Q.h_row.size() << '\n';
    put(out, "g_row", Q.g_row); put(out, "g_col", Q.g_col); put(out, "h_row", Q.h_row); put(out, "h_col", Q.h_col);
    put(out, "g_indptr", Q.g_indptr); put(out, "h_indptr", Q.h_indptr);
    put(out, "tail_owned", Q.tail_owned);
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      const auto& P = Q.ph[ip];
      put(out, "tile_k0", P.tile_k0);
      put(out, "tile_order", P.tile_order);
      if (!P.spec_orders.empty()) {   // the exact staging size of the tiles as cut, row groups included, in both forms
        bool ap = false, ag = false;
        std::vector<int> m = {pcp::phase_lds_out_tiles(P, &ap, &ag), pcp::phase_lds_out_tiles(P, nullptr, nullptr, false), (int)ap, (int)ag};
        for (int n = 2; n <= PC_MAX_ORDER; ++n) m.push_back(pc_row_passes(n, pcp::phase_max_row_len(P, n)));
        put(out, "mixed", m);
      }
      put(out, "goff", P.goff); put(out, "hoff", P.hoff); put(out, "hslot0", P.hslot0); put(out, "hslotN", P.hslotN);
      const int rows = pcp::phase_max_tile_rows(P);
      const int lds_out = pcp::phase_lds_out(P, rows, std::min(tile_nodes, rows + 1));
      std::vector<int> lds = {rows, lds_out};
      for (int W : {1, 2, 4}) lds.push_back(pcp::phase_lds_bytes(P, 64, qa_total, qw_total, lds_out * W, P.compiled_order == 0));
      put(out, "lds", lds);
      // every slot table entry must address the pattern
      for (auto v : P.hslot0) if (v < 0 || v >= (int64_t)Q.h_row.size()) throw std::runtime_error("hslot0 out of range");
      for (auto v : P.hslotN) if (v < 0 || v >= (int64_t)Q.h_row.size()) throw std::runtime_error("hslotN out of range");
    }
    out << "ok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pattern_sanitize: %s\n", e.what());
    return 1;
  }
}
