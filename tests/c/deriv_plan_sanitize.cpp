// CPU-only sanitizer harness for the colouring plan of the derivative check (TEST INFRASTRUCTURE).
//
// Compiles pc_deriv.hpp (colours, located / sum / source flags, per-colour entry lists) together with the headers that
// build the patterns it reads (pc_desc.hpp, pc_pattern.hpp) under g++ -fsanitize=address,undefined, reads a problem
// description in the text format of pattern_sanitize.cpp, builds the plan and prints its arrays.
// tests/test_deriv_plan_sanitize.py compares them with the library's (pc_deriv_plan).
//
//   usage: deriv_plan_sanitize <in.txt> <out.txt>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "desc_reader.hpp"
#include "../../pycollo_amd/csrc/pc_deriv.hpp"

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

    pcp::Problem Q;
    pcp::from_desc(d, Q);
    pce::build_shape(d, Q, in_desc.knobs);
    const pcd::Plan P = pcd::build_plan(Q);
    // every list must address the patterns
    const int64_t nG = (int64_t)Q.g_row.size(), nH = (int64_t)Q.h_row.size();
    for (auto e : P.gl_ent) if (e < 0 || e >= nG || !P.g_flag[e]) throw std::runtime_error("located G entry out of range");
    for (auto e : P.seg_ent) if (e < 0 || e >= nG || P.g_flag[e]) throw std::runtime_error("sum term out of range");
    for (auto e : P.hl_ent) if (e < 0 || e >= nH || !P.h_flag[e]) throw std::runtime_error("located H entry out of range");
    for (auto c : P.cols) if (c < 0 || c >= Q.num_x) throw std::runtime_error("column out of range");
    if ((int64_t)P.gl_ent.size() + (int64_t)P.seg_ent.size() != nG) throw std::runtime_error("G entries lost");
    std::ofstream out(argv[2]);
    out << "sizes " << P.n_colours << ' ' << P.n_seg << ' ' << P.n_h_unlocated << '\n';
    put(out, "colour", P.colour);
    put(out, "g_flag", P.g_flag);
    put(out, "h_flag", P.h_flag);
    put(out, "j_flag", P.j_flag);
    out << "ok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "deriv_plan_sanitize: %s\n", e.what());
    return 1;
  }
}
