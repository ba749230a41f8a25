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

#include "../../pycollo_amd/csrc/pc_desc.hpp"
#include "../../pycollo_amd/csrc/pc_deriv.hpp"

namespace {

template <class T>
std::vector<T> read_vec(std::istream& in, long n) {
  std::vector<T> v((size_t)(n > 0 ? n : 0));
  for (auto& e : v)
    if (!(in >> e)) throw std::runtime_error("input truncated");
  return v;
}

struct PhaseIn {
  std::vector<int32_t> n_k, jr, jc, hr, hc, wk, wi, fk, fo;
  std::vector<double> h_k;
};

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
    pc_problem_desc d{};
    int tile_nodes = 0, qa_total = 0, qw_total = 0;
    in >> d.n_phases >> d.n_s >> d.n_point >> d.n_b >> d.n_jgrad >> d.n_bjac >> d.n_pthess >> tile_nodes >> qa_total >> qw_total;
    if (!in || d.n_phases < 1 || d.n_phases > PC_MAX_PHASES) throw std::runtime_error("bad header");
    std::vector<pc_phase_desc> phases((size_t)d.n_phases);
    std::vector<PhaseIn> store((size_t)d.n_phases);
    for (int ip = 0; ip < d.n_phases; ++ip) {
      pc_phase_desc& s = phases[ip];
      PhaseIn& a = store[ip];
      s = pc_phase_desc{};
      in >> s.n_y >> s.n_u >> s.n_q >> s.n_p >> s.t0_free >> s.tF_free >> s.K >> s.n_jac >> s.n_hess >> s.n_w >> s.compiled_order;
      // mixed build: the orders with a tile body; a caller's tile table (pc_phase_desc::fixed_tile_k0 / fixed_tile_order)
      in >> s.n_spec >> s.spec_orders[0] >> s.spec_orders[1] >> s.spec_orders[2] >> s.spec_orders[3] >> s.n_fixed_tiles;
      if (!in) throw std::runtime_error("bad phase header");
      a.n_k = read_vec<int32_t>(in, s.K);
      a.h_k = read_vec<double>(in, s.K);
      a.jr = read_vec<int32_t>(in, s.n_jac);
      a.jc = read_vec<int32_t>(in, s.n_jac);
      a.hr = read_vec<int32_t>(in, s.n_hess);
      a.hc = read_vec<int32_t>(in, s.n_hess);
      a.wk = read_vec<int32_t>(in, s.n_w);
      a.wi = read_vec<int32_t>(in, s.n_w);
      a.fk = read_vec<int32_t>(in, s.n_fixed_tiles > 0 ? s.n_fixed_tiles + 1 : 0);
      a.fo = read_vec<int32_t>(in, s.n_fixed_tiles > 0 ? s.n_fixed_tiles : 0);
      s.fixed_tile_k0 = s.n_fixed_tiles > 0 ? a.fk.data() : nullptr;
      s.fixed_tile_order = s.n_fixed_tiles > 0 ? a.fo.data() : nullptr;
      s.n_k = a.n_k.data(); s.h_k = a.h_k.data();
      s.jac_row = a.jr.data(); s.jac_col = a.jc.data();
      s.hess_row = a.hr.data(); s.hess_col = a.hc.data();
      s.w_kind = s.n_w > 0 ? a.wk.data() : nullptr;
      s.w_idx = s.n_w > 0 ? a.wi.data() : nullptr;
      s.bulk_kernel = "pc_bulk";
    }
    d.phases = phases.data();
    auto pp = read_vec<int32_t>(in, d.n_point), pk = read_vec<int32_t>(in, d.n_point), pi = read_vec<int32_t>(in, d.n_point);
    auto jg = read_vec<int32_t>(in, d.n_jgrad);
    auto br = read_vec<int32_t>(in, d.n_bjac), bc = read_vec<int32_t>(in, d.n_bjac);
    auto phr = read_vec<int32_t>(in, d.n_pthess), phc = read_vec<int32_t>(in, d.n_pthess);
    d.point_phase = pp.data(); d.point_kind = pk.data(); d.point_idx = pi.data();
    d.jgrad_col = jg.data(); d.bjac_row = br.data(); d.bjac_col = bc.data();
    d.pthess_row = phr.data(); d.pthess_col = phc.data();
    d.device = -1;

    pcp::Problem Q;
    pcp::from_desc(d, Q);
    for (auto& P : Q.ph) pcp::finalize_phase_tables(P, Q.n_s);
    pcp::build_all(Q, tile_nodes);
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
