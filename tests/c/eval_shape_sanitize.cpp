// CPU-only sanitizer harness for the launch shape of the evaluation (TEST INFRASTRUCTURE).
//
// Compiles pc_eval_shape.hpp -- what pc_create decides before it needs a device -- with g++ -fsanitize=address,undefined,
// reads a descriptor in the text format of desc_reader.hpp, builds the shape, walks every table it produced against what
// the table indexes and prints the shape.  The LDS byte counts the rules compare (a workgroup's with 1, 2 and 4 staging
// regions; the worst phase's before the tiles exist, by tile capacity) are printed next to it: tests/test_eval_shape_cpu.py
// restates the rules on those numbers and must arrive at the same shape.  A descriptor the shape refuses prints
// "refused <message>".
//
//   usage: eval_shape_sanitize <in.txt> <out.txt>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "desc_reader.hpp"

namespace {

void require(bool ok, const char* what) {
  if (!ok) throw std::logic_error(std::string("walk: ") + what);
}

void walk(const pce::Shape& S, const pcp::Problem& Q) {
  const int64_t nG = (int64_t)Q.g_row.size(), nH = (int64_t)Q.h_row.size();
  size_t total = 0;
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    const auto& P = Q.ph[ip];
    const auto& D = S.ph[ip];
    require(D.n_tiles == (int)P.tile_k0.size() - 1 && D.n_tiles >= 1, "n_tiles");
    require(P.tile_k0.front() == 0 && P.tile_k0.back() == P.K, "tiles cover the mesh");
    for (int t = 0; t < D.n_tiles; ++t) {
      require(P.tile_k0[t] < P.tile_k0[t + 1], "empty tile");
      require(P.sec_s[P.tile_k0[t + 1]] - P.sec_s[P.tile_k0[t]] + 1 <= S.TB, "tile larger than its workgroup");
    }
    if (S.mixed) {
      require(S.trec_base[ip] == total, "trec_base");
      for (int t = 0; t < D.n_tiles; ++t) {
        require(S.trec_base[ip] + t < S.trec_all.size(), "trec_base past trec_all");
        const PcTileRec& r = S.trec_all[S.trec_base[ip] + t];
        const int k0 = P.tile_k0[t];
        require(r.phase == (int32_t)ip && r.tile == t && r.k0 == k0 && r.nsec == P.tile_k0[t + 1] - k0, "record's tile");
        require(r.n0 == P.sec_s[k0] && r.E0 == P.sec_E[k0], "record's place in the mesh");
        require(r.nprev == (k0 > 0 ? P.n_k[k0 - 1] : 0), "record's previous section");
        require(r.qa_prev >= 0 && r.qa_prev + (r.nprev ? (r.nprev - 1) * r.nprev : 0) <= S.qa_n, "record's A table");
        for (int k = k0; r.order > 0 && k < k0 + r.nsec; ++k) require(P.n_k[k] == r.order, "order-pure tile");
      }
    }
    total += (size_t)D.n_tiles;
    require(D.erec0 >= 0 && D.erec0 <= S.n_rec, "erec0");
  }
  require(S.trec_all.size() == (S.mixed ? total : 0), "trec_all");
  require(S.n_rec == (int32_t)S.rec_slot.size() && S.rec_slot.size() == S.rec_term.size(), "n_rec");
  for (size_t i = 0; i < S.rec_slot.size(); ++i) {
    require(S.rec_slot[i] >= 0 && S.rec_slot[i] < nH, "rec_slot outside the Hessian pattern");
    require(S.rec_term[i] >= 0 && (size_t)S.rec_term[i] < Q.pt_hslot.size(), "rec_term outside the endpoint entries");
    require(Q.pt_hslot[S.rec_term[i]] == S.rec_slot[i] && Q.pt_hlocal[S.rec_term[i]] < 0, "rec_term's entry");
  }
  // the packed blocks: every part on a 256-byte boundary, none overlapping the next
  for (size_t o : {S.o_lam, S.in_total, S.o_c, S.o_G, S.o_H, S.out_total}) require(o % 32 == 0, "block alignment");
  require(S.o_lam >= (size_t)Q.num_x && S.in_total >= S.o_lam + (size_t)Q.num_c, "input block");
  require(S.o_f == 0 && S.o_gn == 1 && S.o_c >= 1 + Q.jgrad_col.size(), "J | grad J");
  require(S.o_G >= S.o_c + (size_t)Q.num_c && S.o_H >= S.o_G + (size_t)nG && S.out_total >= S.o_H + (size_t)nH, "output block");
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
    std::ofstream out(argv[2]);
    {   // the worst phase's LDS bytes before the tiles exist: one region at the three block sizes, two by tile capacity
      pcp::Problem Q0;
      pcp::from_desc(d, Q0);
      for (auto& P : Q0.ph) pcp::finalize_phase_tables(P, Q0.n_s);
      auto need = [&](int tb, int tc, int W, bool uniform_only) {
        int mx = 0;
        for (auto& P : Q0.ph)
          if (!uniform_only || P.spec_orders.empty())
            mx = std::max(mx, pcp::phase_lds_bytes(P, tb, in_desc.qa_total, in_desc.qw_total, W * pcp::phase_lds_out(P, tc - 1, tc), P.compiled_order == 0));
        return mx;
      };
      out << "need1";
      for (int tb : {64, 128, 256}) out << ' ' << need(tb, tb, 1, false);
      out << "\nneed2";
      for (int tc = 2; tc <= 64; ++tc) out << ' ' << need(64, tc, 2, false);
      out << "\nneed2u";
      for (int tc = 2; tc <= 64; ++tc) out << ' ' << need(64, tc, 2, true);
      out << '\n';
    }
    pcp::Problem Q;
    pcp::from_desc(d, Q);
    pce::Shape S;
    try {
      S = pce::build_shape(d, Q, in_desc.knobs);
    } catch (const std::runtime_error& e) {
      out << "refused " << e.what() << '\n';
      return out ? 0 : 3;
    }
    out << "shape " << S.TB << ' ' << S.TC << ' ' << S.two_wave << ' ' << S.mixed << '\n';
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      const auto& D = S.ph[ip];
      out << "phase " << D.n_tiles;
      if (d.plan_only) { out << '\n'; continue; }
      out << ' ' << D.uni_n << ' ' << D.spt << ' ' << D.lds_out << ' ' << D.lds_out4 << ' ' << D.any_pure << ' ' << D.any_generic
          << ' ' << D.nfs << ' ' << D.wpt << ' ' << D.lds_bytes << ' ' << D.erec0 << '\n';
      out << "lds";
      for (int w : {1, 2, 4}) out << ' ' << pce::lds_bytes(S, D, Q.ph[ip], w);
      out << '\n';
      if (!Q.ph[ip].spec_orders.empty()) out << "caps " << Q.ph[ip].mix_cap_rows << ' ' << Q.ph[ip].min_run_rows << '\n';
    }
    if (d.plan_only) {
      out << "ok\n";
      return out ? 0 : 3;
    }
    walk(S, Q);
    out << "merged " << S.wpt_all << ' ' << S.lds_all << '\n';
    out << "tail " << S.lds_max << ' ' << S.lds_nred << ' ' << S.tail_lds_bytes << ' ' << S.heavy_point << ' ' << S.tail_blocks << ' '
        << S.tail_blocks_all << ' ' << S.tail_big << '\n';
    out << "carve " << Q.tail_owned.size() << ' ' << Q.point_x.size() << ' ' << Q.n_b << ' ' << Q.pthess_row.size() << '\n';
    out << "rec " << S.n_rec;
    for (size_t i = 0; i < S.rec_slot.size(); ++i) out << ' ' << S.rec_slot[i] << ':' << S.rec_term[i];
    out << '\n';
    out << "blocks " << S.o_lam << ' ' << S.in_total << ' ' << S.o_f << ' ' << S.o_gn << ' ' << S.o_c << ' ' << S.o_G << ' ' << S.o_H << ' '
        << S.out_total << '\n';
    out << "sizes " << Q.num_x << ' ' << Q.num_c << ' ' << Q.jgrad_col.size() << ' ' << Q.g_row.size() << ' ' << Q.h_row.size() << '\n';
    out << "ok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "eval_shape_sanitize: %s\n", e.what());
    return 1;
  }
}
