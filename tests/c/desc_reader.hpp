// The text form of a problem descriptor (TEST INFRASTRUCTURE): what tests/test_sanitized_host.py::_serialise writes and
// the CPU harnesses under tests/c/ read.  A header line, the phases, the endpoint lists, then the line of the launch
// shape's inputs: two_wave_occupancy, threads_per_block, plan_only, the quadrature orders and weights, every phase's
// eval_ops and n_edge_rec, and the knobs (pc_eval_shape.hpp::Knobs; "set value" pairs for those that may be unset).
#pragma once
#include <cstdint>
#include <istream>
#include <stdexcept>
#include <vector>

#include "../../pycollo_amd/csrc/pc_eval_shape.hpp"

namespace desc_reader {

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

// a descriptor and the arrays it points into
struct DescIn {
  pc_problem_desc d{};
  pce::Knobs knobs;
  int qa_total = 0, qw_total = 0;
  std::vector<pc_phase_desc> phases;
  std::vector<PhaseIn> store;
  std::vector<int32_t> pp, pk, pi, jg, br, bc, phr, phc, orders;
  std::vector<double> quad_A, quad_w;
};

inline void read_optional(std::istream& in, std::optional<int>& dst) {
  int set = 0, v = 0;
  in >> set >> v;
  if (set) dst = v;
}

inline void read_desc(std::istream& in, DescIn& D) {
  pc_problem_desc& d = D.d;
  in >> d.n_phases >> d.n_s >> d.n_point >> d.n_b >> d.n_jgrad >> d.n_bjac >> d.n_pthess >> D.qa_total >> D.qw_total;
  if (!in || d.n_phases < 1 || d.n_phases > PC_MAX_PHASES) throw std::runtime_error("bad header");
  D.phases.assign((size_t)d.n_phases, pc_phase_desc{});
  D.store.resize((size_t)d.n_phases);
  for (int ip = 0; ip < d.n_phases; ++ip) {
    pc_phase_desc& s = D.phases[ip];
    PhaseIn& a = D.store[ip];
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
  d.phases = D.phases.data();
  D.pp = read_vec<int32_t>(in, d.n_point); D.pk = read_vec<int32_t>(in, d.n_point); D.pi = read_vec<int32_t>(in, d.n_point);
  D.jg = read_vec<int32_t>(in, d.n_jgrad);
  D.br = read_vec<int32_t>(in, d.n_bjac); D.bc = read_vec<int32_t>(in, d.n_bjac);
  D.phr = read_vec<int32_t>(in, d.n_pthess); D.phc = read_vec<int32_t>(in, d.n_pthess);
  d.point_phase = D.pp.data(); d.point_kind = D.pk.data(); d.point_idx = D.pi.data();
  d.jgrad_col = D.jg.data(); d.bjac_row = D.br.data(); d.bjac_col = D.bc.data();
  d.pthess_row = D.phr.data(); d.pthess_col = D.phc.data();
  d.device = -1;
  // the launch shape's inputs
  in >> d.two_wave_occupancy >> d.threads_per_block >> d.plan_only >> d.n_orders;
  if (!in || d.n_orders < 0 || d.n_orders > PC_MAX_ORDER) throw std::runtime_error("bad shape line");
  D.orders = read_vec<int32_t>(in, d.n_orders);
  D.quad_w = read_vec<double>(in, D.qw_total);
  D.quad_A.assign((size_t)D.qa_total, 0.0);   // (the shape reads no A table)
  d.orders = D.orders.data(); d.quad_A = D.quad_A.data(); d.quad_w = D.quad_w.data();
  for (auto& s : D.phases) in >> s.eval_ops >> s.n_edge_rec[0] >> s.n_edge_rec[1];
  pce::Knobs& kn = D.knobs;
  int two_wave = 1, resident = 1, merge = 1;
  read_optional(in, kn.tb);
  read_optional(in, kn.wpt);
  read_optional(in, kn.tile_nodes);
  in >> two_wave >> kn.two_wave_max_tiles >> kn.two_wave_tiles >> kn.two_wave_max_waves;
  read_optional(in, kn.mix_min_run_rows);
  in >> kn.mix_cap_rows >> resident >> kn.tail_blocks >> merge >> kn.lds_limit;
  if (!in) throw std::runtime_error("bad shape line");
  kn.two_wave = two_wave != 0; kn.resident = resident != 0; kn.merge = merge != 0;
}

}  // namespace desc_reader
