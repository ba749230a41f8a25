// The launch shape of the evaluation (pure C++, no device code: compiled into pc_engine.hip, and on its own under
// AddressSanitizer / UBSan by tests/c/eval_shape_sanitize.cpp): everything pc_create decides from the descriptor, the
// mesh and the PYCOLLO_AMD_* knobs before it needs a device pointer -- threads per block, tile capacity, which build of
// the tile kernels runs with how many waves per tile and how much LDS, the tail's carve and workgroups, the per-tile and
// edge records, the packed blocks' offsets -- and the descriptors it refuses.  Every threshold is a named constant with
// the measurement it came from next to it.  The environment and the device are read by the caller (Knobs).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <optional>
#include <stdexcept>
#include <vector>

#include "pc_args.h"
#include "pc_desc.hpp"
#include "pc_pattern.hpp"

namespace pce {

// Threads per block by the longest phase's node count when the descriptor leaves it open ...
constexpr int64_t TB128_MIN_NODES = 65536, TB256_MIN_NODES = 262144;
// ... but a one-state model has so little per node that the widest workgroup pays much earlier (hypersensitive, TB =
// 64 / 128 / 256: 20 k nodes 5.11 / 4.94-5.21 / 5.0-5.2 us, 30 k 5.46 / 5.41 / 5.18, 50 k 6.67 / 5.81 / 5.70,
// 65 k 8.92 / 6.76 / 5.90, 150 k 14.5 / 9.05 / 8.27, 250 k 22.1 / 12.1 / 9.97)
constexpr int64_t ONE_STATE_TB256_MIN_NODES = 25000;
// a model of more operations per node than this is "heavy": a wave that shares a tile re-evaluates the node functions
constexpr int HEAVY_EVAL_OPS = 4000;

// Few tiles and several states: W waves share a tile and split its output runs, so that the chip's 1024 SIMDs each
// hold a wave (or two) instead of a fraction of them holding one long-running wave.  Beyond that the replicas only add
// redundant node evaluations (measured on 64-node tiles, W = 1 / 2 / 4: shuttle 381 tiles 22.7 / 19.2 / 17.6 us, 953
// tiles 25.2 / 23.3 / 31.3 us, 2858 tiles 54 / 60 / 81 us).
// (one state: W = 2 measured no faster, 5.58 vs 5.49 us.  A heavy model -- Delta III, ~10k operations -- loses at 834
//  tiles, 358 / 410 / 522 us: every sharing wave re-evaluates the node functions)
constexpr int WPT4_MAX_TILES = 400, WPT2_MAX_TILES_HEAVY = 512, WPT2_MAX_TILES = 1024;

// The two-wave build of a heavy model (codegen: pc_bulk_all_r_w2 / pc_bulk_p<i>_r_w2, <= 256 registers): two waves
// share every 64-node tile, each with its own staging region, and a SIMD holds two of them -- if the CU's 160 KiB of
// LDS hold four tiles.  The tile capacity is the largest that allows it (Delta III, order 5: 60 rows of 40 doubles per
// replica; 4 x 12.5 k nodes 30.6 -> 23.2 us).
// With few tiles (a rank's share of a sharded mesh, a coarse mesh) four waves per tile serve better: one wave per SIMD
// either way, and the shorter one wins -- the build runs above this many 64-node tiles.
constexpr int64_t TWO_WAVE_MIN_TILES64 = 400;
// Four workgroups per CU: a quarter of the 160 KiB less two allocation granules of 1280 B -- measured, Delta III
// 4 x 12.5 k nodes: 37 272 B per workgroup 23.2 us, 39 832 B (nominally still a quarter) 26.8 us
constexpr int QUARTER_CU_LDS = 30 * 1280;
// A two-wave launch is one generation of waves and lasts one wave's life, which grows with the tile's rows (its share
// of the flush): the tile capacity is the one that cuts the mesh into about 896 tiles (3.5 workgroups per CU, 1 792 of
// the chip's 2 048 wave slots) when that is smaller than what the LDS allows.  Measured on one box, Delta III 4 x 12.5 k
// nodes, tiles / us: order 4  796 / 25.8, 928 / 22.3, 984 / 22.4;  order 5  896 / 23.2, 964 / 26.0;  order 6  836 / 32.1,
// 912 / 29.3, 1000 / 28.8;  order 7  836 / 31.4, 928 / 27.7;  order 8  796 / 35.7, 896 / 32.0, 1020 / 33.6
// (profiles/r04_two_wave_tiles.txt).
constexpr int64_t TWO_WAVE_TILES = 896;
// ... and every wave of the launch resident at once (2048 wave slots at two per SIMD): with smaller tiles than that
// allows, the one-wave-per-tile kernel -- itself two waves per SIMD -- is as fast or faster (Delta III order 6: 1160 tiles
// of 45 nodes x 2 waves 34.0 us, 872 tiles x 1 wave 32.2 us; 4 x 25 k nodes, order 5: 42.7 / 42.2 us)
constexpr int64_t TWO_WAVE_MAX_WAVES = 2048;
constexpr int TWO_WAVE_MIN_TC = 24;        // no smaller tile capacity from the tile target ...
constexpr int TWO_WAVE_MIN_TC_LDS = 32;    // ... or from the LDS budget
// Mixed build: a launch is one generation of waves and lasts as long as its slowest one: a tile of several orders runs
// the any-order body, which takes about twice as long per row as an order-specialised one -- such tiles are kept to
// half the rows so that they finish with the others (measured: with 63-row any-order tiles among 835 order-pure ones
// the mixed build ran no faster than the any-order kernel alone, 51.3 / 50.6 us)
constexpr int MIX_CAP_ROWS = 32, MIX_CAP_ROWS_MIN = 8;
// The endpoint block is generated in four parts, one per wave of a 256-thread tail; a small block (at most so many
// endpoint variables, constraints and Hessian entries) is not worth the three extra waves every tile's workgroup then
// carries (they exit at their first instruction)
constexpr size_t HEAVY_POINT_MIN = 17;
constexpr int TAIL_PARTS = 4;
// more than so many strides of partial sums per lane of a separate tail launch in some phase: pc_tail_big
constexpr int TAIL_BIG_STRIDES = 4;

// What the environment (PYCOLLO_AMD_TB, _WPT, _TILE_NODES, _TWO_WAVE, _TWO_WAVE_MAX_TILES, _TWO_WAVE_TILES,
// _TWO_WAVE_MAX_WAVES, _MIX_MIN_RUN_ROWS, _MIX_CAP_ROWS, _RESIDENT, _TAIL_BLOCKS, _MERGE; read in pc_engine.hip) and the
// device may set.  An empty optional is "not set": PYCOLLO_AMD_WPT and _TILE_NODES also switch the two-wave build off
// merely by being present.
struct Knobs {
  std::optional<int> tb;                 // threads per block, overrides the descriptor's (0: by the mesh)
  std::optional<int> wpt;                // waves per tile: 1, 2 or 4, anything else is ignored
  std::optional<int> tile_nodes;         // tile capacity, taken when in [largest section, TB]
  bool two_wave = true;                  // 0 turns the two-wave build off
  int64_t two_wave_max_tiles = 1 << 30;  // ... as do more 64-node tiles than this
  int64_t two_wave_tiles = TWO_WAVE_TILES;   // the tile count its capacity aims at (0: the largest tile the LDS allows)
  int64_t two_wave_max_waves = TWO_WAVE_MAX_WAVES;   // mixed build only
  std::optional<int> mix_min_run_rows;   // pcp::Phase::min_run_rows
  int mix_cap_rows = MIX_CAP_ROWS;
  bool resident = true;                  // 0: always two launches (bulk, then pc_tail)
  int tail_blocks = 0;                   // workgroups of the resident tail, at most TAIL_PARTS (0: by the endpoint block)
  bool merge = true;                     // several phases in one launch (pc_bulk_all)
  int lds_limit = 64 * 1024;             // dynamic LDS a workgroup may request (queried from the device)
};

struct PhaseShape {
  int n_tiles = 0;
  int uni_n = 0, spt = 0;             // uniform section order: index arithmetic replaces the section tables
  int lds_out = 0;                    // staging doubles per replica: the largest tile's runs
  int lds_out4 = 0;                   // ... of a four-wave launch (one pass per state: pc::bulk NPASS)
  bool any_pure = false, any_generic = false;   // mixed build: the tile bodies the phase's tiles run
  int nfs = 0;
  int wpt = 1;                        // waves (replicas) per 64-node tile, see pc::bulk
  int lds_bytes = 0;
  int32_t erec0 = 0;                  // resident tail: first record of this phase's edge-node Hessian entries
};

struct Shape {
  int TB = 64;
  int TC = 64;             // nodes a tile may hold (<= TB)
  bool two_wave = false;   // heavy model in the two-wave build: W = 2, tiles sized for four workgroups per CU
  bool mixed = false;      // some phase runs the mixed build: per-tile records pick the tile body
  bool resident = true;
  int lds_limit = 64 * 1024;
  int32_t qa_off[PC_MAX_ORDER + 1], qw_off[PC_MAX_ORDER + 1];   // order n's tables in the packed A / weight tables, or -1
  int qa_n = 0, qw_n = 0;                                        // their lengths
  std::vector<PhaseShape> ph;
  int wpt_all = 1, lds_all = 0;   // launch shape of pc_bulk_all (several phases)
  int lds_max = 0;
  int lds_nred = 0, tail_lds_bytes = 0;
  bool heavy_point = false;       // the endpoint block is worth one tail workgroup per part when tiles are single waves
  int tail_blocks = 1, tail_blocks_all = 1;   // resident tail's workgroups beside one phase's tiles / the merged launch's
  bool tail_big = false;          // a separate tail launch runs the build that overlaps the partial sums' loads
  std::vector<PcTileRec> trec_all;   // mixed build: records of every tile, phase after phase
  std::vector<size_t> trec_base;     // [n_phases] first record of each phase in trec_all
  std::vector<int64_t> rec_slot;     // [n_rec] H slot of every edge record
  std::vector<int32_t> rec_term;     // [n_rec] endpoint Hessian entry added to the record
  int32_t n_rec = 0;
  // Host-pointer calls stage through ONE packed input block [x~ | lambda] and ONE packed output block
  // [J | grad J non-zeros | c~ | G~ | H~]: offsets in doubles
  size_t o_lam = 0, in_total = 0;
  size_t o_f = 0, o_gn = 0, o_c = 0, o_G = 0, o_H = 0, out_total = 0;
};

// LDS bytes of a phase's workgroups with w staging regions: the larger of the tile bodies the phase's tiles run
inline int lds_bytes(const Shape& S, const PhaseShape& D, const pcp::Phase& P, int w) {
  const int out = (w == 4 ? D.lds_out4 : D.lds_out) * w;
  if (P.spec_orders.empty()) return pcp::phase_lds_bytes(P, S.TB, S.qa_n, S.qw_n, out, P.compiled_order == 0);
  int b = 0;
  if (D.any_generic) b = std::max(b, pcp::phase_lds_bytes(P, S.TB, S.qa_n, S.qw_n, out, true, true));
  if (D.any_pure) b = std::max(b, pcp::phase_lds_bytes(P, S.TB, S.qa_n, S.qw_n, out, false, true));
  return b;
}
// ... and of the launch that holds every phase's
inline int lds_bytes(const Shape& S, const pcp::Problem& Q, int w) {
  int mx = 0;
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) mx = std::max(mx, lds_bytes(S, S.ph[ip], Q.ph[ip], w));
  return mx;
}

// Waves per tile of a launch of `tiles` 64-node tiles whose models have at least n_y states; lds(w): its LDS bytes.
// `heavy` is the phase's own for its launch and "any phase" for the merged one; `one_state_rule` holds for a phase's
// launch only.
template <class Lds>
int pick_wpt(const Shape& S, const Knobs& kn, int n_y, bool heavy, int tiles, bool one_state_rule, Lds lds) {
  if (S.TB != 64) return 1;
  int w = 1;
  if (n_y >= 2 && tiles <= (heavy ? WPT2_MAX_TILES_HEAVY : WPT2_MAX_TILES)) w = 2;
  if (n_y >= 3 && tiles <= WPT4_MAX_TILES) w = 4;
  // One state, one launch per evaluation: the last tile's store phase is what the launch waits for once the tail runs
  // beside the tiles, and four waves get a tile's runs out sooner than one (hypersensitive, W = 1 / 2 / 4: 42 tiles
  // 4.69 / 4.34 / 4.25 us, 167 tiles 4.78-4.99 / 4.59-4.87 / 4.46-4.69, 334 tiles 5.94 / 5.00 / 4.94, 500 tiles
  // 5.92 / 5.29 / 5.44; with a separate tail launch W = 2 measured no gain, 5.58 vs 5.49 us)
  if (one_state_rule && n_y == 1 && !heavy && S.resident) w = tiles <= WPT4_MAX_TILES ? 4 : (tiles <= WPT2_MAX_TILES ? 2 : 1);
  if (kn.wpt && (*kn.wpt == 1 || *kn.wpt == 2 || *kn.wpt == 4)) w = *kn.wpt;
  if (S.two_wave) w = 2;
  while (w > 1 && lds(w) > S.lds_limit) w /= 2;
  return w;
}

// workgroups of the resident tail beside tiles of block_threads threads
inline int tail_blocks(const Shape& S, const Knobs& kn, int block_threads) {
  const int v = std::min(TAIL_PARTS, std::max(0, kn.tail_blocks));
  return v > 0 ? v : ((S.heavy_point && block_threads < 64 * TAIL_PARTS) ? TAIL_PARTS : 1);
}

// The shape of a handle for descriptor d, whose problem Q = from_desc(d) leaves with its tiles cut and, unless
// d.plan_only, its layout and patterns built.  Throws what pc_create refuses without a device.
inline Shape build_shape(const pc_problem_desc& d, pcp::Problem& Q, const Knobs& kn) {
  Shape S;
  S.resident = kn.resident;
  S.lds_limit = kn.lds_limit;
  S.ph.resize(Q.ph.size());
  // quadrature tables
  for (int i = 0; i <= PC_MAX_ORDER; ++i) S.qa_off[i] = S.qw_off[i] = -1;
  {
    size_t oa = 0, ow = 0;
    for (int i = 0; i < d.n_orders; ++i) {
      const int n = d.orders[i];
      if (n < 2 || n > PC_MAX_ORDER) throw std::runtime_error("quadrature order outside [2, 20]");
      S.qa_off[n] = (int32_t)oa;
      S.qw_off[n] = (int32_t)ow;
      oa += (size_t)(n - 1) * n;
      ow += n;
    }
    S.qa_n = (int)oa;
    S.qw_n = (int)ow;
  }
  const int qa_n = S.qa_n, qw_n = S.qw_n;
  // threads per block
  int64_t Nmax = 0, rows_total = 0, tiles64 = 0;
  int max_nk = 2;
  bool one_state = true, fixed = false;
  for (auto& P : Q.ph) {
    int64_t rows = 0;
    for (int k = 0; k < P.K; ++k) {
      rows += P.n_k[k] - 1;
      max_nk = std::max(max_nk, (int)P.n_k[k]);
    }
    Nmax = std::max(Nmax, rows + 1);
    rows_total += rows;
    tiles64 += (rows + 63) / 63;
    one_state = one_state && P.n_y == 1 && P.eval_ops <= HEAVY_EVAL_OPS;
    S.mixed = S.mixed || !P.spec_orders.empty();
    fixed = fixed || !P.fixed_tile_k0.empty();
  }
  int TB = kn.tb ? *kn.tb : d.threads_per_block;
  const bool auto_tb = (TB == 0);
  if (auto_tb) {
    TB = Nmax >= TB256_MIN_NODES ? 256 : (Nmax >= TB128_MIN_NODES ? 128 : 64);
    if (one_state && Nmax >= ONE_STATE_TB256_MIN_NODES) TB = 256;
  }
  if (TB != 64 && TB != 128 && TB != 256) throw std::runtime_error("threads_per_block must be 64, 128 or 256");
  for (auto& P : Q.ph) pcp::finalize_phase_tables(P, Q.n_s);
  // bytes of LDS a workgroup of W waves needs when tiles hold at most `tc` nodes (worst phase; before the tiles exist:
  // a tile of tc nodes has at most tc - 1 defect rows per state); uniform_only: of the phases of a single order
  auto lds_need = [&](int tb, int tc, int W, bool uniform_only = false) {
    int mx = 0;
    for (auto& P : Q.ph)
      if (!uniform_only || P.spec_orders.empty())
        mx = std::max(mx, pcp::phase_lds_bytes(P, W > 1 ? 64 : tb, qa_n, qw_n, W * pcp::phase_lds_out(P, tc - 1, tc), P.compiled_order == 0));
    return mx;
  };
  if (auto_tb)   // largest tile whose staging fits the dynamic LDS a module kernel may request
    while (TB > 64 && lds_need(TB, TB, 1) > S.lds_limit) TB /= 2;
  S.TB = TB;
  // Tile capacity in nodes (<= TB): a tile smaller than its workgroup leaves lanes idle but shortens every
  // wave's store phase and puts more waves on the chip -- what a problem with far fewer tiles than SIMDs wants.
  int TC = TB;
  // The two-wave build (above): for a code object that holds two such waves per SIMD, 64-thread tiles, models of two
  // states or more, and between TWO_WAVE_MIN_TILES64 and the caller's maximum of 64-node tiles -- with many more tiles than
  // the chip holds at once the replicas' second evaluation of the node functions buys nothing: the (split,
  // register-capped) one-wave-per-tile kernel already runs two waves per SIMD.  An explicit wpt / tile_nodes knob leaves
  // the choice to the caller.
  S.two_wave = d.two_wave_occupancy >= 2 && TB == 64 && !kn.wpt && !kn.tile_nodes && kn.two_wave &&
               tiles64 > TWO_WAVE_MIN_TILES64 && tiles64 <= kn.two_wave_max_tiles;
  for (auto& P : Q.ph) S.two_wave = S.two_wave && P.n_y >= 2;
  // the tile capacity that cuts the mesh into about kn.two_wave_tiles tiles, at most tc_max
  auto fill_tc = [&](int tc_max) {
    const int64_t want = kn.two_wave_tiles;
    if (want <= 0) return tc_max;
    const int per = (int)((rows_total + want - 1) / want);
    return std::max(std::max(max_nk, TWO_WAVE_MIN_TC), std::min(tc_max, per + 1));
  };
  // the largest tile capacity at which two staging regions fit a quarter CU
  auto quarter_cu_tc = [&](bool uniform_only) {
    int tc = 64;
    while (tc > std::max(max_nk, TWO_WAVE_MIN_TC_LDS) && lds_need(64, tc, 2, uniform_only) > QUARTER_CU_LDS) --tc;
    return tc;
  };
  if (S.mixed) {
    // Mixed build: tiles are cut per order (pc_pattern.hpp::build_tiles_mixed) under row caps that keep a workgroup's
    // LDS inside the budget -- a quarter CU for the two-wave build, else what a workgroup may request -- and the
    // two-wave build is kept when every wave of the launch is then resident at once, as for a uniform mesh.
    if (kn.mix_min_run_rows)
      for (auto& P : Q.ph) P.min_run_rows = std::max(1, *kn.mix_min_run_rows);
    auto cut = [&](int W, int budget) {
      int64_t tiles = 0;
      for (auto& P : Q.ph) {
        if (!P.spec_orders.empty()) {
          pcp::phase_set_caps(P, W > 1 ? 64 : TB, W, qa_n, qw_n, budget);
          P.mix_cap_rows = std::min(P.mix_cap_rows, std::max(MIX_CAP_ROWS_MIN, kn.mix_cap_rows));
        }
        pcp::build_tiles(P, TC);
        tiles += (int64_t)P.tile_k0.size() - 1;
      }
      return tiles;
    };
    if (S.two_wave) {
      // (phases of a single order inside a mixed problem: one tile capacity for them, as below)
      const int tc = quarter_cu_tc(true);
      bool fits = false;
      if (fixed) {   // the caller's tiles (a rank-local handle): two waves per tile when its actual tiles allow it
        TC = 64;
        const int64_t tiles = cut(2, QUARTER_CU_LDS);
        int need = 0;
        for (auto& P : Q.ph)
          if (!P.spec_orders.empty()) {
            bool ap = false, ag = false;
            const int out = 2 * pcp::phase_lds_out_tiles(P, &ap, &ag);
            if (ag) need = std::max(need, pcp::phase_lds_bytes(P, 64, qa_n, qw_n, out, true, true));
            if (ap) need = std::max(need, pcp::phase_lds_bytes(P, 64, qa_n, qw_n, out, false, true));
          }
        fits = need <= QUARTER_CU_LDS && lds_need(64, 64, 2, true) <= QUARTER_CU_LDS && 2 * tiles <= kn.two_wave_max_waves;
      }
      // the smallest tile capacity from the chip-filling one upwards whose cut keeps every wave resident
      for (int t = std::min(tc, fill_tc(tc)); !fixed && t <= tc && !fits; ++t) {
        TC = t;
        fits = lds_need(64, t, 2, true) <= QUARTER_CU_LDS && 2 * cut(2, QUARTER_CU_LDS) <= kn.two_wave_max_waves;
      }
      if (!fits) {
        S.two_wave = false;
        TC = TB;
      }
    }
    if (!S.two_wave) cut(1, S.lds_limit);
  } else if (S.two_wave) {
    const int tc = quarter_cu_tc(false);
    auto tiles_at = [&](int t) {   // tiles of whole sections of the phase's largest order
      int64_t tiles_tc = 0;
      for (auto& P : Q.ph) {
        int64_t N = 1, nmax = 2;
        for (int k = 0; k < P.K; ++k) { N += P.n_k[k] - 1; nmax = std::max<int64_t>(nmax, P.n_k[k]); }
        const int64_t per_tile = std::max<int64_t>(1, ((t - 1) / (nmax - 1)) * (nmax - 1));
        tiles_tc += (N - 1 + per_tile - 1) / per_tile;
      }
      return tiles_tc;
    };
    bool fits = false;
    if (lds_need(64, tc, 2) <= QUARTER_CU_LDS)
      for (int t = std::min(tc, fill_tc(tc)); t <= tc && !fits; ++t)
        if (2 * tiles_at(t) <= TWO_WAVE_MAX_WAVES) { TC = t; fits = true; }
    if (!fits) S.two_wave = false;
  }
  if (kn.tile_nodes && *kn.tile_nodes >= max_nk && *kn.tile_nodes <= TB) TC = *kn.tile_nodes;
  S.TC = TC;
  if (d.plan_only) {   // the tiling alone (a rank of the section-sharded evaluation asks for its range, sharding.py)
    pcp::build_all(Q, TC, true);
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) S.ph[ip].n_tiles = (int)Q.ph[ip].tile_k0.size() - 1;
    return S;
  }
  pcp::build_all(Q, TC);
  for (auto& P : Q.ph)
    for (int k = 0; k < P.K; ++k)
      if (S.qa_off[P.n_k[k]] < 0) throw std::runtime_error("no quadrature table for a section order in use");
  if (S.mixed) {   // one record per tile: which body runs it and where it sits in the mesh
    S.trec_base.assign(Q.ph.size(), 0);
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      auto& P = Q.ph[ip];
      S.trec_base[ip] = S.trec_all.size();
      for (size_t t = 0; t + 1 < P.tile_k0.size(); ++t) {
        PcTileRec r{};
        const int k0 = P.tile_k0[t];
        r.phase = (int32_t)ip;
        r.tile = (int32_t)t;
        r.order = t < P.tile_order.size() ? P.tile_order[t] : 0;
        r.k0 = k0;
        r.nsec = P.tile_k0[t + 1] - k0;
        r.n0 = P.sec_s[k0];
        r.nprev = k0 > 0 ? P.n_k[k0 - 1] : 0;
        r.qa_prev = r.nprev ? S.qa_off[r.nprev] : 0;
        r.E0 = P.sec_E[k0];
        r.w_prev = r.nprev ? d.quad_w[S.qw_off[r.nprev] + r.nprev - 1] : 0.0;
        S.trec_all.push_back(r);
      }
    }
  }
  if (Q.point_x.size() > PC_MAX_POINT || Q.n_b > PC_MAX_ENDPOINT_ROWS)
    throw std::runtime_error("too many endpoint variables / endpoint constraints for the tail kernel's argument block");
  if (Q.tail_owned.size() > PC_TAIL_OWNED_MAX)
    throw std::runtime_error("too many Hessian entries owned by the tail kernel (static parameters / endpoint terms)");
  S.heavy_point = Q.point_x.size() + (size_t)Q.n_b + Q.pthess_row.size() >= HEAVY_POINT_MIN;
  // the tail's LDS carve (pc::tail_lds): acc | part | sum | xb | lb | hold | hb
  for (auto& P : Q.ph) S.lds_nred = std::max(S.lds_nred, P.nred);
  S.tail_lds_bytes = 8 * (int)(Q.tail_owned.size() + 17 * (size_t)S.lds_nred + Q.point_x.size() + (size_t)Q.n_b +
                               2 * Q.pthess_row.size() + 2);
  int total = 0, min_ny = 1 << 30;
  bool any_heavy = false;
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    auto& P = Q.ph[ip];
    auto& D = S.ph[ip];
    D.n_tiles = (int)P.tile_k0.size() - 1;
    D.nfs = pcp::phase_nfs(P);
    bool same = true;
    for (int k = 0; k < P.K; ++k) same = same && P.n_k[k] == P.n_k[0];
    same = same && P.fixed_tile_k0.empty();   // (a caller's tile table is read from the tables, never computed from the tile index)
    D.uni_n = same ? P.n_k[0] : 0;
    D.spt = same ? (TC - 1) / (P.n_k[0] - 1) : 0;
    if (same && P.tile_k0.size() > 1 && P.tile_k0[1] != std::min(D.spt, P.K))
      throw std::runtime_error("internal error: uniform tiling mismatch");
    const int rows = pcp::phase_max_tile_rows(P);
    D.lds_out = pcp::phase_lds_out(P, rows, std::min(TC, rows + 1));
    D.lds_out4 = pcp::phase_lds_out(P, rows, std::min(TC, rows + 1), false);
    if (!P.spec_orders.empty()) {   // every row with its own order
      D.lds_out = pcp::phase_lds_out_tiles(P, &D.any_pure, &D.any_generic);
      D.lds_out4 = pcp::phase_lds_out_tiles(P, nullptr, nullptr, false);
    }
    const bool heavy = P.eval_ops > HEAVY_EVAL_OPS;
    D.wpt = pick_wpt(S, kn, P.n_y, heavy, D.n_tiles, true, [&](int w) { return lds_bytes(S, D, P, w); });
    D.lds_bytes = lds_bytes(S, D, P, D.wpt);
    S.lds_max = std::max(S.lds_max, D.lds_bytes);
    if (D.lds_bytes > S.lds_limit)
      throw std::runtime_error("tile needs more dynamic LDS than a workgroup may request; use a smaller "
                               "threads_per_block");
    if ((int)P.goff.size() > PC_MAX_GOFF || (int)P.hoff.size() > PC_MAX_HOFF)
      throw std::runtime_error("too many variables/constraints per phase for the kernel argument block");
    total += D.n_tiles;
    S.tail_big = S.tail_big || D.n_tiles > TAIL_BIG_STRIDES * PC_TAIL_THREADS;
    min_ny = std::min(min_ny, P.n_y);
    any_heavy = any_heavy || heavy;
  }
  // launch shape of the all-phases kernel: the phases share one workgroup size, chosen from the total tile count
  if (Q.ph.size() > 1) {
    S.wpt_all = pick_wpt(S, kn, min_ny, any_heavy, total, false, [&](int w) { return lds_bytes(S, Q, w); });
    S.lds_all = lds_bytes(S, Q, S.wpt_all);
  }
  S.tail_blocks = tail_blocks(S, kn, TB * S.ph[0].wpt);
  S.tail_blocks_all = tail_blocks(S, kn, TB * S.wpt_all);
  {
    // Resident tail: a Hessian entry of an edge node 0 / N-1 on which an endpoint term lands reaches the tail
    // workgroup as a record (two granules); the tail adds the term and stores the entry.  Records are numbered per
    // phase, node 0 then node N-1, in the kernels' site order (z-z entries, t strips, s strips) -- the order the
    // generated kernels rank their compile-time flags in (codegen.edge_flags, S<M>::erank).
    std::map<int64_t, int32_t> term_of_slot;   // slot -> endpoint entry
    for (size_t e = 0; e < Q.pt_hslot.size(); ++e)
      if (Q.pt_hlocal[e] < 0) term_of_slot.emplace(Q.pt_hslot[e], (int32_t)e);
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      auto& P = Q.ph[ip];
      const int NZ = P.n_z, NS = P.n_w, NHZZ = (int)P.hslot0.size(), NE = NHZZ + 2 * NZ + NS * NZ;
      S.ph[ip].erec0 = (int32_t)S.rec_slot.size();
      int found[2] = {0, 0};
      for (int edge = 0; edge < 2; ++edge) {
        const int64_t node = edge ? P.N - 1 : 0;
        for (int site = 0; site < NE; ++site) {
          int64_t slot = -1;
          if (site < NHZZ) {
            slot = edge ? P.hslotN[site] : P.hslot0[site];
          } else {
            const int64_t base = P.hoff[NZ + (site - NHZZ)];   // t strips (j, z) then s strips (l, z)
            if (base >= 0) slot = base + node;
          }
          auto it = slot >= 0 ? term_of_slot.find(slot) : term_of_slot.end();
          if (it == term_of_slot.end()) continue;
          S.rec_slot.push_back(slot);
          S.rec_term.push_back(it->second);
          term_of_slot.erase(it);
          ++found[edge];
        }
      }
      if (d.phases[ip].n_edge_rec[0] != found[0] || d.phases[ip].n_edge_rec[1] != found[1])
        throw std::runtime_error("the phase descriptor's edge-record counts do not match the Hessian pattern "
                                 "(codegen.edge_flags and pc_pattern.hpp disagree)");
    }
    if (!term_of_slot.empty())
      throw std::runtime_error("internal error: an endpoint Hessian term lands on an edge-node entry no tile produces");
    S.n_rec = (int32_t)S.rec_slot.size();
  }
  {
    // every part starts on a 256-byte boundary (what a separate allocation would give the kernels)
    auto up = [](size_t v) { return (v + 31) & ~(size_t)31; };
    S.o_lam = up(Q.num_x);
    S.in_total = S.o_lam + up(Q.num_c);
    S.o_f = 0;
    S.o_gn = 1;
    S.o_c = up(1 + Q.jgrad_col.size());
    S.o_G = S.o_c + up(Q.num_c);
    S.o_H = S.o_G + up(Q.g_row.size());
    S.out_total = S.o_H + up(Q.h_row.size());
  }
  return S;
}

}  // namespace pce
