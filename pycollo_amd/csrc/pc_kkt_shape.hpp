// The launch shape of the KKT solver (pure C++, no device code: compiled into pc_kkt.hip, and on its own under
// AddressSanitizer / UBSan by tests/c/kkt_shape_sanitize.cpp): everything pc_kkt_create decides from the descriptor and
// the PYCOLLO_AMD_KKT_* knobs before it needs a device pointer -- the derived index tables, which build of every kernel
// runs with how much LDS, the level lists of the chain's cyclic reduction, the length of every scratch buffer -- and the
// descriptors it refuses.  Integer arithmetic only; the environment is read by the caller (Knobs).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/pycollo_amd.h"
#include "pc_kkt_cr.hpp"

namespace pck {

// rows of the product with more than MV_LONG entries are cut into chunks of MV_CHUNK, a workgroup each (kkt_matvec_long)
constexpr int MV_LONG = 256, MV_CHUNK = 1024;

// Bytes of LDS, as the kernels' dynamic sizes are held against them (constants, not a device query: they decide which
// build runs):
constexpr int64_t LDS_BLOCK_MAX = 64000;    // a whole block staged next to its vectors: a leaf (kkt_leaf_factor / _forward), a
                                            // chain node's panel (kkt_chain_factor), a node of the cyclic reduction
constexpr int64_t LDS_VECTORS_MAX = 60000;  // the staging vectors alone, which every build needs: above it the descriptor is refused
constexpr int64_t LDS_WORKGROUP = 65536;    // what the waves of kkt_cr_top's one workgroup share

// what the environment may set (PYCOLLO_AMD_KKT_RESID_TOL, _LEAF_FWD_LDS, _LEAF_WAVES, _CR, _CR_TOP), read in pc_kkt.hip
struct Knobs {
  // a refined solve stops once ||rhs - K x||_2 <= resid_tol ||rhs||_2 (IPOPT: residual_ratio_max = 1e-10 on its own ratio).
  // Config 2, per interior-point iteration: no test 1.40 ms and 3.9 back-substitutions, 1e-12 1.03 ms with the objective
  // unchanged in all ten printed digits, 1e-11 1.06 ms (objective moves in the 8th digit), 1e-9 0.95 ms
  // (profiles/r04_ipm_iter_time.txt)
  double resid_tol = 1e-12;
  int leaf_fwd = -1;      // kkt_leaf_forward's staging (0 / 1 / 2); -1: by the leaf count
  // four waves per leaf: 0.246 -> 0.221 ms per factorisation at config 2, 0.644 -> 0.594 at config 3 against two (the
  // trailing update of a pivot step is the parallel part); one wave with LDS-only ordering 0.30 / 0.75, six or eight waves
  // no better than four and 4 % worse on the shuttle's blocks (profiles/r04_ipm_iter_time.txt)
  int leaf_waves = 4;     // waves per leaf of kkt_leaf_factor, 1 .. 16
  bool cr = true;         // the chain by cyclic reduction where its blocks allow it
  int cr_top_cap = -1;    // at most so many waves for kkt_cr_top (0 / 1: off); -1: no cap
};

// kkt_cr_top's argument: the trailing levels one workgroup runs
struct CrTop {
  int64_t ptr[18];     // level offsets into cr_nodes: levels [0, n) of the fused range
  int32_t n;
  int32_t wave_bytes;  // LDS per wave: the level kernels' dynamic size + the pull tables
};

struct Shape {
  Knobs knobs;
  int64_t n_leaf = 0, n_chain = 0, nb = 0;
  // derived tables
  std::vector<uint8_t> chain_last;
  std::vector<int64_t> leaf_of_left, leafG_off, chainG_off;
  std::vector<uint32_t> mv_src;                                      // kind << 30 | index of every matvec entry
  std::vector<int64_t> mv_long, mv_long_c0, mv_chunk_e0, mv_chunk_e1;   // rows with more than MV_LONG entries, cut into chunks
  int64_t n_mv_long = 0, n_mv_chunks = 0;
  // dynamic LDS of the launches, bytes
  int lds_leaf = 0, lds_chain = 0, lds_border = 0;
  int lds_leaf_full = 0;      // the leaf factorisation: the largest leaf block that fits, plus its staging vectors
  int lds_chain_factor = 0;
  int32_t chain_lds = 0, nzmax = 1, wcmax = 1;   // (KArgs)
  // the chain by cyclic reduction: one launch per level
  CrPlan cr;
  bool chain_cr = false;
  std::vector<int64_t> cr_lvl_ptr;   // nodes of level l: cr_nodes[cr_lvl_ptr[l-1] .. cr_lvl_ptr[l])
  std::vector<int64_t> cr_nodes;
  size_t cr_top_from = 0;            // levels [cr_top_from, cr_lvl_ptr.size()) run in one launch (kkt_cr_top); = size(): none
  int cr_top_waves = 0, cr_top_lds = 0;
  CrTop cr_top{};
  int lds_cr = 0;
  bool any_export = false;
  std::vector<int64_t> export_nodes;    // chain nodes that are not eliminated (a rank's shared nodes), ascending
  int border_blocks = 0;                // workgroups that sum the border terms (wide borders only); 0: the border kernel's own walk
  // lengths of the scratch buffers (elements)
  int64_t n_vals = 0, n_vec = 0, n_counts = 0, n_leafG = 1, n_chainG = 1, n_mv_long_part = 1, n_crbuf = 0, n_border_part = 0;
  static constexpr int64_t n_norm_part = 4 * 256, n_norm = 4;
};

// kkt_leaf_forward's staging for a solve
// (two waves and the leaf in LDS: pc_kkt_solve 0.199 -> 0.183 ms at config 2, 0.425 -> 0.410 at config 3; with the shuttle's
//  6 000 leaves the LDS costs occupancy and the solve got slower, 0.63 -> 0.65-0.71: staged up to 4 096 leaves)
inline int leaf_forward_stage(const Shape& s) { return s.knobs.leaf_fwd >= 0 ? s.knobs.leaf_fwd : (s.n_leaf <= 4096 ? 2 : 0); }

// pc_kkt_info of a handle with this shape; leaf_forward_stage: what its last forward elimination ran (-1: none yet)
inline void fill_info(const Shape& s, int leaf_forward_stage, pc_kkt_info* info) {
  std::memset(info, 0, sizeof(*info));
  info->n_leaf = s.n_leaf;
  info->n_chain = s.n_chain;
  info->nb = s.nb;
  info->n_mv_long = s.n_mv_long;
  info->chain_cr = s.chain_cr ? 1 : 0;
  info->cr_levels = s.chain_cr ? (int32_t)s.cr_lvl_ptr.size() - 1 : 0;
  info->cr_top_levels = s.chain_cr ? s.cr_top.n : 0;
  info->cr_top_waves = s.chain_cr ? s.cr_top_waves : 0;
  info->border_blocks = s.border_blocks;
  info->leaf_forward_stage = leaf_forward_stage;
  info->leaf_waves = s.knobs.leaf_waves;
}

inline Shape build_shape(const pc_kkt_desc& d, const Knobs& knobs) {
  Shape s;
  s.knobs = knobs;
  s.n_leaf = d.n_leaf;
  s.n_chain = d.n_chain;
  s.nb = d.nb;
  // the product: kind and index in one word, the long rows listed and cut into chunks
  s.mv_src.resize((size_t)d.n_mv);
  for (int64_t e = 0; e < d.n_mv; ++e) {
    if (d.mv_idx[e] < 0 || d.mv_idx[e] >= (1 << 30) || d.mv_kind[e] < 0 || d.mv_kind[e] > 2)
      throw std::runtime_error("matvec table entry out of range");
    s.mv_src[(size_t)e] = ((uint32_t)d.mv_kind[e] << 30) | (uint32_t)d.mv_idx[e];
  }
  s.mv_long_c0.assign(1, 0);
  for (int64_t r = 0; r < d.nu; ++r)
    if (d.mv_ptr[r + 1] - d.mv_ptr[r] > MV_LONG) {
      s.mv_long.push_back(r);
      for (int64_t e = d.mv_ptr[r]; e < d.mv_ptr[r + 1]; e += MV_CHUNK) {
        s.mv_chunk_e0.push_back(e);
        s.mv_chunk_e1.push_back(std::min<int64_t>(e + MV_CHUNK, d.mv_ptr[r + 1]));
      }
      s.mv_long_c0.push_back((int64_t)s.mv_chunk_e0.size());
    }
  s.n_mv_long = (int64_t)s.mv_long.size();
  s.n_mv_chunks = (int64_t)s.mv_chunk_e0.size();
  s.n_mv_long_part = std::max<int64_t>(1, s.n_mv_chunks);
  // derived tables
  s.chain_last.assign((size_t)d.n_chain, 0);
  for (int64_t p = 0; p < d.n_phase; ++p) s.chain_last[(size_t)(d.chain_phase_ptr[p + 1] - 1)] = 1;
  s.leaf_of_left.assign((size_t)d.n_chain, -1);
  s.leafG_off.resize((size_t)d.n_leaf);
  s.chainG_off.resize((size_t)d.n_chain);
  int64_t og = 0, mmax = 1, wmax = 1, nzmax = 1, wcmax = 1, want = 0;
  for (int64_t l = 0; l < d.n_leaf; ++l) {
    const int64_t left = d.leaf_left[l];
    s.leaf_of_left[(size_t)left] = l;
    const int64_t m = d.leaf_ptr[l + 1] - d.leaf_ptr[l];
    const int64_t w = (d.chain_ptr[left + 1] - d.chain_ptr[left]) + (d.chain_ptr[left + 2] - d.chain_ptr[left + 1]) + d.nb;
    s.leafG_off[(size_t)l] = og;
    og += w;
    mmax = std::max(mmax, m);
    wmax = std::max(wmax, w);
    const int64_t need = 8 * (m * (m + w) + 2 * m + w + 2);   // the leaf's block and its staging vectors
    if (need <= LDS_BLOCK_MAX) want = std::max(want, need);
  }
  s.n_leafG = std::max<int64_t>(1, og);
  og = 0;
  for (int64_t c = 0; c < d.n_chain; ++c) {
    const bool last = s.chain_last[(size_t)c] != 0;
    const int64_t nz = d.chain_ptr[c + 1] - d.chain_ptr[c];
    const int64_t nx = last ? 0 : d.chain_ptr[c + 2] - d.chain_ptr[c + 1];
    if (!last && s.leaf_of_left[(size_t)c] < 0) throw std::runtime_error("chain node without a leaf on its right");
    s.chainG_off[(size_t)c] = og;
    og += nx + d.nb;
    nzmax = std::max(nzmax, nz);
    wcmax = std::max(wcmax, nx + d.nb);
  }
  s.n_chainG = std::max<int64_t>(1, og);
  s.lds_leaf = (int)(8 * (2 * mmax + wmax + 2));
  s.lds_leaf_full = (int)std::max<int64_t>(want, s.lds_leaf);
  s.lds_chain = (int)(8 * (2 * nzmax + wcmax + 2));
  {
    const int64_t full = 8 * (2 * nzmax + wcmax + 2 * wcmax * wcmax + nzmax * (nzmax + wcmax) + 2);
    s.nzmax = (int32_t)nzmax;
    s.wcmax = (int32_t)wcmax;
    s.chain_lds = full <= LDS_BLOCK_MAX ? 1 : 0;
    s.lds_chain_factor = (int)(s.chain_lds ? full : s.lds_chain);
  }
  {   // cyclic reduction of the chain: levels, separators, what every node pulls from the levels below (pc_kkt_cr.hpp)
    const int64_t nc = d.n_chain;
    CrPlan& P = s.cr;
    cr_build(nc, d.n_phase, d.chain_phase_ptr, d.chain_ptr, d.nb, d.chain_export, P);
    s.chain_cr = P.ldsmax <= LDS_BLOCK_MAX && P.max_pull <= CR_MAX_PULL && knobs.cr;
    if (P.any_export && !s.chain_cr) throw std::runtime_error("exported chain nodes need the cyclic-reduction kernels (blocks too large for their LDS)");
    s.any_export = P.any_export;
    if (s.chain_cr) {
      s.cr_lvl_ptr.assign(1, 0);
      for (int l = 1; l <= P.lmax; ++l) {
        for (int64_t c = 0; c < nc; ++c)
          if (P.lvl[(size_t)c] == l) s.cr_nodes.push_back(c);
        s.cr_lvl_ptr.push_back((int64_t)s.cr_nodes.size());
      }
      s.lds_cr = (int)P.ldsmax;
      {   // the last levels in one launch (kkt_cr_top): as many trailing levels as hold at most two nodes per wave
        const size_t L = s.cr_lvl_ptr.size();
        const int wave_bytes = (int)(((int64_t)P.ldsmax + 24 * CR_MAX_PULL + 15) & ~(int64_t)15);
        int nw = (int)std::min<int64_t>(16, LDS_WORKGROUP / wave_bytes);
        if (knobs.cr_top_cap >= 0) nw = std::min(nw, knobs.cr_top_cap);
        size_t from = L;
        if (nw >= 2) {
          while (from > 1 && s.cr_lvl_ptr[from - 1] - s.cr_lvl_ptr[from - 2] <= nw && L - (from - 1) <= 17) --from;
          if (L - from < 2) from = L;             // (a single level gains nothing over its own launch)
        }
        s.cr_top_from = from;
        s.cr_top_waves = nw;
        s.cr_top_lds = nw * wave_bytes;
        s.cr_top.n = (int32_t)(L - from);
        s.cr_top.wave_bytes = wave_bytes;
        for (size_t i = 0; from + i <= L && i < 18; ++i) s.cr_top.ptr[i] = s.cr_lvl_ptr[from - 1 + i];
      }
      s.n_crbuf = std::max<int64_t>(1, P.buf_len);
      if (P.any_export)
        for (int64_t c = 0; c < nc; ++c)
          if (P.exported[(size_t)c]) s.export_nodes.push_back(c);
    }
  }
  s.lds_border = (int)(8 * (2 * (int64_t)d.nb + 2 + 256));
  // (also the NLP's own narrow border once there are thousands of terms: the one workgroup's walk took 93 us per
  //  factorisation and 40 us per back-substitution at config 3, 2 x 2 entries x 5 001 terms; config 2's 1 001 terms stay)
  if (d.nb > 0 && ((int64_t)d.nb * d.nb * (d.n_leaf + d.n_chain) > ((int64_t)1 << 18) || d.n_leaf + d.n_chain >= 2048)) {
    s.border_blocks = (int)std::min<int64_t>(256, d.n_leaf + d.n_chain);
    s.n_border_part = (int64_t)s.border_blocks * d.nb * d.nb;   // [border_blocks][nb * nb] partial sums
  }
  if (s.lds_leaf > LDS_VECTORS_MAX || s.lds_chain > LDS_VECTORS_MAX || s.lds_border > LDS_VECTORS_MAX)
    throw std::runtime_error("KKT block too large for the solver's LDS staging");
  if (s.chain_cr && d.n_chain > 0 && ((int64_t)s.cr_nodes.size() != d.n_chain || s.cr_lvl_ptr.back() != d.n_chain))
    throw std::runtime_error("internal: the level lists do not cover the chain");
  s.n_vals = d.total_vals;
  s.n_vec = d.nu;
  s.n_counts = 2 * (d.n_leaf + d.n_chain + 1);
  return s;
}

}  // namespace pck
