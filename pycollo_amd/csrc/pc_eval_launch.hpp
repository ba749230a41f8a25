// What the evaluation's kernels are handed and how they are launched (pure C++, no device code, no environment, no
// handle: compiled into pc_engine.hip, and on its own under AddressSanitizer / UBSan by tests/c/eval_launch_sanitize.cpp).
// pc_eval_shape.hpp decides which kernels run with how many waves and how much LDS; this header packs their argument
// blocks and plans the launches of one call:
//   build_blocks   the argument blocks, rebuilt when the scaling, a tile range or a partials buffer changes
//   plan           the launches of one call -- at most one per phase and the tail -- and pc_info.last_launch
//   kernel_name    the symbol of every kernel a plan can name
// Device addresses are plain pointers that are never dereferenced here.  The layouts and the packed words of the launch
// ABI are in pc_args.h; the fields of last_launch in include/pycollo_amd.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pycollo_amd.h"
#include "pc_args.h"
#include "pc_eval_shape.hpp"

namespace pcl {

static_assert(pce::TAIL_PARTS == PC_MAX_TAIL_BLOCKS, "PcLead::wa and last_launch hold at most PC_MAX_TAIL_BLOCKS tail blocks");
static_assert(PC_MAX_TAIL_BLOCKS <= PC_LAUNCH_TAIL_BLOCKS_MASK && PC_MAX_BLOCK_THREADS / 64 <= PC_LAUNCH_TAIL_WAVES_MASK &&
                  PC_TAIL_THREADS <= PC_MAX_BLOCK_THREADS,
              "the fields of last_launch hold their largest values");

// ---- the kernels of a code object --------------------------------------------------------------------------------
enum Kernel {
  BULK,            // <bulk>: one phase's tiles
  BULK_RES,        // <bulk>_r: a single-phase problem's tiles with the tail as the leading workgroups
  BULK_RES_W,      // <bulk>_r_w<W>: the same with the replica index compiled in, for exactly W waves per tile
  BULK_ALL,        // pc_bulk_all: every phase's tiles in one launch
  BULK_ALL_RES,    // pc_bulk_all_r
  BULK_ALL_RES_W,  // pc_bulk_all_r_w<W>
  TAIL,            // <tail>
  TAIL_BIG,        // <tail>_big: several strides of partial sums in flight per lane
  N_KERNELS
};

// The symbol of kernel k: `phase` picks the phase's bulk kernel (pc_phase_desc::bulk_kernel), `wpt` the waves per tile of
// the _w<W> builds; tail_kernel is pc_problem_desc::tail_kernel.
inline std::string kernel_name(const pcp::Problem& Q, const char* tail_kernel, Kernel k, int phase, int wpt) {
  switch (k) {
    case BULK: return Q.ph[phase].bulk_kernel;
    case BULK_RES: return Q.ph[phase].bulk_kernel + "_r";
    case BULK_RES_W: return Q.ph[phase].bulk_kernel + "_r_w" + std::to_string(wpt);
    case BULK_ALL: return "pc_bulk_all";
    case BULK_ALL_RES: return "pc_bulk_all_r";
    case BULK_ALL_RES_W: return "pc_bulk_all_r_w" + std::to_string(wpt);
    case TAIL: return tail_kernel;
    case TAIL_BIG: return std::string(tail_kernel) + "_big";
    default: throw std::logic_error("kernel_name: no such kernel");
  }
}

// Which of the optional kernels the handle may launch: BULK (every phase) and TAIL are required.  pc_create looks
// BULK_RES up for a single phase only, BULK_ALL for several phases and with the merge knob on, BULK_ALL_RES when BULK_ALL
// is there, a _W build when its plain build is there and the launch has more than one wave per tile.
struct Have {
  bool k[N_KERNELS] = {};
};

// the handle may run the tail beside the tiles: the knob allows it and the code object has the kernel
inline bool has_resident_kernel(const pce::Shape& S, const Have& hv, size_t n_phases) {
  return S.resident && hv.k[n_phases > 1 ? BULK_ALL_RES : BULK_RES];
}
// pc_info.n_launches: one launch per phase and the tail; two with the merged launch; one with the resident tail
inline int launches_per_evaluation(const pce::Shape& S, const Have& hv, size_t n_phases) {
  if (has_resident_kernel(S, hv, n_phases)) return 1;
  return n_phases > 1 && hv.k[BULK_ALL] ? 2 : (int)n_phases + 1;
}

// ---- what the blocks are built from ------------------------------------------------------------------------------
// the launched tiles of a phase (the whole phase unless sharded) and a caller's buffer for its partial sums, or null
struct Range {
  int tile_begin = 0, tile_end = 0;
  double* partials_ext = nullptr;
};

// the scaling the handle holds: per phase the packed doubles of PcPhaseArgs::scal, the endpoint block's tables, w_J
struct Scaling {
  std::vector<std::vector<double>> phase;
  std::vector<double> pointV, pointr, Wend;
  double wJ = 1.0;
};

struct PhaseAddr {
  const int32_t *tile_k0 = nullptr, *tile_n0 = nullptr, *sec_s = nullptr;
  const double* sec_h = nullptr;
  const int64_t *sec_E = nullptr, *hslot0 = nullptr, *hslotN = nullptr, *hsum_slot = nullptr;
  const int32_t* hsum_local = nullptr;
  const double *scal = nullptr, *tab = nullptr;
  double* partials = nullptr;
  unsigned long long* gran = nullptr;
};
struct Addr {
  const double* qa = nullptr;   // the packed A tables, the weight tables right behind them
  const int64_t* point_x = nullptr;
  const double *point_V = nullptr, *point_r = nullptr, *W_end = nullptr;
  const int64_t *tail_owned = nullptr, *pt_hslot = nullptr;
  const int32_t* pt_hlocal = nullptr;
  unsigned long long *erec = nullptr, *hb_gran = nullptr;
  const int64_t* rec_slot = nullptr;
  const int32_t* rec_term = nullptr;
  unsigned* timeout = nullptr;
  const PcPhaseArgs* phase_args = nullptr;   // [n_phases] device copy of Blocks::merged (handles with BULK_ALL)
  const PcTileRec* trec = nullptr;           // device copy of Records::recs (mixed build)
  PhaseAddr ph[PC_MAX_PHASES];
};

// Mixed build: the records a launch reads, one per workgroup -- those of the launched ranges, phase after phase, which
// is the order the merged launch numbers its workgroups in; a phase's own launch starts at first[phase].  Never empty.
struct Records {
  std::vector<PcTileRec> recs;
  int first[PC_MAX_PHASES] = {};
};
inline Records launched_records(const pce::Shape& S, const Range* rg, size_t n_phases) {
  Records R;
  for (size_t ip = 0; ip < n_phases; ++ip) {
    R.first[ip] = (int)R.recs.size();
    for (int t = rg[ip].tile_begin; t < rg[ip].tile_end; ++t) R.recs.push_back(S.trec_all[S.trec_base[ip] + t]);
  }
  if (R.recs.empty()) R.recs.push_back(PcTileRec{});
  return R;
}

// What the kernels that read a finished NLP point (pc_solution.hpp) know about a phase: the point d_x, the phase's place
// in it, its mesh and the variable scaling the handle holds now.
inline PcPhaseView phase_view(const pcp::Problem& Q, const Scaling& sc, const Addr& A, int phase, const double* d_x) {
  const auto& P = Q.ph[phase];
  const auto& s = sc.phase[phase];
  if (s.size() > PC_MAX_SCAL) throw std::runtime_error("too many scaling constants for the kernel argument block");
  PcPhaseView v;
  std::memset(&v, 0, sizeof(v));
  v.x = d_x;
  v.sec_s = A.ph[phase].sec_s;
  v.x_off = P.x_off;
  v.s_off = Q.s_off;
  v.t_fixed[0] = P.t_fixed[0];
  v.t_fixed[1] = P.t_fixed[1];
  v.N = P.N;
  v.K = P.K;
  for (size_t i = 0; i < s.size(); ++i) v.scal[i] = s[i];
  return v;
}

// The argument block of one phase's tiles in a launch of `wpt` waves per tile: everything but the caller's pointers,
// the flags and the epoch.  Four waves stage one pass per state (PhaseShape::lds_out4).
inline PcPhaseArgs phase_args(const pcp::Problem& Q, const pce::Shape& S, const Scaling& sc, const Range* rg, const Addr& A,
                              const Records& rec, size_t ip, int wpt) {
  const auto& P = Q.ph[ip];
  const auto& D = S.ph[ip];
  const auto& pa = A.ph[ip];
  const auto& s = sc.phase[ip];
  PcPhaseArgs a;
  std::memset(&a, 0, sizeof(a));
  a.tile_k0 = pa.tile_k0;
  a.tile_n0 = pa.tile_n0;
  a.sec_s = pa.sec_s;
  a.sec_h = pa.sec_h;
  a.sec_E = pa.sec_E;
  a.qa = A.qa;
  a.qw = A.qa + S.qa_n;
  if (s.size() > PC_MAX_SCAL) throw std::runtime_error("too many scaling constants for the kernel argument block");
  for (size_t i = 0; i < s.size(); ++i) a.scal[i] = s[i];
  for (size_t i = 0; i < P.goff.size(); ++i) a.goff[i] = P.goff[i];
  for (size_t i = 0; i < P.hoff.size(); ++i) a.hoff[i] = P.hoff[i];
  a.uni_n = D.uni_n;
  a.spt = D.spt;
  a.lds_out = wpt == 4 ? D.lds_out4 : D.lds_out;
  a.wpt = wpt;
  a.hslot0 = pa.hslot0;
  a.hslotN = pa.hslotN;
  a.partials = rg[ip].partials_ext ? rg[ip].partials_ext : pa.partials;
  a.gran = pa.gran;
  a.erec = A.erec;
  a.erec0 = D.erec0;
  a.tab = pa.tab;
  a.tile_rec = (S.mixed && A.trec) ? A.trec + rec.first[ip] : nullptr;
  a.x_off = P.x_off;
  a.s_off = Q.s_off;
  a.c_off = P.c_off;
  a.c_path_off = P.c_path_off;
  a.c_int_off = P.c_int_off;
  a.t_fixed[0] = P.t_fixed[0];
  a.t_fixed[1] = P.t_fixed[1];
  a.N = P.N;
  a.K = P.K;
  a.n_tiles = D.n_tiles;
  a.tile_begin = rg[ip].tile_begin;
  a.n_blocks = std::max(0, rg[ip].tile_end - rg[ip].tile_begin);
  a.block_threads = S.TB * wpt;
  a.qa_total = S.qa_n;
  a.qw_total = S.qw_n;
  std::memcpy(a.qa_off, S.qa_off, sizeof(a.qa_off));
  std::memcpy(a.qw_off, S.qw_off, sizeof(a.qw_off));
  return a;
}

// the tail's argument block: everything but the caller's pointers, the flags, sigma, the epoch and who runs it
inline PcTailArgs tail_args(const pcp::Problem& Q, const pce::Shape& S, const Scaling& sc, const Range* rg, const Addr& A) {
  PcTailArgs t;
  std::memset(&t, 0, sizeof(t));
  t.sigma = 1.0;
  t.wJ = sc.wJ;
  t.point_x = A.point_x;
  t.point_V = A.point_V;
  t.point_r = A.point_r;
  t.W_end = A.W_end;
  for (size_t i = 0; i < Q.point_x.size(); ++i) {
    t.pt_x[i] = Q.point_x[i];
    t.pt_V[i] = sc.pointV[i];
    t.pt_r[i] = sc.pointr[i];
  }
  for (size_t r = 0; r < sc.Wend.size(); ++r) t.pt_W[r] = sc.Wend[r];
  t.tail_owned = A.tail_owned;
  t.pt_hslot = A.pt_hslot;
  t.pt_hlocal = A.pt_hlocal;
  t.c_end_off = Q.c_end_off;
  t.g_end_base = Q.g_end_base;
  t.n_tail_owned = (int32_t)Q.tail_owned.size();
  t.block_threads = PC_TAIL_THREADS;
  t.lds_nred = S.lds_nred;
  t.erec = A.erec;
  t.rec_slot = A.rec_slot;
  t.rec_term = A.rec_term;
  t.n_rec = S.n_rec;
  t.n_tail_blocks = 1;
  t.hb_gran = A.hb_gran;
  t.timeout = A.timeout;
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    const auto& P = Q.ph[ip];
    PcTailPhase& tp = t.ph[ip];
    tp.partials = rg[ip].partials_ext ? rg[ip].partials_ext : A.ph[ip].partials;
    tp.gran = A.ph[ip].gran;
    tp.scal = A.ph[ip].scal;
    tp.x_off = P.x_off;
    tp.s_off = Q.s_off;
    tp.c_int_off = P.c_int_off;
    for (int m = 0; m < 8; ++m) tp.gq_base[m] = P.gq_base[m];
    tp.hsum_slot = A.ph[ip].hsum_slot;
    tp.hsum_local = A.ph[ip].hsum_local;
    tp.t_fixed[0] = P.t_fixed[0];
    tp.t_fixed[1] = P.t_fixed[1];
    tp.n_tiles = S.ph[ip].n_tiles;
    tp.N = P.N;
  }
  return t;
}

// (lead scalars..., PcPhaseArgs): the lead is what the command processor preloads into SGPRs (pc_args.h), copies of the
// block's fields of the same name; `tail_blocks` leading workgroups of a resident launch run the tail
inline PcLead lead_of(const PcPhaseArgs& a, int tail_blocks) {
  const int un = a.uni_n > 0 ? a.uni_n : 0;
  return PcLead{a.x + a.x_off, a.lam ? a.lam + a.c_off : nullptr, a.qa, a.sec_h, a.N, a.K, a.tile_begin, a.n_blocks,
                pc_lead_wa(a.flags, a.wpt, a.block_threads, a.spt, tail_blocks),
                un ? pc_lead_wb(a.qa_off[un], a.qa_total + a.qw_off[un]) : 0};
}
// the values lead_of packs fit their fields (flags are the caller's and bounded by PC_FLAG_*: pc_args.h)
inline void check_lead(const PcPhaseArgs& a, int tail_blocks) {
  const int un = a.uni_n > 0 ? a.uni_n : 0;
  if (un > PC_MAX_ORDER || !pc_lead_wa_fits(a.wpt, a.block_threads, a.spt, tail_blocks) ||
      (un && !pc_lead_wb_fits(a.qa_off[un], a.qa_total + a.qw_off[un])))
    throw std::runtime_error("a launch argument does not fit its field of the kernels' lead words (waves per tile " +
                             std::to_string(a.wpt) + ", block threads " + std::to_string(a.block_threads) + ", sections per tile " +
                             std::to_string(a.spt) + ", tail blocks " + std::to_string(tail_blocks) + ", order " + std::to_string(un) + ")");
}

// The _w<W> kernels are compiled for a block of exactly W waves (pc_kernels.hpp: thread count, wave index and tile
// width are constants of each replica's body), so one is planned only with that block.
inline void check_replica_block(int wpt, int block_threads) {
  if (wpt < 1 || block_threads != 64 * wpt)
    throw std::runtime_error("a per-replica kernel (_w<W>) takes a block of exactly 64 W threads (waves per tile " +
                             std::to_string(wpt) + ", block threads " + std::to_string(block_threads) + ")");
}

// ---- the argument blocks -----------------------------------------------------------------------------------------
// Kept filled between calls; a call patches the caller's pointers, the flags, sigma and the epoch into the blocks of
// the launches it plans and hands them over as they lie (nothing is copied, nothing allocated).
struct Blocks {
  size_t n_phases = 0;
  Range rg[PC_MAX_PHASES];           // the ranges the blocks describe
  std::vector<PcBulkArgs> bulk;      // [n_phases] BULK: the phase with its own waves per tile
  std::vector<PcPhaseArgs> merged;   // [n_phases] BULK_ALL*: the phases with the merged launch's waves per tile; the engine
                                     //   keeps a copy on the device (Addr::phase_args)
  PcBulkTailArgs res;                // BULK_RES*: the single phase and the tail
  PcMultiTailArgs multi;             // BULK_ALL*: the call's part, and the tail behind it for BULK_ALL_RES*
  PcTailLaunch tail;                 // TAIL*
  uint32_t epoch = 0;                // tag of the last resident launch's granules: survives a rebuild, never 0 again
};

inline void build_blocks(Blocks& B, const pcp::Problem& Q, const pce::Shape& S, const Scaling& sc, const Range* rg,
                         const Addr& A, const Records& rec) {
  const size_t n = Q.ph.size();
  B.n_phases = n;
  std::copy(rg, rg + n, B.rg);
  B.bulk.resize(n);
  B.merged.resize(n);
  for (size_t ip = 0; ip < n; ++ip) {
    B.bulk[ip].a = phase_args(Q, S, sc, rg, A, rec, ip, S.ph[ip].wpt);
    B.merged[ip] = phase_args(Q, S, sc, rg, A, rec, ip, S.wpt_all);
    check_lead(B.bulk[ip].a, S.tail_blocks);   // (the lead itself holds the caller's pointers: patch)
    check_lead(B.merged[ip], S.tail_blocks_all);   // (no lead words, but last_launch holds the same fields)
  }
  B.tail.t = tail_args(Q, S, sc, rg, A);
  B.res.b = B.bulk[0];
  B.res.t = B.tail.t;
  B.res.t.n_tail_blocks = S.tail_blocks;
  // the merged launch: workgroup b belongs to the phase p with first_block[p] <= b < first_block[p + 1]; a phase with
  // an empty range takes no workgroups, the entries behind the last phase repeat the total
  PcMultiArgs& m = B.multi.m;
  std::memset(&m, 0, sizeof(m));
  m.ph = A.phase_args;
  m.n_phases = (int32_t)n;
  m.trec = S.mixed ? A.trec : nullptr;
  int nb = 0;
  for (size_t ip = 0; ip <= PC_MAX_PHASES; ++ip) {
    m.first_block[ip] = nb;
    if (ip < n) nb += std::max(0, rg[ip].tile_end - rg[ip].tile_begin);
  }
  m.tail_blocks = S.tail_blocks_all;
  B.multi.t = B.tail.t;
  B.multi.t.n_tail_blocks = S.tail_blocks_all;
}

// ---- one call ----------------------------------------------------------------------------------------------------
struct Call {
  const double* x = nullptr;     // [num_x] the point
  const double* lam = nullptr;   // [num_c] multipliers, or null without PC_FLAG_H
  double *c = nullptr, *G = nullptr, *H = nullptr;
  double* fobj = nullptr;        // [1] objective value
  double* grad_nz = nullptr;     // non-zeros of grad J, or null
  int flags = 0;                 // PC_FLAG_*
  double sigma = 1.0;            // objective factor
  bool bulk = true, tail = true; // the tiles' part and the tail's part of the evaluation (a sharded rank runs them apart)
};

struct Launch {
  Kernel kernel;
  int phase;                 // BULK*: the phase; else 0
  unsigned grid, block, lds;
  void* args;                // the kernel's parameters as one block (HIP_LAUNCH_PARAM_BUFFER_POINTER)
  size_t arg_bytes;
};
struct Plan {
  int n = 0;
  Launch l[PC_MAX_PHASES + 1];
  int last_launch = 0;       // pc_info.last_launch (PC_LAUNCH_*)
  void add(Kernel k, int phase, int grid, int block, int lds, void* args, size_t bytes) {
    l[n++] = Launch{k, phase, (unsigned)grid, (unsigned)block, (unsigned)lds, args, bytes};
  }
};

// One launch per evaluation when every phase runs whole on this device: the tail is the leading workgroups of the bulk
// launch and receives the tiles' partial sums as granules (pc_kernels.hpp, RES).  A rank of the section-sharded
// evaluation, whose sums travel through the all-gather first, and the bulk-only / tail-only calls take two launches.
inline bool resident_call(const Blocks& B, const pce::Shape& S, const Have& hv, const Call& c) {
  bool res = c.bulk && c.tail && has_resident_kernel(S, hv, B.n_phases);
  for (size_t ip = 0; res && ip < B.n_phases; ++ip)
    res = B.rg[ip].tile_begin == 0 && B.rg[ip].tile_end == S.ph[ip].n_tiles && !B.rg[ip].partials_ext;
  return res;
}

inline void patch(PcTailArgs& t, const Call& c, int block_threads, uint32_t epoch) {
  t.x = c.x; t.lam = c.lam; t.c = c.c; t.G = c.G; t.H = c.H;
  t.fobj = c.fobj; t.grad_nz = c.grad_nz; t.flags = c.flags; t.sigma = c.sigma;
  t.block_threads = block_threads;   // threads of the workgroup that runs the tail
  t.epoch = epoch;
}
inline void patch(PcBulkArgs& b, const Call& c, uint32_t epoch, int tail_blocks) {
  PcPhaseArgs& a = b.a;
  a.x = c.x; a.lam = c.lam; a.c = c.c; a.G = c.G; a.H = c.H;
  a.flags = c.flags;
  a.epoch = epoch;
  b.lead = lead_of(a, tail_blocks);
}

// The launches of call c, in order.  The blocks of the planned launches are patched in place and B.epoch advances on a
// resident launch (zero is the tag of never-written granules).
inline Plan plan(Blocks& B, const pce::Shape& S, const Have& hv, const Call& c) {
  Plan p;
  const bool res = resident_call(B, S, hv, c);
  if (res && ++B.epoch == 0) B.epoch = 1;
  const bool merged = c.bulk && B.n_phases > 1 && hv.k[BULK_ALL];   // several phases, one launch: their workgroups side by side
  if (merged) {
    PcMultiArgs& m = B.multi.m;
    m.x = c.x; m.lam = c.lam; m.c = c.c; m.G = c.G; m.H = c.H;
    m.flags = c.flags;
    m.epoch = B.epoch;
    const int nb = m.first_block[PC_MAX_PHASES], bt = S.TB * S.wpt_all;
    p.last_launch |= PC_LAUNCH_MERGED;
    if (res) {
      patch(B.multi.t, c, bt, B.epoch);
      if (hv.k[BULK_ALL_RES_W]) check_replica_block(S.wpt_all, bt);
      p.add(hv.k[BULK_ALL_RES_W] ? BULK_ALL_RES_W : BULK_ALL_RES, 0, nb + m.tail_blocks, bt, std::max(S.lds_all, S.tail_lds_bytes),
            &B.multi, sizeof(B.multi));
      p.last_launch |= PC_LAUNCH_RESIDENT | (m.tail_blocks << PC_LAUNCH_TAIL_BLOCKS_SHIFT) | ((bt / 64) << PC_LAUNCH_TAIL_WAVES_SHIFT);
      return p;
    }
    if (nb > 0) p.add(BULK_ALL, 0, nb, bt, S.lds_all, &m, sizeof(m));
  } else if (res) {   // a single phase
    const int bt = S.TB * S.ph[0].wpt, ntb = S.tail_blocks;
    patch(B.res.b, c, B.epoch, ntb);
    patch(B.res.t, c, bt, B.epoch);
    if (hv.k[BULK_RES_W]) check_replica_block(B.res.b.a.wpt, bt);
    p.add(hv.k[BULK_RES_W] ? BULK_RES_W : BULK_RES, 0, S.ph[0].n_tiles + ntb, bt, std::max(S.ph[0].lds_bytes, S.tail_lds_bytes), &B.res,
          sizeof(B.res));
    p.last_launch = PC_LAUNCH_RESIDENT | (ntb << PC_LAUNCH_TAIL_BLOCKS_SHIFT) | ((bt / 64) << PC_LAUNCH_TAIL_WAVES_SHIFT);
    return p;
  } else if (c.bulk) {   // one launch per phase with tiles in its range
    for (size_t ip = 0; ip < B.n_phases; ++ip) {
      if (B.rg[ip].tile_end <= B.rg[ip].tile_begin) continue;
      patch(B.bulk[ip], c, B.epoch, 0);
      p.add(BULK, (int)ip, B.rg[ip].tile_end - B.rg[ip].tile_begin, S.TB * S.ph[ip].wpt, S.ph[ip].lds_bytes, &B.bulk[ip], sizeof(PcBulkArgs));
    }
  }
  if (!c.tail) return p;
  PcTailArgs& t = B.tail.t;
  patch(t, c, PC_TAIL_THREADS, B.epoch);
  B.tail.lead = PcTailLead{t.x, t.ph[0].partials, t.ph[0].scal, t.ph[0].x_off, t.ph[0].n_tiles, t.ph[0].N, t.flags, t.block_threads};
  const bool big = hv.k[TAIL_BIG] && S.tail_big;
  p.add(big ? TAIL_BIG : TAIL, 0, 1, PC_TAIL_THREADS, S.tail_lds_bytes, &B.tail, sizeof(B.tail));
  p.last_launch |= (big ? PC_LAUNCH_TAIL_BIG : 0) | ((PC_TAIL_THREADS / 64) << PC_LAUNCH_TAIL_WAVES_SHIFT);
  return p;
}

}  // namespace pcl
