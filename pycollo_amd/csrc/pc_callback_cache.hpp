// The cache behind IPOPT's new_x flag (pure C++: no HIP, no handle, no environment; compiled into pc_engine.hip, and on
// its own under AddressSanitizer / UBSan by tests/c/callback_cache_sanitize.cpp, which runs it against a simulated device).
// The engine names events and does what the returned record says; every write to the cache's state is in this file.
//
// State     x_staged   the staged x~ is the caller's point
//           filled     J, grad J, c~ and G~ at that point have been launched (new_x = 0 reuses them)
//           small_down, G_down   the host copy of [J | grad J | c~] / of G~ is complete
//           G_queued   a copy-down of G~ has been queued for this fill
// Settings  prefetch   copy G~ down with every fill (IPOPT asks for it next); off: only when pc_eval_jac_g asks
//           mode       bit 0: the kernels read the pinned input block, bit 1: they write the pinned result block
// generation moves whenever x~ is staged, the cache is filled or any of it is invalidated: a caller that remembers the
// point and the generation of its last new_x = 1 call may pass new_x = 0 while both are unchanged (pc_cache_generation).
//
// Events    callback   pc_eval_f / grad_f / g (want SMALL), pc_eval_jac_g (want G), pc_row_norms_jac (want NOTHING):
//                      stage x~ when new_x or nothing is staged (then filled = 0); when not filled launch c~ | G~, queue
//                      the small copy and ev_small, queue G~'s copy and ev_G when prefetch or mode bit 1 (G_queued),
//                      filled = 1, nothing down.  SMALL not down: wait on ev_small.  G not down: queue its copy and
//                      ev_G now unless queued, wait on ev_G, which completes the small copy as well.
//           hessian    pc_eval_h: stage x~ by the same rule; the engine stages lambda, launches H~, copies it down, drains.
//           drained    the stream is empty: the small copy is complete if there is a fill, G~'s if it was queued.
//           filled_all pc_eval_all staged [x~ | lambda], launched everything, copied everything down and drained.
//           launched   every launch (launch_all): one that is not the cache's own and writes into the handle's result
//                      block (writes_result_block) is "result block overwritten": filled = small_down = G_down = 0.
//           input_overwritten   pc_mesh_error, pc_eval_resident, pc_set_scaling, set_mode: x_staged = filled = 0.
//           range_changed       pc_set_tile_range: filled = 0.
//           ThroughMirror, row_norms_done   see below.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pcc {

struct Cache {
  bool x_staged = false, filled = false, small_down = false, G_down = false, G_queued = false;
  bool prefetch = true;
  int mode = 0;
  uint64_t generation = 0;
};

enum Want { NOTHING, SMALL, G };
enum Wait { NO_WAIT, EV_SMALL, EV_G };

// what a callback does before it reads the pinned result block, in this order
struct Todo {
  bool stage_x = false;      // x~ into the pinned block unless it is there; copied up unless mode bit 0
  bool launch = false;       // c~ | G~ (callback); the Hessian's launch is the engine's own
  bool queue_small = false;  // copy [J | grad J | c~] down unless mode bit 1, record ev_small
  bool queue_G = false;      // copy G~ down unless mode bit 1, record ev_G
  Wait wait = NO_WAIT;       // ... then check the tail's timeout word
};

inline void stage(Cache& c, int new_x, Todo& t) {
  if (!new_x && c.x_staged) return;
  t.stage_x = true;
  c.x_staged = true;
  c.filled = false;
  ++c.generation;
}

inline Todo callback(Cache& c, int new_x, Want want) {
  Todo t;
  stage(c, new_x, t);
  if (!c.filled) {
    t.launch = t.queue_small = true;
    t.queue_G = c.G_queued = c.prefetch || (c.mode & 2);
    c.filled = true;
    c.small_down = c.G_down = false;
    ++c.generation;
  }
  if (want == SMALL && !c.small_down) {
    t.wait = EV_SMALL;
    c.small_down = true;
  }
  if (want == G && !c.G_down) {
    if (!c.G_queued) t.queue_G = c.G_queued = true;   // G~ stayed on the device until somebody asked for it
    t.wait = EV_G;
    c.small_down = c.G_down = true;
  }
  return t;
}

inline Todo hessian(Cache& c, int new_x) {
  Todo t;
  stage(c, new_x, t);
  return t;
}

inline void drained(Cache& c) {
  c.small_down = c.filled;
  c.G_down = c.filled && c.G_queued;
}

inline void filled_all(Cache& c) {
  c.x_staged = c.filled = c.small_down = c.G_down = c.G_queued = true;   // (G~ came down with the rest)
  ++c.generation;
}

inline void input_overwritten(Cache& c) {
  c.x_staged = c.filled = false;
  ++c.generation;
}

inline void range_changed(Cache& c) {
  c.filled = false;
  ++c.generation;
}

inline void set_prefetch(Cache& c, bool on) { c.prefetch = on; }

// pc_set_host_mode, after its drain: the staged x~ may be in the other block
inline void set_mode(Cache& c, int mode) {
  c.mode = mode;
  input_overwritten(c);
}

// [p, p + n) of either of the handle's result blocks holds q
inline bool in_block(const double* q, const double* p, size_t n) {
  return p && reinterpret_cast<uintptr_t>(q) >= reinterpret_cast<uintptr_t>(p) &&
         reinterpret_cast<uintptr_t>(q) < reinterpret_cast<uintptr_t>(p + n);
}
// a call's outputs c, G, H, fobj, grad_nz: does one of them point into the device or the pinned result block?
inline bool writes_result_block(const double* const out[5], const double* d_out, const double* h_out, size_t out_total) {
  for (int i = 0; i < 5; ++i)
    if (out[i] && (in_block(out[i], d_out, out_total) || in_block(out[i], h_out, out_total))) return true;
  return false;
}
// launch_all's report: `own` is a fill or a Hessian of the host-pointer calls themselves
inline void launched(Cache& c, bool own, bool writes_block) {
  if (own || !writes_block) return;
  c.filled = c.small_down = c.G_down = false;   // x_staged stays: the staged input was not touched
  ++c.generation;
}

// Evaluate through the device mirror (pc_eval_resident, pc_row_norms_jac: what follows reads the device's results):
// mode 0 now, the caller's mode on every exit.
struct ThroughMirror {
  Cache& c;
  const int mode;
  explicit ThroughMirror(Cache& c_) : c(c_), mode(c_.mode) { c.mode = 0; }
  ~ThroughMirror() { c.mode = mode; }
  ThroughMirror(const ThroughMirror&) = delete;
  ThroughMirror& operator=(const ThroughMirror&) = delete;
};

// pc_row_norms_jac after its drain (before: input_overwritten and callback(1, NOTHING) inside a ThroughMirror): the fill
// describes the device mirror, which is what the cache means in mode 0 only
inline void row_norms_done(Cache& c) {
  c.x_staged = c.filled = (c.mode == 0);
  drained(c);
  ++c.generation;
}

}  // namespace pcc
