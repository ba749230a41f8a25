// CPU-only sanitizer harness for the callback cache (TEST INFRASTRUCTURE).
//
// Compiles pc_callback_cache.hpp with g++ -fsanitize=address,undefined and drives it the way pc_engine.hip does, against
// a simulated device.  Every buffer carries a tag -- the point it was computed at, the scaling / tile-range epoch, and
// whether it is complete: the staged x~ (pinned) and its device mirror, the device result block (small part, G~, H~) and
// the pinned result block as the host sees it.  A queued copy, or a kernel writing the pinned block, makes the host's
// view incomplete at once and complete only at a wait on an event recorded after it or at a drain: the worst case an
// asynchronous copy allows.  The caller has a current point, passes new_x = 1 when it moves and may pass new_x = 0 at
// its current point after any other call in between.
//
// Every launch asks writes_result_block with the pointers the engine would pass (offsets into two real result blocks, a
// caller's own buffers), and main checks the edges of that question before anything else.
//
//   usage: callback_cache_sanitize <length> <scripts.txt> <out.txt>
//
// (1) every sequence of calls up to <length> from each of the 8 starting settings: after every callback the data handed
//     back must be complete, of the caller's point and of the current epoch; prints "sequences N" and "callbacks N".
// (2) for every sequence of at most 2 calls in the 8 settings and for every line of <scripts.txt> ("mode prefetch tok ..."),
//     one line per call: token, the record (stage_x launch queue_small queue_G wait), the state afterwards
//     (x_staged filled small_down G_down G_queued), prefetch, mode, generation.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../pycollo_amd/csrc/pc_callback_cache.hpp"

namespace {

const char* const TOKENS[] = {"f0", "f1", "gf0", "gf1", "g0", "g1", "jac0", "jac1", "h0", "h1", "all", "dev", "ipm", "mesh",
                              "norms", "res", "scal", "range", "mode0", "mode1", "mode2", "mode3", "pf0", "pf1"};
const int N_TOKENS = 24, N_CALLBACKS = 10;   // the first ten hand data back by the new_x protocol

struct Tag {
  int point = -1, epoch = -1;
  bool complete = false;
};
enum Part { SMALL, GJ, HS, N_PARTS };

// The handle's two result blocks and a caller's own buffers, for launch_all's question (writes_result_block): real
// arrays, so that the pointer arithmetic is the engine's.  [f | grad J | c~ | G~ | H~] at these offsets.
const size_t O_F = 0, O_GN = 1, O_C = 8, O_G = 16, O_H = 40, OUT_TOTAL = 64;
double d_out[OUT_TOTAL], h_out[OUT_TOTAL], own[OUT_TOTAL + 1];

bool writes_block(const double* c, const double* G, const double* H, const double* fobj, const double* grad_nz) {
  const double* const out[5] = {c, G, H, fobj, grad_nz};
  return pcc::writes_result_block(out, d_out, h_out, OUT_TOTAL);
}

struct Sim {
  pcc::Cache c;
  Tag hx, dx;                      // staged x~: the pinned block, the device mirror
  Tag dev[N_PARTS], host[N_PARTS]; // result blocks: the device's, the pinned one as the host sees it
  struct Pending { int seq; int part; Tag tag; } q[16];
  int nq = 0, seq = 0, ev_small = -1, ev_G = -1;
  int epoch = 0, cur = 1, next = 1; // the caller's point, the last point handed out
  pcc::Todo last;

  void arrive(int part, Tag t) {   // queued for the pinned block: unreadable until waited for
    host[part].complete = false;
    if (nq == 16) { std::fprintf(stderr, "pending queue overflow\n"); std::exit(3); }
    q[nq++] = Pending{seq++, part, t};
  }
  void complete_upto(int ev) {
    int k = 0;
    for (int i = 0; i < nq; ++i) {
      if (q[i].seq <= ev) host[q[i].part] = q[i].tag;
      else q[k++] = q[i];
    }
    nq = k;
  }
  void drain() { complete_upto(seq); }
  void stage_x(int point) {
    hx = Tag{point, 0, true};
    if (!(c.mode & 1)) dx = hx;
  }
  void launch(int parts_mask) {   // the handle's own launch, at the x~ the kernels are handed
    const Tag x = (c.mode & 1) ? hx : dx;
    double* out = (c.mode & 2) ? h_out : d_out;   // host_call: the outputs its flags name, J and grad J always
    pcc::launched(c, true, writes_block((parts_mask >> SMALL & 1) ? out + O_C : nullptr, (parts_mask >> GJ & 1) ? out + O_G : nullptr,
                                        (parts_mask >> HS & 1) ? out + O_H : nullptr, out + O_F, out + O_GN));
    for (int p = 0; p < N_PARTS; ++p) {
      if (!(parts_mask >> p & 1)) continue;
      const Tag t{x.point, epoch, x.complete};
      if (c.mode & 2) arrive(p, t); else dev[p] = t;
    }
  }
  void copy_down(int part) {
    if (!(c.mode & 2)) arrive(part, dev[part]);
  }
  // somebody else's launch wrote these parts of the device result block, on any stream; `writes`: launch_all's answer
  void clobber(int parts_mask, bool writes) {
    for (int p = 0; p < N_PARTS; ++p) {
      if (!(parts_mask >> p & 1)) continue;
      dev[p] = Tag{++next, epoch, true};
      for (int i = 0; i < nq; ++i) if (q[i].part == p) q[i].tag.complete = false;
    }
    pcc::launched(c, false, writes);
  }
  void callback(int new_x, pcc::Want want) {   // pc_engine.hip: callback()
    last = pcc::callback(c, new_x, want);
    if (last.stage_x) stage_x(cur);
    if (last.launch) launch(1 << SMALL | 1 << GJ);
    if (last.queue_small) { copy_down(SMALL); ev_small = seq - 1; }   // an event covers everything queued before it
    if (last.queue_G) { copy_down(GJ); ev_G = seq - 1; }
    if (last.wait == pcc::EV_SMALL) complete_upto(ev_small);
    if (last.wait == pcc::EV_G) complete_upto(ev_G);
  }
  bool good(const Tag& t) const { return t.complete && t.point == cur && t.epoch == epoch; }

  // one call of the alphabet; false: it handed back something it must not
  bool call(int tok) {
    last = pcc::Todo{};
    switch (tok) {
      case 0: case 1: case 2: case 3: case 4: case 5:
        if (tok & 1) cur = ++next;
        callback(tok & 1, pcc::SMALL);
        return good(host[SMALL]);
      case 6: case 7:
        if (tok & 1) cur = ++next;
        callback(tok & 1, pcc::G);
        return good(host[GJ]);
      case 8: case 9:
        if (tok & 1) cur = ++next;
        last = pcc::hessian(c, tok & 1);
        if (last.stage_x) stage_x(cur);
        launch(1 << HS);
        copy_down(HS);
        drain();
        pcc::drained(c);
        return good(host[HS]);
      case 10:   // pc_eval_all at a point the caller moves to
        cur = ++next;
        hx = Tag{cur, 0, true};
        if (!(c.mode & 1)) dx = hx;
        launch(7);
        for (int p = 0; p < N_PARTS; ++p) copy_down(p);
        drain();
        pcc::filled_all(c);
        return good(host[SMALL]) && good(host[GJ]) && good(host[HS]);
      case 11:   // device-pointer launch: the caller's c~, G~, H~, J into the handle's block (device_call)
        clobber(1 << SMALL, writes_block(own + O_C, own + O_G, own + O_H, d_out + O_F, nullptr));
        return true;
      case 12:   // interior-point launches: c~, G~, H~ into the handle's block, J and grad J into the solver's own
        clobber(1 << SMALL | 1 << GJ | 1 << HS, writes_block(d_out + O_C, d_out + O_G, d_out + O_H, own, own + 1));
        return true;
      case 13:   // pc_mesh_error at another point
        pcc::input_overwritten(c);
        hx = dx = Tag{++next, 0, true};
        drain();
        return true;
      case 14: {   // pc_row_norms_jac at a point the caller moves to
        cur = ++next;
        pcc::input_overwritten(c);
        {
          pcc::ThroughMirror mirror(c);
          callback(1, pcc::NOTHING);
        }
        const bool ok = good(dev[GJ]);   // what the row reduction reads
        drain();
        pcc::row_norms_done(c);
        return ok;
      }
      case 15: {   // pc_eval_resident at another point
        pcc::input_overwritten(c);
        pcc::ThroughMirror mirror(c);
        hx = dx = Tag{++next, 0, true};
        launch(7);
        copy_down(SMALL);
        drain();
        return true;
      }
      case 16: drain(); ++epoch; pcc::input_overwritten(c); return true;   // pc_set_scaling
      case 17: drain(); ++epoch; pcc::range_changed(c); return true;       // pc_set_tile_range
      case 18: case 19: case 20: case 21: drain(); pcc::set_mode(c, tok - 18); return true;
      default: pcc::set_prefetch(c, tok == 23); return true;
    }
  }
  void print(std::FILE* f, int tok) const {
    std::fprintf(f, "%s %d %d %d %d %d | %d %d %d %d %d %d %d %llu\n", TOKENS[tok], last.stage_x, last.launch, last.queue_small,
                 last.queue_G, (int)last.wait, c.x_staged, c.filled, c.small_down, c.G_down, c.G_queued, c.prefetch, c.mode,
                 (unsigned long long)c.generation);
  }
};

Sim start(int mode, int prefetch) {
  Sim s;
  pcc::set_mode(s.c, mode);
  pcc::set_prefetch(s.c, prefetch != 0);
  return s;
}

long long n_sequences = 0, n_callbacks = 0;
std::vector<int> path;

void explore(const Sim& s, int depth) {
  for (int tok = 0; tok < N_TOKENS; ++tok) {
    Sim t = s;
    path.push_back(tok);
    ++n_sequences;
    if (tok < N_CALLBACKS) ++n_callbacks;
    if (!t.call(tok)) {
      std::fprintf(stderr, "stale or incomplete data handed back after:");
      for (int p : path) std::fprintf(stderr, " %s", TOKENS[p]);
      std::fprintf(stderr, " (mode %d prefetch %d)\n", t.c.mode, t.c.prefetch);
      std::exit(2);
    }
    if (depth > 1) explore(t, depth - 1);
    path.pop_back();
  }
}

int token(const std::string& w) {
  for (int i = 0; i < N_TOKENS; ++i) if (w == TOKENS[i]) return i;
  std::fprintf(stderr, "unknown token %s\n", w.c_str());
  std::exit(3);
}

void print_sequence(std::FILE* f, int mode, int prefetch, const std::vector<int>& toks) {
  Sim s = start(mode, prefetch);
  std::fprintf(f, "start %d %d\n", mode, prefetch);
  for (int tok : toks) {
    if (!s.call(tok)) { std::fprintf(stderr, "a printed sequence handed back stale data\n"); std::exit(2); }
    s.print(f, tok);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: callback_cache_sanitize <length> <scripts.txt> <out.txt>\n"); return 3; }
  const int length = std::atoi(argv[1]);
  std::FILE* f = std::fopen(argv[3], "w");
  if (!f || length < 1) return 3;
  // launch_all's question, edge by edge: inside either block, its first and last entry; one past its end, in front of it,
  // null outputs, a handle without blocks; a call with buffers of its own (the derivative check) leaves the cache alone
  const bool edges = writes_block(d_out, nullptr, nullptr, nullptr, nullptr) && writes_block(nullptr, nullptr, nullptr, nullptr, d_out + OUT_TOTAL - 1) &&
                     writes_block(nullptr, h_out + O_G, nullptr, nullptr, nullptr) && writes_block(own, own, own, h_out + O_F, own) &&
                     !writes_block(nullptr, nullptr, nullptr, nullptr, nullptr) && !writes_block(own, own + O_G, own + O_H, own + OUT_TOTAL, own + 1);
  const double* const past[5] = {d_out + OUT_TOTAL, nullptr, nullptr, nullptr, nullptr};   // (against d_out alone: h_out may follow it)
  const double* const in_front[5] = {d_out + 8, nullptr, nullptr, nullptr, nullptr};
  pcc::Cache before = start(0, 1).c, after = before;
  pcc::launched(after, false, writes_block(own, own + O_G, own + O_H, own + OUT_TOTAL, own + 1));
  if (!edges || pcc::writes_result_block(past, d_out, nullptr, OUT_TOTAL) || pcc::writes_result_block(past, nullptr, d_out, OUT_TOTAL) || pcc::writes_result_block(in_front, d_out + 9, h_out, OUT_TOTAL - 9) ||
      pcc::writes_result_block(in_front, nullptr, nullptr, OUT_TOTAL) || after.generation != before.generation) {
    std::fprintf(stderr, "writes_result_block: an edge is wrong\n");
    return 2;
  }
  for (int mode = 0; mode < 4; ++mode)
    for (int prefetch = 0; prefetch < 2; ++prefetch) explore(start(mode, prefetch), length);
  std::fprintf(f, "sequences %lld\ncallbacks %lld\n", n_sequences, n_callbacks);
  for (int mode = 0; mode < 4; ++mode)
    for (int prefetch = 0; prefetch < 2; ++prefetch)
      for (int a = 0; a < N_TOKENS; ++a) {
        print_sequence(f, mode, prefetch, {a});
        for (int b = 0; b < N_TOKENS; ++b) print_sequence(f, mode, prefetch, {a, b});
      }
  std::ifstream scripts(argv[2]);
  for (std::string line; std::getline(scripts, line);) {
    std::istringstream in(line);
    int mode, prefetch;
    if (!(in >> mode >> prefetch)) continue;
    std::vector<int> toks;
    for (std::string w; in >> w;) toks.push_back(token(w));
    print_sequence(f, mode, prefetch, toks);
  }
  std::fprintf(f, "ok\n");
  std::fclose(f);
  return 0;
}
