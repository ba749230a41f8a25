// The KKT solver's launch shape (pycollo_amd/csrc/pc_kkt_shape.hpp) under AddressSanitizer + UBSan.
// usage: kkt_shape_sanitize cases.txt
// The file holds synthetic descriptors, one block each ("3x5" stands for 3 3 3 3 3):
//   case NAME
//   nb N
//   chain NZ ...          unknowns per chain node
//   seg P0 P1 ...         chain_phase_ptr
//   leaf M ...            unknowns per leaf
//   left C ...            leaf_left (default: the k-th chain node that is not the last of its segment)
//   rows LEN ...          entries per row of the product (nu = number of rows; entry e: index e % 1000, kind e % 3)
//   entry E IDX KIND      overwrite one entry of the product's tables
//   export F ...          chain_export
//   knobs LEAF_FWD LEAF_WAVES CR CR_TOP_CAP
//   end
// For every block the shape is built, every offset table is walked against the buffer it indexes with checked accesses, and
// the shape is printed, one "name values..." line per item ("error TEXT" for a refused descriptor), for the test to compare
// with its own restatement of the rules.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "../../pycollo_amd/csrc/pc_kkt_shape.hpp"

using I64 = std::vector<int64_t>;

template <class V>
static void line(const char* name, const V& v) {
  std::printf("%s", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}
static void num(const char* name, long long v) { std::printf("%s %lld\n", name, v); }

static void need(bool ok, const char* what) {
  if (!ok) throw std::out_of_range(what);
}

// every offset a kernel would form from the shape's tables, against the length of the buffer it indexes
static void walk(const pc_kkt_desc& d, const pck::Shape& s) {
  const int64_t nc = d.n_chain;
  auto nz = [&](int64_t c) { return d.chain_ptr[c + 1] - d.chain_ptr[c]; };
  for (int64_t l = 0; l < d.n_leaf; ++l) {
    const int64_t left = d.leaf_left[l], w = nz(left) + nz(left + 1) + d.nb;
    need(s.leafG_off.at((size_t)l) >= 0 && s.leafG_off.at((size_t)l) + w <= s.n_leafG, "leafG_off");
    need(s.leaf_of_left.at((size_t)left) == l, "leaf_of_left");
  }
  for (int64_t c = 0; c < nc; ++c) {
    const int64_t wc = (s.chain_last.at((size_t)c) ? 0 : nz(c + 1)) + d.nb;
    need(s.chainG_off.at((size_t)c) >= 0 && s.chainG_off.at((size_t)c) + wc <= s.n_chainG, "chainG_off");
    need(s.leaf_of_left.at((size_t)c) >= -1 && s.leaf_of_left.at((size_t)c) < d.n_leaf, "leaf_of_left range");
  }
  need((int64_t)s.mv_src.size() == d.n_mv, "mv_src");
  need((int64_t)s.mv_long.size() == s.n_mv_long && (int64_t)s.mv_long_c0.size() == s.n_mv_long + 1, "mv_long");
  need((int64_t)s.mv_chunk_e0.size() == s.n_mv_chunks && (int64_t)s.mv_chunk_e1.size() == s.n_mv_chunks, "mv_chunk");
  need(s.n_mv_long_part >= 1 && s.n_mv_long_part >= s.n_mv_chunks, "mv_long_part");
  for (int64_t i = 0; i < s.n_mv_long; ++i) {
    need(s.mv_long.at((size_t)i) >= 0 && s.mv_long.at((size_t)i) < d.nu, "mv_long row");
    for (int64_t q = s.mv_long_c0.at((size_t)i); q < s.mv_long_c0.at((size_t)i + 1); ++q)
      need(s.mv_chunk_e0.at((size_t)q) >= 0 && s.mv_chunk_e0.at((size_t)q) < s.mv_chunk_e1.at((size_t)q) && s.mv_chunk_e1.at((size_t)q) <= d.n_mv,
           "mv_chunk range");
  }
  if (s.chain_cr) {
    const CrPlan& P = s.cr;
    need((int64_t)s.cr_nodes.size() == nc && s.cr_lvl_ptr.at(0) == 0 && s.cr_lvl_ptr.back() == nc, "level lists");
    for (size_t l = 1; l < s.cr_lvl_ptr.size(); ++l) need(s.cr_lvl_ptr[l - 1] <= s.cr_lvl_ptr[l], "cr_lvl_ptr order");
    for (int64_t c : s.cr_nodes) need(c >= 0 && c < nc, "cr_nodes");
    for (int64_t c = 0; c < nc; ++c) {
      const int64_t a = P.ca.at((size_t)c), b = P.cb.at((size_t)c);
      need(a >= -1 && a < nc && b >= -1 && b < nc, "separators");
      const int64_t w = (a >= 0 ? nz(a) : 0) + (b >= 0 ? nz(b) : 0) + d.nb;
      need(P.oP.at((size_t)c) >= 0 && P.oP.at((size_t)c) + nz(c) * (nz(c) + w) <= s.n_crbuf, "crP_off");
      need(P.oS.at((size_t)c) >= 0 && P.oS.at((size_t)c) + w * w <= s.n_crbuf, "crS_off");
      need(P.oG.at((size_t)c) >= 0 && P.oG.at((size_t)c) + w <= s.n_crbuf, "crG_off");
      need(P.pull_ptr.at((size_t)c) <= P.pull_ptr.at((size_t)c + 1) && P.pull_ptr.at((size_t)c + 1) <= (int64_t)P.pull_e.size(), "pull_ptr");
      for (int64_t e = P.pull_ptr[(size_t)c]; e < P.pull_ptr[(size_t)c + 1]; ++e)
        need((P.pull_e.at((size_t)e) >> 1) >= 0 && (P.pull_e.at((size_t)e) >> 1) < nc, "pull_e");
    }
    const size_t L = s.cr_lvl_ptr.size();
    need(s.cr_top_from >= 1 && s.cr_top_from <= L && (size_t)s.cr_top.n == L - s.cr_top_from && s.cr_top.n <= 17, "cr_top range");
    for (int i = 0; s.cr_top.n && i <= s.cr_top.n; ++i) need(s.cr_top.ptr[i] == s.cr_lvl_ptr.at(s.cr_top_from - 1 + (size_t)i), "cr_top.ptr");
    if (s.cr_top.n) need(s.cr_top_waves >= 2 && (int64_t)s.cr_top_lds == (int64_t)s.cr_top_waves * s.cr_top.wave_bytes && s.cr_top_lds <= pck::LDS_WORKGROUP, "cr_top lds");
    for (int64_t c : s.export_nodes) need(c >= 0 && c < nc && P.exported.at((size_t)c), "export_nodes");
  }
  need(s.n_border_part == (int64_t)s.border_blocks * d.nb * d.nb, "border_part");
  need(s.n_counts == 2 * (d.n_leaf + d.n_chain + 1) && s.n_vec == d.nu && s.n_vals == d.total_vals, "scratch counts");
}

static I64 values(std::istringstream& in) {
  I64 v;
  std::string tok;
  while (in >> tok) {
    const size_t x = tok.find('x');
    if (x == std::string::npos) v.push_back(std::atoll(tok.c_str()));
    else v.insert(v.end(), (size_t)std::atoll(tok.c_str() + x + 1), std::atoll(tok.substr(0, x).c_str()));
  }
  return v;
}

static void run(const std::string& name, int64_t nb, const I64& chain, const I64& seg, const I64& leaf, I64 left, bool has_left,
                const I64& rows, const std::vector<I64>& entries, const I64& exp, const pck::Knobs& kn) {
  std::printf("case %s\n", name.c_str());
  const int64_t nc = (int64_t)chain.size(), nl = (int64_t)leaf.size(), nu = (int64_t)rows.size();
  I64 chain_ptr(1, 0), leaf_ptr(1, 0), mv_ptr(1, 0);
  for (int64_t v : chain) chain_ptr.push_back(chain_ptr.back() + v);
  for (int64_t v : leaf) leaf_ptr.push_back(leaf_ptr.back() + v);
  for (int64_t v : rows) mv_ptr.push_back(mv_ptr.back() + v);
  if (!has_left) {
    std::vector<uint8_t> last((size_t)nc, 0);
    for (size_t p = 1; p < seg.size(); ++p) last.at((size_t)seg[p] - 1) = 1;
    for (int64_t c = 0; c < nc && (int64_t)left.size() < nl; ++c)
      if (!last[(size_t)c]) left.push_back(c);
  }
  need((int64_t)left.size() == nl, "one left node per leaf");
  const int64_t n_mv = mv_ptr.back();
  std::vector<int32_t> mv_idx((size_t)n_mv), mv_kind((size_t)n_mv);
  for (int64_t e = 0; e < n_mv; ++e) { mv_idx[(size_t)e] = (int32_t)(e % 1000); mv_kind[(size_t)e] = (int32_t)(e % 3); }
  for (const I64& t : entries) { mv_idx.at((size_t)t.at(0)) = (int32_t)t.at(1); mv_kind.at((size_t)t.at(0)) = (int32_t)t.at(2); }
  std::vector<uint8_t> exp8(exp.begin(), exp.end());
  need(exp8.empty() || (int64_t)exp8.size() == nc, "one export flag per chain node");
  pc_kkt_desc d{};
  d.nu = nu; d.n_leaf = nl; d.n_chain = nc; d.n_phase = (int64_t)seg.size() - 1; d.nb = nb; d.n_mv = n_mv;
  d.total_vals = leaf_ptr.back() * 3 + 7;
  d.leaf_ptr = leaf_ptr.data(); d.chain_ptr = chain_ptr.data(); d.chain_phase_ptr = seg.data(); d.leaf_left = left.data();
  d.mv_ptr = mv_ptr.data(); d.mv_idx = mv_idx.data(); d.mv_kind = mv_kind.data();
  d.chain_export = exp8.empty() ? nullptr : exp8.data();
  pck::Shape s;
  try {
    s = pck::build_shape(d, kn);
  } catch (const std::runtime_error& e) {
    std::printf("error %s\nend\n", e.what());
    return;
  }
  walk(d, s);
  line("chain_last", s.chain_last); line("leaf_of_left", s.leaf_of_left); line("leafG_off", s.leafG_off); line("chainG_off", s.chainG_off);
  num("n_leafG", s.n_leafG); num("n_chainG", s.n_chainG);
  unsigned long long h = 1469598103934665603ull;   // FNV-1a of the packed words (the test packs them itself)
  for (uint32_t w : s.mv_src) h = (h ^ w) * 1099511628211ull;
  std::printf("mv_src_hash %llu\n", h);
  line("mv_long", s.mv_long); line("mv_long_c0", s.mv_long_c0); line("mv_chunk_e0", s.mv_chunk_e0); line("mv_chunk_e1", s.mv_chunk_e1);
  num("n_mv_long", s.n_mv_long); num("n_mv_chunks", s.n_mv_chunks); num("n_mv_long_part", s.n_mv_long_part);
  num("lds_leaf", s.lds_leaf); num("lds_leaf_full", s.lds_leaf_full); num("lds_chain", s.lds_chain);
  num("lds_chain_factor", s.lds_chain_factor); num("chain_lds", s.chain_lds); num("nzmax", s.nzmax); num("wcmax", s.wcmax);
  num("lds_border", s.lds_border);
  num("chain_cr", s.chain_cr); num("any_export", s.any_export);
  if (s.chain_cr) {
    line("cr_lvl_ptr", s.cr_lvl_ptr); line("cr_nodes", s.cr_nodes); line("export_nodes", s.export_nodes);
    num("cr_top_from", (long long)s.cr_top_from); num("cr_top_waves", s.cr_top_waves); num("cr_top_lds", s.cr_top_lds);
    num("cr_top_n", s.cr_top.n); num("cr_top_wave_bytes", s.cr_top.wave_bytes);
    line("cr_top_ptr", I64(s.cr_top.ptr, s.cr_top.ptr + (s.cr_top.n ? s.cr_top.n + 1 : 0)));
    num("lds_cr", s.lds_cr); num("n_crbuf", s.n_crbuf);
  }
  num("border_blocks", s.border_blocks); num("n_border_part", s.n_border_part);
  num("n_vals", s.n_vals); num("n_vec", s.n_vec); num("n_counts", s.n_counts);
  num("leaf_forward_stage", pck::leaf_forward_stage(s));
  pc_kkt_info info;
  pck::fill_info(s, -1, &info);
  const long long iv[] = {info.n_leaf, info.n_chain, info.nb, info.n_mv_long, info.chain_cr, info.cr_levels, info.cr_top_levels,
                          info.cr_top_waves, info.border_blocks, info.leaf_forward_stage, info.leaf_waves};
  line("info", std::vector<long long>(iv, iv + 11));
  std::printf("end\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string ln, name;
  int64_t nb = 0;
  I64 chain, seg, leaf, left, rows, exp;
  std::vector<I64> entries;
  bool has_left = false;
  pck::Knobs kn;
  try {
    while (std::getline(f, ln)) {
      std::istringstream in(ln);
      std::string key;
      if (!(in >> key)) continue;
      if (key == "case") {
        in >> name;
        nb = 0; chain.clear(); seg.assign(1, 0); leaf.clear(); left.clear(); rows.clear(); exp.clear(); entries.clear();
        has_left = false; kn = pck::Knobs();
      } else if (key == "nb") in >> nb;
      else if (key == "chain") chain = values(in);
      else if (key == "seg") seg = values(in);
      else if (key == "leaf") leaf = values(in);
      else if (key == "left") { left = values(in); has_left = true; }
      else if (key == "rows") rows = values(in);
      else if (key == "entry") entries.push_back(values(in));
      else if (key == "export") exp = values(in);
      else if (key == "knobs") { int cr = 1; in >> kn.leaf_fwd >> kn.leaf_waves >> cr >> kn.cr_top_cap; kn.cr = cr != 0; }
      else if (key == "end") run(name, nb, chain, seg, leaf, left, has_left, rows, entries, exp, kn);
      else return 2;
    }
  } catch (const std::out_of_range& e) {
    std::fprintf(stderr, "case %s: out of bounds: %s\n", name.c_str(), e.what());
    return 3;
  }
  return 0;
}
