// Host-side colouring plan of the derivative check (pc_check_derivatives_device, pc_deriv_check.hpp): which columns of
// x~ may be perturbed together so that central differences of c~, J~ and grad L recover every stored entry of G~, grad J~
// and H~.  The reference only promises this check (pycollo/settings.py:360-361 check_nlp_functions; pycollo/iteration.py:
// 455-458 raises NotImplementedError); IPOPT's derivative_test perturbs one column at a time (n + 1 evaluations).
//
// Collocation couples node variables within a section only, and a Hessian entry joins variables of one node, so:
//   * node variable v at a node i that is neither the first nor the last of its phase gets colour (v, i mod n_max), n_max
//     the largest number of nodes of any section: two nodes of one section never share a colour, phases share them;
//   * the first / last node of every phase and every global column (q, t0 / tF, s) -- the columns endpoint rows, endpoint
//     Hessian blocks and grad J~ touch -- are "special": coloured greedily, a colour shared only by columns that have no
//     row of G~ (J~ counted as one more row) and no row of the full symmetric H~ in common.
// The number of colours does not grow with the mesh.  The plan is then validated against the real patterns in O(nnz):
// a G~ entry (r, j) is located when j is the only column of its colour in row r, else it is one term of the
// directional-derivative sum of (row r, colour of j); an H~ entry (r, c) of the lower triangle is located from column
// c's colour when row r of the full H~ sees c alone in it, or from r's colour when row c sees r alone.
// Pure C++ (no HIP): unit-testable on a CPU-only machine (tests/c/deriv_plan_sanitize.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "pc_pattern.hpp"

namespace pcd {

struct Plan {
  int32_t n_colours = 0, n_interior = 0, n_max = 0;
  std::vector<int32_t> colour;                 // [n] colour of every column
  std::vector<int64_t> col_ptr;                // [n_colours + 1] ...
  std::vector<int32_t> cols;                   // ... the columns of every colour, ascending
  std::vector<uint8_t> g_flag;                 // [nnz G] 1 located, 0 term of a sum
  std::vector<uint8_t> h_flag;                 // [nnz H] bit 0: located from the column's colour, bit 1: from the row's
  std::vector<uint8_t> j_flag;                 // [n_jgrad] 1 located
  // per colour k, lists in entry order: [x_ptr[k], x_ptr[k + 1])
  std::vector<int64_t> gl_ptr, gl_ent;         // located G~ entries
  std::vector<int64_t> seg_ptr;                // sums (row, colour) of the colour, numbered globally
  std::vector<int32_t> seg_row;                // [n_seg] row of every sum
  std::vector<int64_t> seg_eptr, seg_ent;      // [n_seg + 1], the G~ entries of every sum (ascending column)
  std::vector<int64_t> hl_ptr, hl_ent;         // located H~ entries ...
  std::vector<int32_t> hl_lrow, hl_scol;       // ... the row of grad L the difference is read from, the column whose step divides
  std::vector<int64_t> jl_ptr;
  std::vector<int32_t> jl_ent;                 // located grad J~ non-zeros
  std::vector<int64_t> lr_ptr;
  std::vector<int32_t> lr_rows;                // rows of grad L the colour's H~ entries read (distinct, ascending)
  // G~ by columns (the order grad L = sigma grad J~ + G~^T lambda is summed in): CSR entry index per position
  std::vector<int64_t> csc_ptr, csc_ent;
  std::vector<int32_t> jg_of_col;              // [n] grad J~ non-zero of the column, -1 if none
  int64_t n_g_located = 0, n_g_sum = 0, n_seg = 0, n_h_located = 0, n_h_unlocated = 0, n_j_located = 0;
};

// items stably grouped by their colour: out[ptr[k] .. ptr[k + 1]) = the items of colour k, in input order
template <class T>
inline void bucket(int nc, const std::vector<int32_t>& key, const std::vector<T>& item, std::vector<int64_t>& ptr,
                   std::vector<T>& out) {
  ptr.assign((size_t)nc + 1, 0);
  for (int32_t k : key) ++ptr[(size_t)k + 1];
  for (int k = 0; k < nc; ++k) ptr[k + 1] += ptr[k];
  out.resize(item.size());
  std::vector<int64_t> pos(ptr.begin(), ptr.end() - 1);
  for (size_t i = 0; i < item.size(); ++i) out[(size_t)pos[key[i]]++] = item[i];
}

inline Plan build_plan(const pcp::Problem& Q) {
  Plan P;
  const int64_t n = Q.num_x, m = Q.num_c;
  const int64_t nG = (int64_t)Q.g_col.size(), nH = (int64_t)Q.h_col.size();
  if ((int64_t)Q.g_indptr.size() != m + 1 || (int64_t)Q.h_indptr.size() != n + 1)
    throw std::runtime_error("derivative plan: the handle has no patterns (plan-only handle)");
  int n_max = 2, max_nz = 0;
  for (const auto& ph : Q.ph) {
    for (int32_t nk : ph.n_k) n_max = std::max(n_max, (int)nk);
    max_nz = std::max(max_nz, ph.n_z);
  }
  P.n_max = n_max;
  // ---- classify: raw interior colour v * n_max + i mod n_max, or special (-1)
  const int n_raw = max_nz * n_max;
  std::vector<int32_t> raw(n, -1);
  for (const auto& ph : Q.ph)
    for (int v = 0; v < ph.n_z; ++v)
      for (int i = 1; i + 1 < ph.N; ++i) raw[ph.x_off + (int64_t)v * ph.N + i] = v * n_max + i % n_max;
  // compact the interior colours to the ones used
  std::vector<int32_t> used(n_raw, -1);
  for (int64_t j = 0; j < n; ++j)
    if (raw[j] >= 0) used[raw[j]] = 0;
  int ni = 0;
  for (int k = 0; k < n_raw; ++k)
    if (used[k] == 0) used[k] = ni++;
  P.colour.assign(n, -1);
  for (int64_t j = 0; j < n; ++j)
    if (raw[j] >= 0) P.colour[j] = used[raw[j]];
  P.n_interior = ni;
  // ---- G~ by columns
  P.csc_ptr.assign(n + 1, 0);
  for (int64_t e = 0; e < nG; ++e) ++P.csc_ptr[(size_t)Q.g_col[e] + 1];
  for (int64_t j = 0; j < n; ++j) P.csc_ptr[j + 1] += P.csc_ptr[j];
  P.csc_ent.resize(nG);
  {
    std::vector<int64_t> pos(P.csc_ptr.begin(), P.csc_ptr.end() - 1);
    for (int64_t e = 0; e < nG; ++e) P.csc_ent[(size_t)pos[Q.g_col[e]]++] = e;
  }
  // ---- full symmetric H~ by rows: (column, lower entry, 0 = stored orientation / 1 = transposed)
  std::vector<int64_t> fh_ptr(n + 1, 0);
  for (int64_t e = 0; e < nH; ++e) {
    ++fh_ptr[(size_t)Q.h_row[e] + 1];
    if (Q.h_row[e] != Q.h_col[e]) ++fh_ptr[(size_t)Q.h_col[e] + 1];
  }
  for (int64_t j = 0; j < n; ++j) fh_ptr[j + 1] += fh_ptr[j];
  std::vector<int32_t> fh_col(fh_ptr[n]);
  std::vector<int64_t> fh_ent(fh_ptr[n]);
  {
    std::vector<int64_t> pos(fh_ptr.begin(), fh_ptr.end() - 1);
    for (int64_t e = 0; e < nH; ++e) {
      const int32_t r = Q.h_row[e], c = Q.h_col[e];
      fh_col[pos[r]] = c;
      fh_ent[pos[r]++] = e << 1;
      if (r != c) {
        fh_col[pos[c]] = r;
        fh_ent[pos[c]++] = (e << 1) | 1;
      }
    }
  }
  // ---- grad J~ columns
  P.jg_of_col.assign(n, -1);
  const int64_t nJ = (int64_t)Q.jgrad_col.size();
  for (int64_t e = 0; e < nJ; ++e) P.jg_of_col[Q.point_x[Q.jgrad_col[e]]] = (int32_t)e;
  // ---- greedy colours of the special columns, in x order: rows of G~ (+ the J~ row m) and of the full H~
  {
    std::vector<std::vector<int32_t>> g_seen(m + 1), h_seen(n);   // special colours already present in a row
    std::vector<int64_t> stamp;
    int ns = 0;
    for (int64_t j = 0; j < n; ++j) {
      if (P.colour[j] >= 0) continue;
      auto forbid = [&](const std::vector<int32_t>& cs) {
        for (int32_t c : cs) stamp[c] = j;
      };
      stamp.resize((size_t)ns + 1, -1);
      for (int64_t p = P.csc_ptr[j]; p < P.csc_ptr[j + 1]; ++p) forbid(g_seen[Q.g_row[P.csc_ent[p]]]);
      if (P.jg_of_col[j] >= 0) forbid(g_seen[m]);
      for (int64_t p = fh_ptr[j]; p < fh_ptr[j + 1]; ++p) forbid(h_seen[fh_col[p]]);
      int c = 0;
      while (stamp[c] == j) ++c;
      if (c == ns) ++ns;
      for (int64_t p = P.csc_ptr[j]; p < P.csc_ptr[j + 1]; ++p) g_seen[Q.g_row[P.csc_ent[p]]].push_back(c);
      if (P.jg_of_col[j] >= 0) g_seen[m].push_back(c);
      for (int64_t p = fh_ptr[j]; p < fh_ptr[j + 1]; ++p) h_seen[fh_col[p]].push_back(c);
      P.colour[j] = ni + c;
    }
    P.n_colours = ni + ns;
  }
  const int nc = P.n_colours;
  {
    std::vector<int32_t> all(n);
    for (int64_t j = 0; j < n; ++j) all[j] = (int32_t)j;
    bucket(nc, P.colour, all, P.col_ptr, P.cols);
  }
  // ---- validate G~: located entries, sums per (row, colour)
  std::vector<int32_t> cnt(nc, 0);
  std::vector<int64_t> seg_of(nc, -1);
  P.g_flag.assign(nG, 0);
  std::vector<int32_t> gl_key, seg_key;
  std::vector<int64_t> gl_item;
  std::vector<int64_t> seg_items;          // entries of the sums, grouped by sum (in order of creation)
  std::vector<int64_t> seg_start;          // first item of every sum
  for (int64_t r = 0; r < m; ++r) {
    const int64_t b = Q.g_indptr[r], e1 = Q.g_indptr[r + 1];
    for (int64_t e = b; e < e1; ++e) ++cnt[P.colour[Q.g_col[e]]];
    // every sum of the row collects its entries in column order: a row's sums are contiguous in seg_items
    std::vector<int64_t> row_segs;
    for (int64_t e = b; e < e1; ++e) {
      const int32_t k = P.colour[Q.g_col[e]];
      if (cnt[k] == 1) {
        P.g_flag[e] = 1;
        gl_key.push_back(k);
        gl_item.push_back(e);
      } else if (seg_of[k] < 0) {
        seg_of[k] = (int64_t)row_segs.size();
        row_segs.push_back(k);
      }
    }
    for (int32_t k : row_segs) {
      seg_start.push_back((int64_t)seg_items.size());
      seg_key.push_back(k);
      P.seg_row.push_back((int32_t)r);
      for (int64_t e = b; e < e1; ++e)
        if (P.colour[Q.g_col[e]] == k) seg_items.push_back(e);
      seg_of[k] = -1;
    }
    for (int64_t e = b; e < e1; ++e) cnt[P.colour[Q.g_col[e]]] = 0;
  }
  P.n_g_located = (int64_t)gl_item.size();
  P.n_g_sum = nG - P.n_g_located;
  bucket(nc, gl_key, gl_item, P.gl_ptr, P.gl_ent);
  {   // sums renumbered colour by colour
    const int64_t ns = (int64_t)seg_key.size();
    seg_start.push_back((int64_t)seg_items.size());
    std::vector<int64_t> ids(ns);
    for (int64_t s = 0; s < ns; ++s) ids[s] = s;
    std::vector<int64_t> order;
    bucket(nc, seg_key, ids, P.seg_ptr, order);
    std::vector<int32_t> rows(ns);
    P.seg_eptr.assign(ns + 1, 0);
    P.seg_ent.clear();
    for (int64_t t = 0; t < ns; ++t) {
      const int64_t s = order[t];
      rows[t] = P.seg_row[s];
      for (int64_t i = seg_start[s]; i < seg_start[s + 1]; ++i) P.seg_ent.push_back(seg_items[i]);
      P.seg_eptr[t + 1] = (int64_t)P.seg_ent.size();
    }
    P.seg_row = rows;
    P.n_seg = ns;
  }
  // ---- validate H~ on the full rows
  P.h_flag.assign(nH, 0);
  for (int64_t r = 0; r < n; ++r) {
    for (int64_t p = fh_ptr[r]; p < fh_ptr[r + 1]; ++p) ++cnt[P.colour[fh_col[p]]];
    for (int64_t p = fh_ptr[r]; p < fh_ptr[r + 1]; ++p)
      if (cnt[P.colour[fh_col[p]]] == 1) P.h_flag[fh_ent[p] >> 1] |= (fh_ent[p] & 1) ? 2 : 1;
    for (int64_t p = fh_ptr[r]; p < fh_ptr[r + 1]; ++p) cnt[P.colour[fh_col[p]]] = 0;
  }
  std::vector<int32_t> hl_key;
  std::vector<int64_t> hl_item;
  for (int64_t e = 0; e < nH; ++e) {
    if (!P.h_flag[e]) {
      ++P.n_h_unlocated;
      continue;
    }
    const int32_t r = Q.h_row[e], c = Q.h_col[e];
    hl_key.push_back(P.colour[(P.h_flag[e] & 1) ? c : r]);
    hl_item.push_back(e);
  }
  P.n_h_located = (int64_t)hl_item.size();
  bucket(nc, hl_key, hl_item, P.hl_ptr, P.hl_ent);
  P.hl_lrow.resize(P.hl_ent.size());
  P.hl_scol.resize(P.hl_ent.size());
  for (size_t i = 0; i < P.hl_ent.size(); ++i) {
    const int64_t e = P.hl_ent[i];
    const int32_t r = Q.h_row[e], c = Q.h_col[e];
    const bool cside = P.h_flag[e] & 1;
    P.hl_lrow[i] = cside ? r : c;
    P.hl_scol[i] = cside ? c : r;
  }
  // rows of grad L each colour reads
  {
    std::vector<int32_t> mark(n, -1);
    P.lr_ptr.assign((size_t)nc + 1, 0);
    for (int k = 0; k < nc; ++k) {
      const size_t first = P.lr_rows.size();
      for (int64_t i = P.hl_ptr[k]; i < P.hl_ptr[k + 1]; ++i)
        if (mark[P.hl_lrow[i]] != k) {
          mark[P.hl_lrow[i]] = k;
          P.lr_rows.push_back(P.hl_lrow[i]);
        }
      std::sort(P.lr_rows.begin() + first, P.lr_rows.end());
      P.lr_ptr[k + 1] = (int64_t)P.lr_rows.size();
    }
  }
  // ---- grad J~ (one row)
  P.j_flag.assign(nJ, 0);
  std::vector<int32_t> jl_key, jl_item;
  for (int64_t e = 0; e < nJ; ++e) ++cnt[P.colour[Q.point_x[Q.jgrad_col[e]]]];
  for (int64_t e = 0; e < nJ; ++e) {
    const int32_t k = P.colour[Q.point_x[Q.jgrad_col[e]]];
    if (cnt[k] == 1) {
      P.j_flag[e] = 1;
      jl_key.push_back(k);
      jl_item.push_back((int32_t)e);
    }
  }
  P.n_j_located = (int64_t)jl_item.size();
  bucket(nc, jl_key, jl_item, P.jl_ptr, P.jl_ent);
  return P;
}

}  // namespace pcd
