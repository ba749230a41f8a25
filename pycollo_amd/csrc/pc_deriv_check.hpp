// Derivative check of G~, grad J~ and H~ by coloured central differences (pc_check_derivatives_device).  The reference
// promises the check (pycollo/settings.py:360-361 check_nlp_functions) and raises NotImplementedError where it would run
// (pycollo/iteration.py:455-458); IPOPT's derivative_test perturbs one column at a time.  Here the columns of one colour
// of the plan (pc_deriv.hpp) move together, so a check costs 1 + 2 x colours evaluations at any mesh size:
//   per colour S: deriv_perturb writes x~ + h_S and x~ - h_S into two scratch vectors and puts the previous colour's
//   columns back (O(|S|)); the evaluations at both
//   points go through launch_all with the checker's own c / G / J / grad J buffers (flags c + G: what both the Jacobian
//   and the Hessian differences read); deriv_lagrangian_grad forms grad L(x+) - grad L(x-), grad L = sigma grad J~ +
//   G~^T lambda, for the rows the colour's H~ entries read, one wave per chunk of a column in CSC order; deriv_compare turns every
//   entry of the colour's lists into an error (one lane per located entry, one wave per sum).
// Then deriv_reduce_* finds the largest error per kind (lowest index on ties), the failure counts and, in entry order,
// the first max_report failures: only those come back to the host, with one synchronisation.  Nothing uses atomics:
// the report is bit-reproducible.
// Included at the end of pc_engine.hip (same translation unit: it launches the evaluation through launch_all).
#pragma once

#include <cfloat>

struct pc_deriv_dev {
  int64_t nG = 0, nH = 0, nJ = 0, nS = 0, T = 0;
  int nb_red = 1;
  DevBuf<int32_t> cols, g_row, g_col, h_row, h_col, hl_lrow, hl_scol, seg_row, seg_colour, lr_rows, jg_of_col, jl_ent, jcol;
  DevBuf<int64_t> gl_ent, seg_eptr, seg_ent, hl_ent, csc_ptr, csc_ent;
  // grad L rows cut into chunks (deriv_lagrangian_grad), per colour [ch_ptr[k], ch_ptr[k + 1]); rows of several chunks
  std::vector<int64_t> ch_ptr, mr_ptr;
  DevBuf<int32_t> ch_row, mr_row;
  DevBuf<int64_t> ch_p0, ch_p1, mr_c0, mr_c1;
  DevBuf<double> part;
  DevBuf<double> xp, xm, step2, cP, cM, GP, GM, f3, gnP, gnM, c0, G0, H0, gn0, lam, dL, err, fdG, fdH, fdJ, segA, segF;
  DevBuf<double> r_max;
  DevBuf<int64_t> r_idx, r_cnt, r_pfx;
  DevBuf<char> out;      // DerivOut
  PinBuf<char> h_out;
  PinBuf<double> h_lam;
  DevBuf<char> saved;    // the handle's hand-over buffers, kept aside during a check
};

namespace {

struct DerivOut {
  double max_err[4];
  int64_t argmax[4], n_fail[4];
  pc_deriv_entry worst[3];
  pc_deriv_entry fail[PC_DERIV_MAX_REPORT];
};

constexpr int DERIV_THREADS = 256;

struct DerivView {   // what the compare / reduce kernels read, by value
  const int32_t *g_row, *g_col, *h_row, *h_col, *seg_row, *seg_colour, *jcol;
  const double *Gan, *Han, *Jan, *fdG, *fdH, *fdJ, *segA, *segF, *err;
  int64_t nG, nS, nH, nJ;
};

__device__ __forceinline__ double deriv_err(double num, double den) {
  const double e = num / den;
  return (e <= DBL_MAX) ? e : INFINITY;   // NaN / inf (of a value or of the quotient) count as +inf
}

// x~ -/+ h on the columns of the current colour; the previous colour's columns (prev) are put back to x~ in the same launch
__global__ void deriv_perturb(const double* __restrict__ x, double* __restrict__ xp, double* __restrict__ xm,
                              double* __restrict__ step2, const int32_t* __restrict__ prev, int64_t n_prev,
                              const int32_t* __restrict__ cols, int64_t n_cols, double delta) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_prev) {
    const int32_t j = prev[i];
    xp[j] = x[j];
    xm[j] = x[j];
    return;
  }
  i -= n_prev;
  if (i >= n_cols) return;
  const int32_t j = cols[i];
  const double xj = x[j];
  const double h = delta * fmax(1.0, fabs(xj));
  const double a = xj + h, b = xj - h;
  xp[j] = a;
  xm[j] = b;
  step2[j] = a - b;   // the step the arithmetic actually took
}

__device__ __forceinline__ double wave_sum(double v) {   // fixed tree: lane 0 ends with the sum in the same order every time
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// grad L(x+) - grad L(x-) for the rows of grad L (= columns of G~) the colour's H~ entries read: sigma (grad J+ - grad J-)
// + the column's (G+ - G-) lambda_r in row order.  A column is cut into chunks of at most DERIV_CHUNK entries (a free
// time's column runs through every defect row of its phase), one wave per chunk: lane l sums the entries l, l + 64, ...,
// then a fixed shuffle tree.  A column of one chunk is finished there; the chunks of a longer one go to `part` and
// deriv_lagrangian_sum adds them in chunk order.
constexpr int64_t DERIV_CHUNK = 1024;
__global__ void deriv_lagrangian_grad(const int32_t* __restrict__ ch_row, const int64_t* __restrict__ ch_p0,
                                      const int64_t* __restrict__ ch_p1, int64_t n_ch, const int64_t* __restrict__ csc_ent,
                                      const int32_t* __restrict__ g_row, const double* __restrict__ GP,
                                      const double* __restrict__ GM, const double* __restrict__ lam,
                                      const double* __restrict__ gnP, const double* __restrict__ gnM,
                                      const int32_t* __restrict__ jg_of_col, double sigma, double* __restrict__ dL,
                                      double* __restrict__ part) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (w >= n_ch) return;
  const int32_t q = ch_row[w];
  double acc = 0.0;
  for (int64_t p = ch_p0[w] + lane; p < ch_p1[w]; p += 64) {
    const int64_t e = csc_ent[p];
    acc += (GP[e] - GM[e]) * lam[g_row[e]];
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    if (q >= 0) {
      const int32_t g = jg_of_col[q];
      dL[q] = (g >= 0 ? sigma * (gnP[g] - gnM[g]) : 0.0) + acc;
    } else {
      part[w] = acc;   // (a chunk of a long column: ch_row = -1 - the column)
    }
  }
}

__global__ void deriv_lagrangian_sum(const int32_t* __restrict__ mr_row, const int64_t* __restrict__ mr_c0,
                                     const int64_t* __restrict__ mr_c1, int64_t n_mr, const double* __restrict__ part,
                                     const double* __restrict__ gnP, const double* __restrict__ gnM,
                                     const int32_t* __restrict__ jg_of_col, double sigma, double* __restrict__ dL) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_mr) return;
  const int32_t q = mr_row[i];
  double acc = 0.0;
  for (int64_t c = mr_c0[i]; c < mr_c1[i]; ++c) acc += part[c];
  const int32_t g = jg_of_col[q];
  dL[q] = (g >= 0 ? sigma * (gnP[g] - gnM[g]) : 0.0) + acc;
}

struct DerivColour {
  const int64_t* gl_ent;   // located G~ entries of the colour
  const int32_t* seg_row;  // the colour's sums (already offset to its first)
  const int64_t* seg_eptr;
  const int64_t* hl_ent;
  const int32_t *hl_lrow, *hl_scol, *jl_ent;
  int64_t n_gl, n_seg, n_hl, n_jl, seg0;
};

// blocks [0, nb_loc): one lane per located entry (G~, H~, grad J~); the blocks after them: one wave per sum
__global__ void deriv_compare(DerivColour L, int nb_loc, const int32_t* __restrict__ g_row, const int32_t* __restrict__ g_col,
                              const int64_t* __restrict__ seg_ent, const int32_t* __restrict__ jcol,
                              const double* __restrict__ step2, const double* __restrict__ cP, const double* __restrict__ cM,
                              const double* __restrict__ fPM, const double* __restrict__ dL, const double* __restrict__ Gan,
                              const double* __restrict__ Han, const double* __restrict__ Jan, double* __restrict__ errG,
                              double* __restrict__ errS, double* __restrict__ errH, double* __restrict__ errJ,
                              double* __restrict__ fdG, double* __restrict__ fdH, double* __restrict__ fdJ,
                              double* __restrict__ segA, double* __restrict__ segF) {
  if ((int)blockIdx.x >= nb_loc) {   // sum_j an_j h_j against (c+_r - c-_r) / 2, relative to its largest term
    const int64_t i = ((int64_t)(blockIdx.x - nb_loc) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= L.n_seg) return;
    const int32_t r = L.seg_row[i];
    double sum = 0.0, big = 0.0, hmax = 0.0, bad = 0.0;
    for (int64_t p = L.seg_eptr[i] + lane; p < L.seg_eptr[i + 1]; p += 64) {
      const int64_t e = seg_ent[p];
      const double h = 0.5 * step2[g_col[e]], an = Gan[e];
      sum += an * h;
      big = fmax(big, fabs(an) * h);
      hmax = fmax(hmax, h);
      bad = fabs(an) <= DBL_MAX ? bad : 1.0;
      fdG[e] = NAN;
      errG[e] = -1.0;   // (judged as a sum: never a located entry's maximum or failure)
    }
    sum = wave_sum(sum);
    big = wave_max(big);
    hmax = wave_max(hmax);
    bad = wave_max(bad);
    if (lane == 0) {
      const double fd = 0.5 * (cP[r] - cM[r]);
      segA[L.seg0 + i] = sum;
      segF[L.seg0 + i] = fd;
      errS[L.seg0 + i] = bad == 0.0 ? deriv_err(fabs(sum - fd), fmax(big, hmax)) : INFINITY;
    }
    return;
  }
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L.n_gl) {
    const int64_t e = L.gl_ent[i];
    const int32_t r = g_row[e];
    const double fd = (cP[r] - cM[r]) / step2[g_col[e]], an = Gan[e];
    fdG[e] = fd;
    errG[e] = deriv_err(fabs(an - fd), fmax(1.0, fabs(an)));
    return;
  }
  i -= L.n_gl;
  if (i < L.n_hl) {
    const int64_t e = L.hl_ent[i];
    const double fd = dL[L.hl_lrow[i]] / step2[L.hl_scol[i]], an = Han[e];
    fdH[e] = fd;
    errH[e] = deriv_err(fabs(an - fd), fmax(1.0, fabs(an)));
    return;
  }
  i -= L.n_hl;
  if (i < L.n_jl) {
    const int32_t g = L.jl_ent[i];
    const double fd = (fPM[0] - fPM[1]) / step2[jcol[g]], an = Jan[g];
    fdJ[g] = fd;
    errJ[g] = deriv_err(fabs(an - fd), fmax(1.0, fabs(an)));
  }
}

__device__ __forceinline__ int deriv_kind(const DerivView& V, int64_t t, int64_t& idx) {
  if (t < V.nG) { idx = t; return PC_DERIV_JAC; }
  t -= V.nG;
  if (t < V.nS) { idx = t; return PC_DERIV_JAC_SUM; }
  t -= V.nS;
  if (t < V.nH) { idx = t; return PC_DERIV_HESS; }
  idx = t - V.nH;
  return PC_DERIV_GRAD;
}

__device__ pc_deriv_entry deriv_entry(const DerivView& V, int64_t t) {
  pc_deriv_entry o;
  int64_t i = 0;
  o.kind = deriv_kind(V, t, i);
  o.index = i;
  o.located = o.kind != PC_DERIV_JAC_SUM;
  o.err = V.err[t];
  switch (o.kind) {
    case PC_DERIV_JAC: o.row = V.g_row[i]; o.col = V.g_col[i]; o.analytic = V.Gan[i]; o.fd = V.fdG[i]; break;
    case PC_DERIV_JAC_SUM: o.row = V.seg_row[i]; o.col = V.seg_colour[i]; o.analytic = V.segA[i]; o.fd = V.segF[i]; break;
    case PC_DERIV_HESS: o.row = V.h_row[i]; o.col = V.h_col[i]; o.analytic = V.Han[i]; o.fd = V.fdH[i]; break;
    default: o.row = -1; o.col = V.jcol[i]; o.analytic = V.Jan[i]; o.fd = V.fdJ[i]; break;
  }
  return o;
}

// (max, lowest index) of the pair
__device__ __forceinline__ void deriv_better(double& m, int64_t& a, double m2, int64_t a2) {
  if (m2 > m || (m2 == m && a2 < a)) { m = m2; a = a2; }
}

// stage 1: every block scans its own contiguous chunk of the concatenated error array [G | sums | H | grad J]
__global__ void __launch_bounds__(DERIV_THREADS) deriv_reduce_blocks(DerivView V, int64_t chunk, double tol,
                                                                     double* __restrict__ r_max, int64_t* __restrict__ r_idx,
                                                                     int64_t* __restrict__ r_cnt) {
  __shared__ double sm[4][DERIV_THREADS];
  __shared__ int64_t si[4][DERIV_THREADS], sc[4][DERIV_THREADS];
  const int tid = threadIdx.x;
  const int64_t T = V.nG + V.nS + V.nH + V.nJ;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < T ? b0 + chunk : T;
  double mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int64_t ax[4] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX}, cn[4] = {0, 0, 0, 0};
  for (int64_t t = b0 + tid; t < b1; t += DERIV_THREADS) {
    int64_t i;
    const int k = deriv_kind(V, t, i);
    const double e = V.err[t];
    deriv_better(mx[k], ax[k], e, t);
    cn[k] += e > tol ? 1 : 0;
  }
  for (int k = 0; k < 4; ++k) { sm[k][tid] = mx[k]; si[k][tid] = ax[k]; sc[k][tid] = cn[k]; }
  __syncthreads();
  for (int s = DERIV_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 4; ++k) {
        deriv_better(sm[k][tid], si[k][tid], sm[k][tid + s], si[k][tid + s]);
        sc[k][tid] += sc[k][tid + s];
      }
    __syncthreads();
  }
  if (tid < 4) {
    r_max[4 * blockIdx.x + tid] = sm[tid][0];
    r_idx[4 * blockIdx.x + tid] = si[tid][0];
    r_cnt[4 * blockIdx.x + tid] = sc[tid][0];
  }
}

// stage 2 (one wave): the blocks' partials in block order; exclusive prefix of every block's failures; the worst entries
__global__ void deriv_reduce_final(DerivView V, int nb, const double* __restrict__ r_max, const int64_t* __restrict__ r_idx,
                                   const int64_t* __restrict__ r_cnt, int64_t* __restrict__ r_pfx, DerivOut* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < 4) {
    double m = -INFINITY;
    int64_t a = INT64_MAX, c = 0;
    for (int b = 0; b < nb; ++b) {
      deriv_better(m, a, r_max[4 * b + k], r_idx[4 * b + k]);
      c += r_cnt[4 * b + k];
    }
    out->max_err[k] = m;
    out->argmax[k] = a;
    out->n_fail[k] = c;
  }
  __syncthreads();
  if (k == 0) {
    int64_t s = 0;
    for (int b = 0; b < nb; ++b) {
      r_pfx[b] = s;
      s += r_cnt[4 * b] + r_cnt[4 * b + 1] + r_cnt[4 * b + 2] + r_cnt[4 * b + 3];
    }
    r_pfx[nb] = s;
    // G~: the located entries and the sums together
    double m = out->max_err[0];
    int64_t a = out->argmax[0];
    deriv_better(m, a, out->max_err[1], out->argmax[1]);
    const int64_t w[3] = {a, out->argmax[2], out->argmax[3]};
    for (int j = 0; j < 3; ++j) {
      if (w[j] != INT64_MAX) {
        out->worst[j] = deriv_entry(V, w[j]);
      } else {
        out->worst[j] = pc_deriv_entry{};
        out->worst[j].kind = -1;
      }
    }
  }
}

// stage 3: every block with failures among the first max_report writes them, ranked in entry order
__global__ void __launch_bounds__(DERIV_THREADS) deriv_compact(DerivView V, int64_t chunk, double tol, int max_report,
                                                               const int64_t* __restrict__ r_pfx, DerivOut* __restrict__ out) {
  __shared__ int64_t wsum[DERIV_THREADS / 64];
  __shared__ int64_t s_base;
  const int64_t T = V.nG + V.nS + V.nH + V.nJ;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = b0 + chunk < T ? b0 + chunk : T;
  if (r_pfx[blockIdx.x] >= max_report || r_pfx[blockIdx.x + 1] == r_pfx[blockIdx.x]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_base = r_pfx[blockIdx.x];
  __syncthreads();
  for (int64_t t0 = b0; t0 < b1; t0 += DERIV_THREADS) {
    const int64_t base = s_base;   // (uniform: read after the barrier)
    if (base >= max_report) break;
    const int64_t t = t0 + tid;
    const bool f = t < b1 && V.err[t] > tol;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int64_t off = 0, tot = 0;
    for (int w = 0; w < DERIV_THREADS / 64; ++w) {
      off += w < wave ? wsum[w] : 0;
      tot += wsum[w];
    }
    const int64_t rank = base + off + before;
    if (f && rank < max_report) out->fail[rank] = deriv_entry(V, t);
    __syncthreads();
    if (tid == 0) s_base = base + tot;
    __syncthreads();
  }
}

inline unsigned deriv_grid(int64_t n) { return (unsigned)((n + DERIV_THREADS - 1) / DERIV_THREADS); }

template <class T>
void deriv_upload(DevBuf<T>& d, const std::vector<T>& v) {
  if (v.empty()) {
    d.alloc(1);   // (a valid pointer for empty lists)
    return;
  }
  d.upload(v);
}

// the plan (host) of a handle with patterns, built once
const pcd::Plan& deriv_plan_of(const pc_handle* h) {
  if (!h->deriv_plan) h->deriv_plan = std::make_shared<pcd::Plan>(pcd::build_plan(h->Q));
  return *h->deriv_plan;
}

pc_deriv_dev& deriv_dev_of(pc_handle* h) {
  if (h->deriv_dev) return *h->deriv_dev;
  const pcd::Plan& P = deriv_plan_of(h);
  const auto& Q = h->Q;
  auto D = std::make_shared<pc_deriv_dev>();
  D->nG = (int64_t)Q.g_col.size();
  D->nH = (int64_t)Q.h_col.size();
  D->nJ = (int64_t)Q.jgrad_col.size();
  D->nS = P.n_seg;
  D->T = D->nG + D->nS + D->nH + D->nJ;
  const int64_t n = Q.num_x, m = Q.num_c;
  deriv_upload(D->cols, P.cols);
  deriv_upload(D->g_row, Q.g_row);
  deriv_upload(D->g_col, Q.g_col);
  deriv_upload(D->h_row, Q.h_row);
  deriv_upload(D->h_col, Q.h_col);
  deriv_upload(D->hl_lrow, P.hl_lrow);
  deriv_upload(D->hl_scol, P.hl_scol);
  deriv_upload(D->seg_row, P.seg_row);
  std::vector<int32_t> seg_colour(P.n_seg);
  for (int k = 0; k < P.n_colours; ++k)
    for (int64_t s = P.seg_ptr[k]; s < P.seg_ptr[k + 1]; ++s) seg_colour[s] = k;
  deriv_upload(D->seg_colour, seg_colour);
  deriv_upload(D->lr_rows, P.lr_rows);
  deriv_upload(D->jg_of_col, P.jg_of_col);
  deriv_upload(D->jl_ent, P.jl_ent);
  std::vector<int32_t> jcol(D->nJ);
  for (int64_t e = 0; e < D->nJ; ++e) jcol[e] = (int32_t)Q.point_x[Q.jgrad_col[e]];
  deriv_upload(D->jcol, jcol);
  deriv_upload(D->gl_ent, P.gl_ent);
  deriv_upload(D->seg_eptr, P.seg_eptr);
  deriv_upload(D->seg_ent, P.seg_ent);
  deriv_upload(D->hl_ent, P.hl_ent);
  deriv_upload(D->csc_ptr, P.csc_ptr);
  {   // the chunks of the grad L rows, colour by colour
    std::vector<int32_t> ch_row, mr_row;
    std::vector<int64_t> ch_p0, ch_p1, mr_c0, mr_c1;
    D->ch_ptr.assign(P.n_colours + 1, 0);
    D->mr_ptr.assign(P.n_colours + 1, 0);
    for (int k = 0; k < P.n_colours; ++k) {
      for (int64_t i = P.lr_ptr[k]; i < P.lr_ptr[k + 1]; ++i) {
        const int32_t q = P.lr_rows[i];
        const int64_t p0 = P.csc_ptr[q], p1 = P.csc_ptr[q + 1];
        const int64_t nch = std::max<int64_t>(1, (p1 - p0 + DERIV_CHUNK - 1) / DERIV_CHUNK);
        if (nch > 1) {
          mr_row.push_back(q);
          mr_c0.push_back((int64_t)ch_row.size());
          mr_c1.push_back((int64_t)ch_row.size() + nch);
        }
        for (int64_t c = 0; c < nch; ++c) {
          ch_row.push_back(nch > 1 ? -1 - q : q);
          ch_p0.push_back(p0 + c * DERIV_CHUNK);
          ch_p1.push_back(std::min(p1, p0 + (c + 1) * DERIV_CHUNK));
        }
      }
      D->ch_ptr[k + 1] = (int64_t)ch_row.size();
      D->mr_ptr[k + 1] = (int64_t)mr_row.size();
    }
    D->part.alloc(std::max<size_t>(ch_row.size(), 1));
    deriv_upload(D->ch_row, ch_row);
    deriv_upload(D->ch_p0, ch_p0);
    deriv_upload(D->ch_p1, ch_p1);
    deriv_upload(D->mr_row, mr_row);
    deriv_upload(D->mr_c0, mr_c0);
    deriv_upload(D->mr_c1, mr_c1);
  }
  deriv_upload(D->csc_ent, P.csc_ent);
  const size_t gmin = (size_t)std::max<int64_t>(D->nG, 1), hmin = (size_t)std::max<int64_t>(D->nH, 1);
  const size_t jmin = (size_t)std::max<int64_t>(D->nJ, 1), smin = (size_t)std::max<int64_t>(D->nS, 1);
  D->xp.alloc(n); D->xm.alloc(n); D->step2.alloc(n); D->dL.alloc(n);
  D->cP.alloc(m + 1); D->cM.alloc(m + 1); D->c0.alloc(m + 1); D->lam.alloc(m + 1);
  D->GP.alloc(gmin); D->GM.alloc(gmin); D->G0.alloc(gmin); D->fdG.alloc(gmin);
  D->H0.alloc(hmin); D->fdH.alloc(hmin);
  D->gnP.alloc(jmin); D->gnM.alloc(jmin); D->gn0.alloc(jmin); D->fdJ.alloc(jmin);
  D->segA.alloc(smin); D->segF.alloc(smin);
  D->f3.alloc(3);
  D->err.alloc((size_t)std::max<int64_t>(D->T, 1));
  D->nb_red = (int)std::min<int64_t>(256, std::max<int64_t>(1, (D->T + 4095) / 4096));
  D->r_max.alloc(4 * D->nb_red);
  D->r_idx.alloc(4 * D->nb_red);
  D->r_cnt.alloc(4 * D->nb_red);
  D->r_pfx.alloc(D->nb_red + 1);
  D->out.alloc(sizeof(DerivOut));
  D->h_out.alloc(sizeof(DerivOut));
  D->h_lam.alloc(m + 1);
  // the hand-over buffers an evaluation writes besides its outputs: restored after the check
  size_t bytes = 0;
  for (auto& pd : h->pd) bytes += pd->partials.n * sizeof(double) + pd->gran.n * sizeof(unsigned long long);
  bytes += h->d_erec.n * sizeof(unsigned long long) + h->d_hb_gran.n * sizeof(unsigned long long);
  D->saved.alloc(std::max<size_t>(bytes, 1));
  h->deriv_dev = D;
  return *D;
}

// copy the hand-over buffers aside (dir = 0) or back (dir = 1)
void deriv_handover(pc_handle* h, pc_deriv_dev& D, int dir, hipStream_t st) {
  size_t off = 0;
  auto one = [&](void* p, size_t bytes) {
    if (!bytes) return;
    char* s = D.saved.p + off;
    HIP_OK(hipMemcpyAsync(dir ? p : s, dir ? s : p, bytes, hipMemcpyDeviceToDevice, st));
    off += bytes;
  };
  for (auto& pd : h->pd) {
    one(pd->partials.p, pd->partials.n * sizeof(double));
    one(pd->gran.p, pd->gran.n * sizeof(unsigned long long));
  }
  one(h->d_erec.p, h->d_erec.n * sizeof(unsigned long long));
  one(h->d_hb_gran.p, h->d_hb_gran.n * sizeof(unsigned long long));
}

// lambda of a check without one: uniform in [-1, 1] (splitmix64)
void deriv_seed_lambda(double* out, int64_t m, uint64_t seed) {
  uint64_t s = seed;
  for (int64_t i = 0; i < m; ++i) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    out[i] = 2.0 * ((double)(z >> 11) * 0x1.0p-53) - 1.0;
  }
}

}  // namespace

extern "C" {

int pc_deriv_plan(const pc_handle* h, int32_t* n_colours, int32_t* colour, uint8_t* jac_flag, uint8_t* hess_flag,
                  uint8_t* jgrad_flag) {
  return guarded(g_err, [&] {
    if (!h) throw std::runtime_error("null handle");
    const pcd::Plan& P = deriv_plan_of(h);
    if (n_colours) *n_colours = P.n_colours;
    if (colour) std::memcpy(colour, P.colour.data(), P.colour.size() * sizeof(int32_t));
    if (jac_flag) std::memcpy(jac_flag, P.g_flag.data(), P.g_flag.size());
    if (hess_flag) std::memcpy(hess_flag, P.h_flag.data(), P.h_flag.size());
    if (jgrad_flag) std::memcpy(jgrad_flag, P.j_flag.data(), P.j_flag.size());
  });
}

int pc_check_derivatives_device(pc_handle* h, const double* d_x, double obj_factor, const double* d_lambda,
                                const double* d_jac_override, const double* d_hess_override, const pc_deriv_opts* opts,
                                pc_deriv_report* report, void* stream) {
  return guarded(g_err, [&] {
    require_device(h);
    if (!d_x || !report) throw std::runtime_error("null x or report");
    for (size_t ip = 0; ip < h->pd.size(); ++ip) {
      const pcl::Range& rg = h->rg[ip];
      if (rg.tile_begin != 0 || rg.tile_end != h->ph[ip].n_tiles || rg.partials_ext)
        throw std::runtime_error("derivative check: phase " + std::to_string(ip) +
                                 " is restricted to a tile range (or hands its partial sums to the caller); a check needs "
                                 "the whole NLP");
    }
    const pcd::Plan& P = deriv_plan_of(h);
    if (P.n_h_unlocated > 0 || P.n_j_located != (int64_t)h->Q.jgrad_col.size())
      throw std::runtime_error("derivative check: the colouring leaves " + std::to_string(P.n_h_unlocated) +
                               " Hessian entries unlocated; this model needs more colours");
    pc_deriv_opts o{};
    if (opts) o = *opts;
    const double tol = o.tol > 0 ? o.tol : 1e-4, delta = o.delta > 0 ? o.delta : 1e-5;
    const int max_report = std::max(0, std::min<int>(o.max_report, PC_DERIV_MAX_REPORT));
    pc_deriv_dev& D = deriv_dev_of(h);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int64_t n = h->Q.num_x, m = h->Q.num_c;
    const double sigma = obj_factor;
    const double* lam = d_lambda;
    if (!lam) {
      deriv_seed_lambda(D.h_lam.p, m, o.seed);
      HIP_OK(hipMemcpyAsync(D.lam.p, D.h_lam.p, m * sizeof(double), hipMemcpyHostToDevice, st));
      lam = D.lam.p;
    }
    deriv_handover(h, D, 0, st);
    // analytic values at x~
    pcl::Call call = device_call(h, d_x, lam, D.c0.p, D.G0.p, D.H0.p);
    call.fobj = D.f3.p + 2;
    call.grad_nz = D.gn0.p;
    call.sigma = sigma;
    launch_all(h, call, st);
    const double* Gan = d_jac_override ? d_jac_override : D.G0.p;
    const double* Han = d_hess_override ? d_hess_override : D.H0.p;
    const double* Jan = o.d_jgrad_override ? o.d_jgrad_override : D.gn0.p;
    HIP_OK(hipMemcpyAsync(D.xp.p, d_x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(D.xm.p, d_x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    double* errG = D.err.p;
    double* errS = errG + D.nG;
    double* errH = errS + D.nS;
    double* errJ = errH + D.nH;
    int64_t prev0 = 0, n_prev = 0;   // the columns of the last colour perturbed (put back by the next perturbation)
    for (int k = 0; k < P.n_colours; ++k) {
      const int64_t c0 = P.col_ptr[k], nc = P.col_ptr[k + 1] - c0;
      if (nc == 0) continue;
      hipLaunchKernelGGL(deriv_perturb, dim3(deriv_grid(n_prev + nc)), dim3(DERIV_THREADS), 0, st, d_x, D.xp.p, D.xm.p,
                         D.step2.p, D.cols.p + prev0, n_prev, D.cols.p + c0, nc, delta);
      prev0 = c0;
      n_prev = nc;
      pcl::Call plus = device_call(h, D.xp.p, nullptr, D.cP.p, D.GP.p, nullptr), minus = device_call(h, D.xm.p, nullptr, D.cM.p, D.GM.p, nullptr);
      plus.fobj = D.f3.p;
      plus.grad_nz = D.gnP.p;
      minus.fobj = D.f3.p + 1;
      minus.grad_nz = D.gnM.p;
      plus.flags = minus.flags = PC_FLAG_C | PC_FLAG_G;
      plus.sigma = minus.sigma = sigma;
      launch_all(h, plus, st);
      launch_all(h, minus, st);
      const int64_t nch = D.ch_ptr[k + 1] - D.ch_ptr[k], nmr = D.mr_ptr[k + 1] - D.mr_ptr[k];
      if (nch > 0)
        hipLaunchKernelGGL(deriv_lagrangian_grad, dim3(deriv_grid(64 * nch)), dim3(DERIV_THREADS), 0, st,
                           D.ch_row.p + D.ch_ptr[k], D.ch_p0.p + D.ch_ptr[k], D.ch_p1.p + D.ch_ptr[k], nch, D.csc_ent.p,
                           D.g_row.p, D.GP.p, D.GM.p, lam, D.gnP.p, D.gnM.p, D.jg_of_col.p, sigma, D.dL.p, D.part.p + D.ch_ptr[k]);
      if (nmr > 0)   // (chunk indices of mr_c0 / mr_c1 are global: part is read from its start)
        hipLaunchKernelGGL(deriv_lagrangian_sum, dim3(deriv_grid(nmr)), dim3(DERIV_THREADS), 0, st, D.mr_row.p + D.mr_ptr[k],
                           D.mr_c0.p + D.mr_ptr[k], D.mr_c1.p + D.mr_ptr[k], nmr, D.part.p, D.gnP.p, D.gnM.p, D.jg_of_col.p,
                           sigma, D.dL.p);
      DerivColour L;
      L.gl_ent = D.gl_ent.p + P.gl_ptr[k];
      L.n_gl = P.gl_ptr[k + 1] - P.gl_ptr[k];
      L.seg0 = P.seg_ptr[k];
      L.seg_row = D.seg_row.p + L.seg0;
      L.seg_eptr = D.seg_eptr.p + L.seg0;
      L.n_seg = P.seg_ptr[k + 1] - L.seg0;
      L.hl_ent = D.hl_ent.p + P.hl_ptr[k];
      L.hl_lrow = D.hl_lrow.p + P.hl_ptr[k];
      L.hl_scol = D.hl_scol.p + P.hl_ptr[k];
      L.n_hl = P.hl_ptr[k + 1] - P.hl_ptr[k];
      L.jl_ent = D.jl_ent.p + P.jl_ptr[k];
      L.n_jl = P.jl_ptr[k + 1] - P.jl_ptr[k];
      const int nb_loc = (int)deriv_grid(L.n_gl + L.n_hl + L.n_jl);
      const int nb = nb_loc + (int)deriv_grid(64 * L.n_seg);
      if (nb > 0)
        hipLaunchKernelGGL(deriv_compare, dim3(nb), dim3(DERIV_THREADS), 0, st, L, nb_loc, D.g_row.p, D.g_col.p,
                           D.seg_ent.p, D.jcol.p, D.step2.p, D.cP.p, D.cM.p, D.f3.p, D.dL.p, Gan, Han, Jan, errG, errS, errH,
                           errJ, D.fdG.p, D.fdH.p, D.fdJ.p, D.segA.p, D.segF.p);
    }
    HIP_OK(hipGetLastError());
    deriv_handover(h, D, 1, st);
    DerivView V{D.g_row.p, D.g_col.p, D.h_row.p, D.h_col.p, D.seg_row.p, D.seg_colour.p, D.jcol.p, Gan, Han, Jan,
                D.fdG.p, D.fdH.p, D.fdJ.p, D.segA.p, D.segF.p, D.err.p, D.nG, D.nS, D.nH, D.nJ};
    const int nb = D.nb_red;
    const int64_t chunk = std::max<int64_t>(1, (D.T + nb - 1) / nb);
    DerivOut* dout = reinterpret_cast<DerivOut*>(D.out.p);
    HIP_OK(hipMemsetAsync(D.out.p, 0, sizeof(DerivOut), st));
    hipLaunchKernelGGL(deriv_reduce_blocks, dim3(nb), dim3(DERIV_THREADS), 0, st, V, chunk, tol, D.r_max.p, D.r_idx.p, D.r_cnt.p);
    hipLaunchKernelGGL(deriv_reduce_final, dim3(1), dim3(64), 0, st, V, nb, D.r_max.p, D.r_idx.p, D.r_cnt.p, D.r_pfx.p, dout);
    if (max_report > 0)
      hipLaunchKernelGGL(deriv_compact, dim3(nb), dim3(DERIV_THREADS), 0, st, V, chunk, tol, max_report, D.r_pfx.p, dout);
    HIP_OK(hipGetLastError());
    if (o.d_jac_fd && D.nG) HIP_OK(hipMemcpyAsync(o.d_jac_fd, D.fdG.p, D.nG * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (o.d_hess_fd && D.nH) HIP_OK(hipMemcpyAsync(o.d_hess_fd, D.fdH.p, D.nH * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (o.d_jgrad_fd && D.nJ) HIP_OK(hipMemcpyAsync(o.d_jgrad_fd, D.fdJ.p, D.nJ * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_OK(hipMemcpyAsync(D.h_out.p, D.out.p, sizeof(DerivOut), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    check_timeout(h);
    const DerivOut& r = *reinterpret_cast<const DerivOut*>(D.h_out.p);
    std::memset(report, 0, sizeof(*report));
    report->tol = tol;
    report->n_colours = P.n_colours;
    report->n_evaluations = 1 + 2 * P.n_colours;
    auto fix = [](double v) { return v < 0 ? 0.0 : v; };   // (no entry of a kind: -inf; sum terms: -1)
    report->max_err[0] = fix(std::max(r.max_err[0], r.max_err[1]));
    report->max_err[1] = fix(r.max_err[2]);
    report->max_err[2] = fix(r.max_err[3]);
    for (int j = 0; j < 3; ++j) report->worst[j] = r.worst[j];
    report->n_fail[0] = r.n_fail[0] + r.n_fail[1];
    report->n_fail[1] = r.n_fail[2];
    report->n_fail[2] = r.n_fail[3];
    const int64_t total = r.n_fail[0] + r.n_fail[1] + r.n_fail[2] + r.n_fail[3];
    report->ok = total == 0;
    report->n_report = (int32_t)std::min<int64_t>(total, max_report);
    for (int i = 0; i < report->n_report; ++i) report->fail[i] = r.fail[i];
    report->n_jac_located = P.n_g_located;
    report->n_jac_sum_terms = P.n_g_sum;
    report->n_sums = P.n_seg;
    report->n_hess_located = P.n_h_located;
    report->n_jgrad_located = P.n_j_located;
  });
}

}  // extern "C"
