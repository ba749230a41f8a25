// Kernels that read a finished NLP point: the dense output (pycollo/solution/solution_abc.py:60-142,
// casadi_solution.py:15-86), the costates, the propagation and the ph mesh-error estimate.
// Included by the generated code object after pc_kernels.hpp (S<M>, static_for, M::eval_f).
//
// Per section k (n nodes, section variable c in [-1, 1]):
//   ydot(c) = sum_m a_m P_m(c),  a = tabD_n . f(nodes)      (Lobatto: degree n-1; Radau: degree n-2, last row of tabD zero)
//   u(c)    = sum_m e_m P_m(c),  e = tabU_n . u(nodes)      (degree n-1 through all n nodes)
//   y(c)    = y(tau_k) + stretch (h_k / 2) sum_m a_m int_{-1}^{c} P_m,   int P_m = (P_{m+1} - P_{m-1}) / (2m + 1)
// Both sums are evaluated by Clenshaw's recurrence.
#ifndef PC_SOLUTION_HPP
#define PC_SOLUTION_HPP

#include "pc_step_control.hpp"

namespace pc {

// ---- what the kernels share: unscaling through the phase view, the lanes of a tile, the table contraction ----
template <class M>
__device__ __forceinline__ void sol_times(const PcPhaseView& V, double& t0, double& tF) {
  using St = S<M>;
  const double* sc = V.scal;
  t0 = V.t_fixed[0];
  tF = V.t_fixed[1];
  const int64_t t_off = V.x_off + (int64_t)St::NZ * V.N + St::NQ;
  int j = 0;
  if constexpr (M::T0_FREE) { t0 = sc[St::O_VT + j] * V.x[t_off + j] + sc[St::O_RT + j]; ++j; }
  if constexpr (M::TF_FREE) { tF = sc[St::O_VT + j] * V.x[t_off + j] + sc[St::O_RT + j]; }
}

// the q / t / s arguments of f, unscaled, into v[NZ ..]
template <class M>
__device__ __forceinline__ void sol_params(const PcPhaseView& V, double* v) {
  using St = S<M>;
  const double* sc = V.scal;
  static_for<0, St::NS>([&](auto l_) {
    constexpr int l = decltype(l_)::value;
    constexpr int kind = M::wk(l), idx = M::wi(l);   // static parameter, or this phase's q / free t
    const int64_t col = kind == 0 ? V.s_off + idx : V.x_off + (int64_t)St::NZ * V.N + (kind == 1 ? idx : St::NQ + idx);
    v[St::NZ + l] = sc[St::O_VS + l] * V.x[col] + sc[St::O_RS + l];
  });
}

// the states and controls of a node, unscaled, into v[0 .. NZ)
template <class M>
__device__ __forceinline__ void sol_node(const PcPhaseView& V, int node, double* v) {
  using St = S<M>;
  const double* sc = V.scal;
  static_for<0, St::NZ>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    v[b] = sc[St::O_VZ + b] * V.x[V.x_off + (int64_t)b * V.N + node] + sc[St::O_RZ + b];
  });
}

// The tile of a workgroup is the run of sections k0 .. k1 (tile_k0[blockIdx.x], tile_k0[blockIdx.x + 1]); section k owns
// the n_k + extra consecutive lanes from lane0[k] (the host's pcs::section_tiles).  Which section a lane belongs to goes
// through s_sec [blockDim].  Returned: the lane's section k, its first node sk, its nodes n, its first lane l0 and the
// lane's place j in it; a lane beyond the tile's last section is not active.  Two barriers: what the kernel staged
// before the call is visible after it.
struct SolLane {
  int k, sk, n, l0, j;
  bool active;
};
__device__ __forceinline__ SolLane sol_lane_map(const PcPhaseView& V, int k0, int k1, const int32_t* lane0, int extra,
                                                int* s_sec) {
  const int tid = threadIdx.x, TB = blockDim.x;
  s_sec[tid] = -1;
  __syncthreads();
  for (int k = k0 + tid; k < k1; k += TB) {
    const int lanes = V.sec_s[k + 1] - V.sec_s[k] + 1 + extra, l0 = lane0[k];
    for (int j = 0; j < lanes; ++j)
      if (l0 + j < TB) s_sec[l0 + j] = k;
  }
  __syncthreads();
  SolLane L;
  L.k = s_sec[tid];
  L.active = L.k >= 0;
  const int kc = L.active ? L.k : k0;   // (a lane without a section reads the tile's first: its values are not used)
  L.sk = V.sec_s[kc];
  L.n = V.sec_s[kc + 1] - L.sk + 1;
  L.l0 = lane0[kc];
  L.j = tid - L.l0;
  return L;
}

// a node shared by two sections is written by the section it opens (the last node: by the last section)
__device__ __forceinline__ bool sol_owner(const SolLane& L, int K) { return L.j < L.n - 1 || L.k == K - 1; }

// row . vals over n entries, ascending: a lane's row of a section table against the section's staged values
__device__ __forceinline__ double sol_row_dot(const double* row, const double* vals, int n) {
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc += row[i] * vals[i];
  return acc;
}

// ---------------------------------------------------------------------------------------------
// pc_sol_fit_p<i>: one workgroup per run of sections, section k owns n_k consecutive lanes = its nodes.
//   1. unscale the node, f at the node (casadi_solution.py:71), node values out
//   2. lane j of a section contracts row j of the section's tables with the section's node values: coefficient j
// Every sum runs over the section's nodes in order; nothing is accumulated across lanes.
// ---------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void sol_fit(const PcSolFitArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const PcPhaseView& V = A.v;
  double* s_D = smem;
  double* s_U = s_D + A.tab_total;
  double* s_f = s_U + A.tab_total;                  // [NY][TB]
  double* s_u = s_f + (NY > 0 ? NY : 1) * TB;       // [NU][TB]
  int* s_sec = reinterpret_cast<int*>(s_u + (NU > 0 ? NU : 1) * TB);   // [TB] section of every lane
  for (int i = tid; i < A.tab_total; i += TB) {
    s_D[i] = A.tabD[i];
    s_U[i] = A.tabU[i];
  }
  const SolLane L = sol_lane_map(V, A.tile_k0[blockIdx.x], A.tile_k0[blockIdx.x + 1], A.lane0, 0, s_sec);
  double t0, tF;
  sol_times<M>(V, t0, tF);
  if (L.active) {
    const int node = L.sk + L.j;
    double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1];
    sol_params<M>(V, v);
    sol_node<M>(V, node, v);
    M::eval_f(v, F);
    const bool owner = sol_owner(L, V.K);
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      s_f[a * TB + tid] = F[a];
      if (owner) {
        A.node_y[(int64_t)a * V.N + node] = v[a];
        A.node_f[(int64_t)a * V.N + node] = F[a];
      }
    });
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      s_u[b * TB + tid] = v[NY + b];
      if (owner) A.node_u[(int64_t)b * V.N + node] = v[NY + b];
    });
    if (owner) A.node_t[node] = A.tau[node] * (0.5 * (tF - t0)) + 0.5 * (t0 + tF);   // casadi_solution.py:80-83
  }
  __syncthreads();
  if (L.active) {
    const int n = L.n, row = A.offC[n] + L.j * n;
    const int64_t slot = (int64_t)L.sk + L.k + L.j;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      A.coef_dy[(int64_t)a * A.NC + slot] = sol_row_dot(s_D + row, s_f + a * TB + L.l0, n);
    });
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      A.coef_u[(int64_t)b * A.NC + slot] = sol_row_dot(s_U + row, s_u + b * TB + L.l0, n);
    });
  }
}

// ---------------------------------------------------------------------------------------------
// pc_sol_sample_p<i>: one lane per query.  The lane maps its time to tau, finds its section by bisection over the
// K + 1 section boundaries (a boundary belongs to the section on its right, tau = +1 to the last section) and reads
// the section's coefficients from high to low degree -- one pass feeds the Clenshaw recurrences of ydot and of its
// integral.  Outputs are variable-major [var][Q]: neighbouring lanes write neighbouring doubles.
// ---------------------------------------------------------------------------------------------
// where a query lands
struct SolSpot {
  int k, sk, n;        // section, its first node, its nodes
  double c, w;         // section variable in [-1, 1], section width in tau
  double stretch;
  int64_t off;         // the section's first coefficient
};

// false: the query is outside the phase (or NaN) and is not extrapolated -- every output of the lane is NaN
template <class M>
__device__ __forceinline__ bool sol_locate(const PcSolSampleArgs& A, int64_t i, SolSpot& s) {
  double t0, tF;
  sol_times<M>(A.v, t0, tF);
  const double stretch = 0.5 * (tF - t0), shift = 0.5 * (t0 + tF);
  const double q = A.t[i];
  double tau;
  bool inside;
  if (A.flags & PC_SOL_TAU) {
    tau = q;
    inside = q >= -1.0 && q <= 1.0;
  } else {
    // a time within a few ulp of the phase's ends is the end (node_time's own last entry, tau stretch + shift, may
    // round past tF)
    tau = (q - shift) / stretch;
    inside = fabs(tau) <= 1.0 + PC_SOL_END_SLACK;
    if (inside) tau = fmin(1.0, fmax(-1.0, tau));
  }
  if (!(inside || ((A.flags & PC_SOL_EXTRAPOLATE) && tau == tau))) return false;
  // the last boundary <= tau, kept inside [0, K - 1]
  int lo = 0, hi = A.v.K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.c.sec_tau[mid] <= tau) lo = mid; else hi = mid;
  }
  s.k = lo;
  s.sk = A.v.sec_s[lo];
  s.n = A.v.sec_s[lo + 1] - s.sk + 1;
  const double ta = A.c.sec_tau[lo];
  s.w = A.c.sec_tau[lo + 1] - ta;
  s.c = 2.0 * (tau - ta) / s.w - 1.0;
  s.stretch = stretch;
  s.off = (int64_t)s.sk + lo;
  return true;
}

// state a at the spot (the integrated form) and, in d, its derivative
__device__ __forceinline__ double sol_state(const PcSolSampleArgs& A, const SolSpot& s, int a, double& d) {
  const double* cf = A.c.coef_dy + (int64_t)a * A.c.NC + s.off;
  const double c = s.c;
  // j = n .. 0: b_j = a_(j-1) / (2j - 1) - a_(j+1) / (2j + 3) are the coefficients of int_{-1}^{c} ydot
  // (b_0 = a_0 - a_1 / 3); ydot's own Clenshaw step j uses a_j
  double a_hi = 0.0, a_mid = 0.0;
  double y1 = 0.0, y2 = 0.0, d1 = 0.0, d2 = 0.0;
  for (int j = s.n; j >= 0; --j) {
    const double a_lo = j >= 1 ? cf[j - 1] : 0.0;
    const double bj = (j >= 1 ? a_lo / (double)(2 * j - 1) : a_mid) - a_hi / (double)(2 * j + 3);
    const double al = (double)(2 * j + 1) / (double)(j + 1) * c, be = (double)(j + 1) / (double)(j + 2);
    const double yn = bj + (al * y1 - be * y2);
    y2 = y1;
    y1 = yn;
    const double dn = a_mid + (al * d1 - be * d2);
    d2 = d1;
    d1 = dn;
    a_hi = a_mid;
    a_mid = a_lo;
  }
  d = d1;
  return A.c.node_y[(int64_t)a * A.v.N + s.sk] + s.stretch * ((0.5 * s.w) * y1);
}

// sum_j cf[j] P_j(c), j < n (Clenshaw): the controls, the costates
__device__ __forceinline__ double sol_legendre(const double* cf, int n, double c) {
  double u1 = 0.0, u2 = 0.0;
  for (int j = n - 1; j >= 0; --j) {
    const double al = (double)(2 * j + 1) / (double)(j + 1) * c, be = (double)(j + 1) / (double)(j + 2);
    const double un = cf[j] + (al * u1 - be * u2);
    u2 = u1;
    u1 = un;
  }
  return u1;
}

template <class M>
__device__ __forceinline__ void sol_sample(const PcSolSampleArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.Q) return;
  SolSpot s;
  if (!sol_locate<M>(A, i, s)) {
    const double nan = __builtin_nan("");
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      if (A.out_y) A.out_y[(int64_t)a * A.Q + i] = nan;
      if (A.out_dy) A.out_dy[(int64_t)a * A.Q + i] = nan;
      if (A.out_f) A.out_f[(int64_t)a * A.Q + i] = nan;
    });
    static_for<0, NU>([&](auto b_) {
      if (A.out_u) A.out_u[(int64_t) decltype(b_)::value * A.Q + i] = nan;
    });
    return;
  }
  double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1];
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    double d;
    const double y = sol_state(A, s, a, d);
    v[a] = y;
    if (A.out_y) A.out_y[(int64_t)a * A.Q + i] = y;
    if (A.out_dy) A.out_dy[(int64_t)a * A.Q + i] = d;
  });
  static_for<0, NU>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    const double u = sol_legendre(A.c.coef_u + (int64_t)b * A.c.NC + s.off, s.n, s.c);
    v[NY + b] = u;
    if (A.out_u) A.out_u[(int64_t)b * A.Q + i] = u;
  });
  if (A.out_f) {
    sol_params<M>(A.v, v);
    M::eval_f(v, F);
    static_for<0, NY>([&](auto a_) { A.out_f[(int64_t) decltype(a_)::value * A.Q + i] = F[decltype(a_)::value]; });
  }
}

// ---------------------------------------------------------------------------------------------
// Costates and the Hamiltonian.  Lam = W lam~ / w are the multipliers of the unscaled rows for the
// unscaled objective.  Per node j, over the one or two sections k that contain it (lower section first, rows ascending,
// one division at the end):
//   omega_j = sum_k h_k A_k[n_k - 2][pos_k(j)]
//   p_a(j)  = ( sum_k h_k sum_r Lam_a[s_k + r] A_k[r][pos_k(j)] ) / omega_j;   omega_j == 0 (the Radau phase-final node,
//             an exact zero of the table): p_a = Lam_a[N - 2], H = NaN
//   nu_m    = -Lam_q[m];   H(j) = sum_a p_a f_a + sum_m nu_m g_m at the node's (y, u, q, t, s)
//
// pc_sol_costate_p<i>: the tiles and lanes of pc_sol_fit.  The workgroup stages the A and C_u tables and the rows of
// Lam its nodes need (those of its sections and of the two neighbour sections its end lanes reach into); both lanes of
// a shared node run the same sums on the same operands, the section the node opens writes it.  Then lane j of a
// section contracts row j of C_u with the section's costates: coefficient j.
// ---------------------------------------------------------------------------------------------
#define PC_SOL_LAM_ROWS(TB) ((TB) + 2 * PC_MAX_ORDER)   // staged rows of one state: <= TB - 1 own + 2 x 19 neighbour rows

template <class M>
__device__ __forceinline__ void sol_costate(const PcSolCostateArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NQ = St::NQ;
  constexpr int NY1 = NY > 0 ? NY : 1, NQ1 = NQ > 0 ? NQ : 1;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, TB = blockDim.x, LW = PC_SOL_LAM_ROWS(TB);
  const PcPhaseView& V = A.v;
  double* s_U = smem;
  double* s_A = s_U + A.tab_total;
  double* s_lam = s_A + A.a_total;                   // [NY][LW] Lam of rows r_lo ..
  double* s_p = s_lam + NY1 * LW;                    // [NY][TB]
  int* s_sec = reinterpret_cast<int*>(s_p + NY1 * TB);   // [TB] section of every lane
  const int k0 = A.tile_k0[blockIdx.x], k1 = A.tile_k0[blockIdx.x + 1];
  const double* sc = V.scal;
  for (int i = tid; i < A.tab_total; i += TB) s_U[i] = A.tabU[i];
  for (int i = tid; i < A.a_total; i += TB) s_A[i] = A.tabA[i];
  // rows of the tile's sections and of the sections before and after it
  const int r_lo = V.sec_s[k0 > 0 ? k0 - 1 : 0], r_hi = V.sec_s[k1 < V.K ? k1 + 1 : V.K];
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    const double* la = A.lam + A.c_off + (int64_t)a * (V.N - 1) + r_lo;
    for (int i = tid; i < r_hi - r_lo && i < LW; i += TB) s_lam[a * LW + i] = sc[St::O_WD + a] * la[i] / A.wJ;
  });
  const SolLane L = sol_lane_map(V, k0, k1, A.lane0, 0, s_sec);
  if (L.active) {
    const int k = L.k, n = L.n, j = L.j, node = L.sk + j;
    // the sections of the node: [ka, kb], positions pa (in ka) and 0 (in kb > ka)
    int ka = k, pa = j, kb = k;
    if (j == 0 && k > 0) { ka = k - 1; pa = L.sk - V.sec_s[k - 1]; }
    if (j == n - 1 && k < V.K - 1) kb = k + 1;
    double omega = 0.0, num[NY1];
    static_for<0, NY>([&](auto a_) { num[decltype(a_)::value] = 0.0; });
    for (int kk = ka; kk <= kb; ++kk) {
      const int s0 = V.sec_s[kk], nn = V.sec_s[kk + 1] - s0 + 1, pos = kk == ka ? pa : 0;
      const double h = A.sec_tau[kk + 1] - A.sec_tau[kk];
      const double* At = s_A + A.offA[nn] + pos;
      omega += h * At[(nn - 2) * nn];
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        const double* la = s_lam + a * LW + (s0 - r_lo);
        double acc = 0.0;
        for (int r = 0; r < nn - 1; ++r) acc += la[r] * At[r * nn];
        num[a] += h * acc;
      });
    }
    double v[St::NV > 0 ? St::NV : 1], F[NY1], G[NQ1], p[NY1];
    sol_params<M>(V, v);
    sol_node<M>(V, node, v);
    M::eval_fg(v, F, G);
    const bool weighted = !(node == V.N - 1 && omega == 0.0);   // (the tile of node N - 1 stages row N - 2)
    double H = 0.0;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      p[a] = weighted ? num[a] / omega : s_lam[a * LW + (V.N - 2 - r_lo)];
      H += p[a] * F[a];
    });
    static_for<0, NQ>([&](auto m_) {
      constexpr int m = decltype(m_)::value;
      const double nu = -(sc[St::O_WI + m] * A.lam[A.c_int_off + m] / A.wJ);
      H += nu * G[m];
      if (blockIdx.x == 0 && tid == 0) A.nu[m] = nu;
    });
    const bool owner = sol_owner(L, V.K);
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      s_p[a * TB + tid] = p[a];
      if (owner) A.node_p[(int64_t)a * V.N + node] = p[a];
    });
    if (owner) A.node_H[node] = weighted ? H : __builtin_nan("");
  }
  __syncthreads();
  if (L.active) {
    const int n = L.n;
    const double* Ur = s_U + A.offC[n] + L.j * n;
    const int64_t slot = (int64_t)L.sk + L.k + L.j;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      A.coef_p[(int64_t)a * A.NC + slot] = sol_row_dot(Ur, s_p + a * TB + L.l0, n);
    });
  }
}

// ---------------------------------------------------------------------------------------------
// pc_sol_sample_costate_p<i>: one lane per query, located as in pc_sol_sample.  p(t) is the section's interpolant of
// the node costates; H(t) = sum_a p_a(t) f_a + sum_m nu_m g_m with f, g at the interpolated (y(t), u(t)).
// ---------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void sol_sample_costate(const PcSolCostateSampleArgs& B) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU, NQ = St::NQ;
  const PcSolSampleArgs& A = B.s;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.Q) return;
  SolSpot s;
  if (!sol_locate<M>(A, i, s)) {
    const double nan = __builtin_nan("");
    static_for<0, NY>([&](auto a_) { B.out_p[(int64_t) decltype(a_)::value * A.Q + i] = nan; });
    B.out_H[i] = nan;
    return;
  }
  double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1], G[NQ > 0 ? NQ : 1];
  static_for<0, NY>([&](auto a_) {
    double d;
    v[decltype(a_)::value] = sol_state(A, s, decltype(a_)::value, d);
  });
  static_for<0, NU>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    v[NY + b] = sol_legendre(A.c.coef_u + (int64_t)b * A.c.NC + s.off, s.n, s.c);
  });
  sol_params<M>(A.v, v);
  M::eval_fg(v, F, G);
  double H = 0.0;
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    const double p = sol_legendre(B.coef_p + (int64_t)a * A.c.NC + s.off, s.n, s.c);
    B.out_p[(int64_t)a * A.Q + i] = p;
    H += p * F[a];
  });
  static_for<0, NQ>([&](auto m_) { H += B.nu[decltype(m_)::value] * G[decltype(m_)::value]; });
  B.out_H[i] = H;
}

// ---------------------------------------------------------------------------------------------
// Path and bound multipliers, the gradients of the augmented Hamiltonian.  With omega_j the node weight of
// the costate kernel (same sections, same order of the sum) and den = stretch omega_j:
//   mu_i(j)   = (Wp_i lam~[c_path_off + i N + j] / w) / den
//   zeta_b(j) = (z~[x_off + b N + j] / (w V_b)) / den;  a state's entry at nodes 0 and N - 1 is the endpoint bound's: zeta
//               is 0 there and the value without den goes to end_z [NY][2]
//   H_z(j)    = sum over the tape's first partials, table order, of mult[jr] Jv on column jc < NZ, mult = [p | mu | rho nu],
//               rho = int_scale: the integral rows' node weight over omega_j (1 under Lobatto, 2 under Radau)
// The Radau phase-final node (omega = 0): mu, zeta_u and H_z are NaN, and 0 is staged for the contraction below.
//
// pc_sol_multipliers_p<i>: the tiles and lanes of pc_sol_fit.  Lane j of a section then contracts row j of the C_u table
// (the phase's last section: of the ydot table, whose Radau form leaves the final node out) with the section's staged
// node values: coefficient j of mu and zeta.  Both lanes of a shared node compute the same values; the section the node
// opens writes them.
// ---------------------------------------------------------------------------------------------
// d/dc of sum_j cf[j] P_j(c), j < n: Clenshaw's recurrence differentiated (u_j' = (2j+1)/(j+1) u_(j+1) + al u_(j+1)' - be u_(j+2)')
__device__ __forceinline__ double sol_legendre_d(const double* cf, int n, double c) {
  double u1 = 0.0, u2 = 0.0, d1 = 0.0, d2 = 0.0;
  for (int j = n - 1; j >= 0; --j) {
    const double g = (double)(2 * j + 1) / (double)(j + 1), al = g * c, be = (double)(j + 1) / (double)(j + 2);
    const double dn = g * u1 + (al * d1 - be * d2);
    const double un = cf[j] + (al * u1 - be * u2);
    d2 = d1;
    d1 = dn;
    u2 = u1;
    u1 = un;
  }
  return d1;
}

// Hz [NZ]: the node-variable columns of sum_r mult[r] d(f | p | g)_r / dz at v, from one eval_fj
template <class M>
__device__ __forceinline__ void sol_hgrad(const double* v, const double* mult, double* Hz) {
  using St = S<M>;
  constexpr int NZ = St::NZ, NJ = St::NJ, NFN = St::NFN;
  double F[NFN > 0 ? NFN : 1], Jv[NJ > 0 ? NJ : 1];
  M::eval_fj(v, F, Jv);
  static_for<0, NZ>([&](auto b_) { Hz[decltype(b_)::value] = 0.0; });
  static_for<0, NJ>([&](auto e_) {
    constexpr int e = decltype(e_)::value;
    if constexpr (M::jc(e) < NZ) Hz[M::jc(e)] += mult[M::jr(e)] * Jv[e];
  });
}

template <class M>
__device__ __forceinline__ void sol_multipliers(const PcSolMultiplierArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NZ = St::NZ, NP = St::NP, NQ = St::NQ, NFN = St::NFN;
  constexpr int NM = NP + NZ, NM1 = NM > 0 ? NM : 1;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const PcPhaseView& V = A.v;
  double* s_U = smem;
  double* s_D = s_U + A.tab_total;
  double* s_W = s_D + A.tab_total;
  double* s_val = s_W + A.w_total;                      // [NP + NZ][TB] mu, then zeta
  int* s_sec = reinterpret_cast<int*>(s_val + NM1 * TB);   // [TB] section of every lane
  const double* sc = V.scal;
  for (int i = tid; i < A.tab_total; i += TB) {
    s_U[i] = A.tabU[i];
    s_D[i] = A.tabD[i];
  }
  for (int i = tid; i < A.w_total; i += TB) s_W[i] = A.tabW[i];
  const SolLane L = sol_lane_map(V, A.tile_k0[blockIdx.x], A.tile_k0[blockIdx.x + 1], A.lane0, 0, s_sec);
  const bool has_z = A.z != nullptr;
  double t0, tF;
  sol_times<M>(V, t0, tF);
  const double stretch = 0.5 * (tF - t0);
  if (L.active) {
    const int k = L.k, n = L.n, j = L.j, node = L.sk + j, N = V.N;
    // the node weight, summed as pc_sol_costate sums it
    int ka = k, pa = j, kb = k;
    if (j == 0 && k > 0) { ka = k - 1; pa = L.sk - V.sec_s[k - 1]; }
    if (j == n - 1 && k < V.K - 1) kb = k + 1;
    double omega = 0.0;
    for (int kk = ka; kk <= kb; ++kk) {
      const int s0 = V.sec_s[kk], nn = V.sec_s[kk + 1] - s0 + 1, pos = kk == ka ? pa : 0;
      omega += (A.sec_tau[kk + 1] - A.sec_tau[kk]) * s_W[A.offW[nn] + pos];
    }
    const bool weighted = !(node == N - 1 && omega == 0.0);
    const bool owner = sol_owner(L, V.K);
    const double den = stretch * omega, nan = __builtin_nan("");
    double mult[NFN > 0 ? NFN : 1];
    static_for<0, NY>([&](auto a_) { mult[decltype(a_)::value] = A.node_p[(int64_t) decltype(a_)::value * N + node]; });
    static_for<0, NP>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      const double mu = weighted ? (sc[St::O_WP + i] * A.lam[A.c_path_off + (int64_t)i * N + node] / A.wJ) / den : nan;
      mult[NY + i] = mu;
      s_val[i * TB + tid] = weighted ? mu : 0.0;
      if (owner) A.node_mu[(int64_t)i * N + node] = mu;
    });
    static_for<0, NQ>([&](auto m_) { mult[NY + NP + decltype(m_)::value] = A.int_scale * A.nu[decltype(m_)::value]; });
    if (has_z) {
      static_for<0, NZ>([&](auto b_) {
        constexpr int b = decltype(b_)::value;
        const double zs = A.z[V.x_off + (int64_t)b * N + node] / (A.wJ * sc[St::O_VZ + b]);
        const bool end = b < NY && (node == 0 || node == N - 1);
        const double zeta = end ? 0.0 : (weighted ? zs / den : nan);
        s_val[(NP + b) * TB + tid] = weighted ? zeta : 0.0;
        if (owner) {
          A.node_zeta[(int64_t)b * N + node] = zeta;
          if (end) A.end_z[2 * b + (node == 0 ? 0 : 1)] = zs;
        }
      });
    }
    double v[St::NV > 0 ? St::NV : 1], Hz[NZ > 0 ? NZ : 1];
    sol_params<M>(V, v);
    sol_node<M>(V, node, v);
    sol_hgrad<M>(v, mult, Hz);
    if (owner) static_for<0, NZ>([&](auto b_) {
      A.node_Hz[(int64_t) decltype(b_)::value * N + node] = weighted ? Hz[decltype(b_)::value] : nan;
    });
  }
  __syncthreads();
  if (L.active) {
    const int n = L.n;
    const double* Tr = (L.k == V.K - 1 ? s_D : s_U) + A.offC[n] + L.j * n;
    const int64_t slot = (int64_t)L.sk + L.k + L.j;
    static_for<0, NP>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      A.coef_mu[(int64_t)i * A.NC + slot] = sol_row_dot(Tr, s_val + i * TB + L.l0, n);
    });
    if (has_z) static_for<0, NZ>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      A.coef_zeta[(int64_t)b * A.NC + slot] = sol_row_dot(Tr, s_val + (NP + b) * TB + L.l0, n);
    });
  }
}

// ---------------------------------------------------------------------------------------------
// pc_sol_sample_optimality_p<i>: one lane per query, located as in pc_sol_sample.  mu(t), zeta(t) and p(t) are the
// sections' interpolants, dp/dt = 2 / (w_k stretch) d/dc of p's; H_y(t), H_u(t) from the tape at the interpolated
// (y(t), u(t)) with p(t), mu(t) and rho nu.  Outputs variable-major [var][Q].
// ---------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void sol_sample_optimality(const PcSolOptimalitySampleArgs& B) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU, NZ = St::NZ, NP = St::NP, NQ = St::NQ, NFN = St::NFN;
  const PcSolSampleArgs& A = B.s;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.Q) return;
  const bool has_z = B.coef_zeta != nullptr;
  SolSpot s;
  if (!sol_locate<M>(A, i, s)) {
    const double nan = __builtin_nan("");
    static_for<0, NY>([&](auto a_) {
      B.out_Hy[(int64_t) decltype(a_)::value * A.Q + i] = nan;
      B.out_dp[(int64_t) decltype(a_)::value * A.Q + i] = nan;
    });
    static_for<0, NU>([&](auto b_) { B.out_Hu[(int64_t) decltype(b_)::value * A.Q + i] = nan; });
    static_for<0, NP>([&](auto i_) { B.out_mu[(int64_t) decltype(i_)::value * A.Q + i] = nan; });
    if (has_z) static_for<0, NZ>([&](auto b_) { B.out_zeta[(int64_t) decltype(b_)::value * A.Q + i] = nan; });
    return;
  }
  double v[St::NV > 0 ? St::NV : 1], mult[NFN > 0 ? NFN : 1], Hz[NZ > 0 ? NZ : 1];
  static_for<0, NY>([&](auto a_) {
    double d;
    v[decltype(a_)::value] = sol_state(A, s, decltype(a_)::value, d);
  });
  static_for<0, NU>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    v[NY + b] = sol_legendre(A.c.coef_u + (int64_t)b * A.c.NC + s.off, s.n, s.c);
  });
  sol_params<M>(A.v, v);
  const double dcdt = 2.0 / (s.w * s.stretch);
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    const double* cf = B.coef_p + (int64_t)a * A.c.NC + s.off;
    mult[a] = sol_legendre(cf, s.n, s.c);
    B.out_dp[(int64_t)a * A.Q + i] = dcdt * sol_legendre_d(cf, s.n, s.c);
  });
  static_for<0, NP>([&](auto i_) {
    constexpr int ii = decltype(i_)::value;
    const double mu = sol_legendre(B.coef_mu + (int64_t)ii * A.c.NC + s.off, s.n, s.c);
    mult[NY + ii] = mu;
    B.out_mu[(int64_t)ii * A.Q + i] = mu;
  });
  static_for<0, NQ>([&](auto m_) { mult[NY + NP + decltype(m_)::value] = B.int_scale * B.nu[decltype(m_)::value]; });
  sol_hgrad<M>(v, mult, Hz);
  static_for<0, NY>([&](auto a_) { B.out_Hy[(int64_t) decltype(a_)::value * A.Q + i] = Hz[decltype(a_)::value]; });
  static_for<0, NU>([&](auto b_) { B.out_Hu[(int64_t) decltype(b_)::value * A.Q + i] = Hz[NY + decltype(b_)::value]; });
  if (has_z) static_for<0, NZ>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    B.out_zeta[(int64_t)b * A.Q + i] = sol_legendre(B.coef_zeta + (int64_t)b * A.c.NC + s.off, s.n, s.c);
  });
}

// ---------------------------------------------------------------------------------------------
// Propagation: dy/dc = stretch (w_k / 2) f(y, u(c), q, t0, tF, s) integrated by Dormand-Prince 5(4) across
// node intervals, u(c) the section's control interpolant (sol_legendre on coef_u, what pc_sol_sample returns).
//
// pc_sol_propagate_p<i>: one lane per segment [seg_node[i], seg_node[i+1]].  The lane starts from the NLP's node value,
// walks its node intervals in order (its first section is seg_sec[i]; it moves to the next section when it reaches that
// section's first node) and writes, at the node every interval ends at, the arriving state and the interval's step
// counts: its own columns only.  No step straddles a node.  No LDS, no atomics; the seven stage vectors live in
// registers (7 NY doubles), which is why a workgroup is one wave: many small workgroups spread over the CUs.
// The walk is prop_walk, for this kernel and pc_sol_propagate_dense alike; each of the two is a method handed to it
// (pc_sol_propagate_stiff still carries its own copy, see there).  The steps of an interval are placed by StepControl
// (pc_step_control.hpp):
//   fixed (substeps = m >= 1): step i of an interval starts at c_j + i h, h = (c_{j+1} - c_j) / m, and has width h (the
//     last one: c_{j+1} - its start).  Six stages: the seventh only feeds the error estimate.
//   adaptive (substeps = 0): h starts as the whole interval; err = max_a |e_a| / (atol_a + rtol max(|y_a|, |ynew_a|));
//     accepted when err <= 1; factor = clamp(0.9 err^(-1/5), 0.2, 5) (5 at err = 0, at most 1 right after a rejection,
//     0.2 when err is not finite, which rejects); next h = min(h factor, rest of the interval).  An interval that has
//     not arrived after max_steps steps (accepted + rejected) ends the lane: seg_status = its first node, NaN from
//     there to the segment's end.  Every loop is bounded: intervals by N, steps by max_steps or substeps (<= 2^20).
// ---------------------------------------------------------------------------------------------
// Dormand-Prince tableau: rows 1 .. 5 of a, row 6 = b (the fifth-order weights, also stage 7's row), e = b - b^
__host__ __device__ constexpr double dp_a(int s, int i) {
  constexpr double t[7][6] = {
      {0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
      {1.0 / 5.0, 0.0, 0.0, 0.0, 0.0, 0.0},
      {3.0 / 40.0, 9.0 / 40.0, 0.0, 0.0, 0.0, 0.0},
      {44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0, 0.0, 0.0, 0.0},
      {19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0, 0.0, 0.0},
      {9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0, 0.0},
      {35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0}};
  return t[s][i];
}
__host__ __device__ constexpr double dp_c(int s) {
  constexpr double t[7] = {0.0, 1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0};
  return t[s];
}
__host__ __device__ constexpr double dp_e(int s) {
  constexpr double t[7] = {-71.0 / 57600.0, 0.0, 71.0 / 16695.0, -71.0 / 1920.0, 17253.0 / 339200.0, -22.0 / 525.0, 1.0 / 40.0};
  return t[s];
}

// Shampine's continuous extension of the pair (SIAM J. Numer. Anal. 23, 1986): over an accepted step the value at
// c + theta h is y + h sum_i K_i b_i(theta), b_i(theta) = theta (P[i][0] + theta (P[i][1] + theta (P[i][2] + theta P[i][3])));
// b_i(1) = b_i.  Row 1 is zero, as b_1 is.
__host__ __device__ constexpr double dp_p(int s, int i) {
  constexpr double t[7][4] = {
      {1.0, -8048581381.0 / 2820520608.0, 8663915743.0 / 2820520608.0, -12715105075.0 / 11282082432.0},
      {0.0, 0.0, 0.0, 0.0},
      {0.0, 131558114200.0 / 32700410799.0, -68118460800.0 / 10900136933.0, 87487479700.0 / 32700410799.0},
      {0.0, -1754552775.0 / 470086768.0, 14199869525.0 / 1410260304.0, -10690763975.0 / 1880347072.0},
      {0.0, 127303824393.0 / 49829197408.0, -318862633887.0 / 49829197408.0, 701980252875.0 / 199316789632.0},
      {0.0, -282668133.0 / 205662961.0, 2019193451.0 / 616988883.0, -1453857185.0 / 822651844.0},
      {0.0, 40617522.0 / 29380423.0, -110615467.0 / 29380423.0, 69997945.0 / 29380423.0}};
  return t[s][i];
}
__host__ __device__ constexpr bool dp_p_row(int s) {
  return dp_p(s, 0) != 0.0 || dp_p(s, 1) != 0.0 || dp_p(s, 2) != 0.0 || dp_p(s, 3) != 0.0;
}

// The stages of one step of width h from (c, y) in the section whose coefficients start at off (n of them per
// control); g = stretch w_k / 2.  v holds the q / t / s arguments of f behind NZ.  Ks: the stages g f; ynew: the
// fifth-order solution.  The seventh stage (f at ynew) is evaluated with ERR, or when stage7 says so.  NG > 0: the NG
// integrals I ride along -- Gs: the stages g g_m at the same arguments (M::eval_fg), Inew by the same row and order.
template <class M, bool ERR, int NG, class Args>
__device__ __forceinline__ void prop_stages(const Args& A, double* v, const double* y, const double* I, int64_t off, int n, double c,
                                            double h, double g, bool stage7, double (&Ks)[7][S<M>::NY > 0 ? S<M>::NY : 1],
                                            double (&Gs)[7][NG > 0 ? NG : 1], double* ynew, double* Inew) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU, NY1 = NY > 0 ? NY : 1;
  static_for<0, 7>([&](auto s_) {
    constexpr int s = decltype(s_)::value;
    // the stage's state: y + h sum_i a[s][i] K_i, i ascending, zero entries of the tableau left out
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      double acc = 0.0;
      static_for<0, s>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        constexpr double w = dp_a(s, i);
        if constexpr (w != 0.0) acc += w * Ks[i][a];
      });
      v[a] = s == 0 ? y[a] : y[a] + h * acc;
      if constexpr (s == 6) ynew[a] = v[a];
    });
    if constexpr (s == 6)
      static_for<0, NG>([&](auto m_) {
        constexpr int m = decltype(m_)::value;
        double acc = 0.0;
        static_for<0, 6>([&](auto i_) {
          constexpr int i = decltype(i_)::value;
          constexpr double w = dp_a(6, i);
          if constexpr (w != 0.0) acc += w * Gs[i][m];
        });
        Inew[m] = I[m] + h * acc;
      });
    if (s < 6 || ERR || stage7) {
      constexpr double cs = dp_c(s);
      const double cc = s == 0 ? c : c + cs * h;
      static_for<0, NU>([&](auto b_) {
        constexpr int b = decltype(b_)::value;
        v[NY + b] = sol_legendre(A.c.coef_u + (int64_t)b * A.c.NC + off, n, cc);
      });
      double F[NY1];
      M::eval_f(v, F);
      static_for<0, NY>([&](auto a_) { Ks[s][decltype(a_)::value] = g * F[decltype(a_)::value]; });
      if constexpr (NG > 0) {
        // (f stays eval_f's, so that the states round as pc_sol_propagate's do: the common subexpressions of f and g
        // together may associate a shared sum or product differently)
        double Fg[NY1], G[NG];
        M::eval_fg(v, Fg, G);
        static_for<0, NG>([&](auto m_) { Gs[s][decltype(m_)::value] = g * G[decltype(m_)::value]; });
      }
    }
  });
}

// err = max_a |h sum_i e_i K_i,a| / (atol_a + rtol max(|y_a|, |ynew_a|)) over the N components of Ks, folded into err
// (bad: a term is not finite)
template <int N, int N1>
__device__ __forceinline__ void prop_err(const double (&Ks)[7][N1], const double* y, const double* ynew, double h, const double* atol,
                                         double rtol, double& err, bool& bad) {
  static_for<0, N>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    double acc = 0.0;
    static_for<0, 7>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      constexpr double w = dp_e(i);
      if constexpr (w != 0.0) acc += w * Ks[i][a];
    });
    const double r = fabs(h * acc) / (atol[a] + rtol * fmax(fabs(y[a]), fabs(ynew[a])));
    if (!(r <= 1.7976931348623157e308)) bad = true;   // NaN or inf (fmax would drop a NaN)
    err = fmax(err, r);
  });
}

// One node interval of a lane's walk: its section's slice of the coefficient arrays (n per control from off), the
// section's start and width in tau (a point's c is 2 (tau - ta) / w - 1), the interval's ends in c, g = stretch w_k / 2.
struct PropInterval {
  int64_t off;
  int n;
  double ta, w, ca, cb, g;
};

// The walk of one lane over the node intervals of its segment, for every method: the start from the node value and
// column 0, the section step, the interval's constants, the steps StepControl places (pc_step_control.hpp), what is
// behind a failure, the arriving columns and seg_status.  The method supplies
//   Control                                        its constants for StepControl;
//   start(first, y)                                its own state at the segment's start; first: its writes to column 0;
//   open(j)                                        before interval (j, j+1), run or not;
//   attempt<FIXED>(iv, v, y, c, h, ce, ynew, err, bad)   one attempt of width h from (c, y) that ends at ce: ynew and, in
//                                                  adaptive mode, err and bad; false: a Newton failure;
//   accept(iv, y, ynew, c, h, ce)                  the attempt was accepted, before y becomes ynew;
//   arrive(j, ctl, failed)                         its own columns at node j + 1 (failed: at or behind a failure, where
//                                                  ctl's counts are zero behind it).
template <class M, class Method>
__device__ __forceinline__ void prop_walk(const PcSolPropCommon& P, Method& mth) {
  using St = S<M>;
  constexpr int NY = St::NY, NY1 = NY > 0 ? NY : 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n_seg) return;
  const int N = P.v.N;
  const int32_t* sec_s = P.v.sec_s;
  const int j0 = P.seg_node[i], j1 = P.seg_node[i + 1];
  int k = P.seg_sec[i];
  double t0, tF;
  sol_times<M>(P.v, t0, tF);
  const double stretch = 0.5 * (tF - t0);
  double v[St::NV > 0 ? St::NV : 1], y[NY1], ynew[NY1];
  sol_params<M>(P.v, v);
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    y[a] = P.c.node_y[(int64_t)a * N + j0];
    if (j0 == 0) P.y_arrive[(int64_t)a * N] = y[a];
  });
  if (j0 == 0) P.accepted[0] = P.rejected[0] = 0;
  mth.start(j0 == 0, y);
  int status = -1;
  StepControl<typename Method::Control> ctl;
  for (int j = j0; j < j1; ++j) {
    mth.open(j);
    if (status >= 0) {   // behind the interval that failed
      ctl.clear();
    } else {
      if (j >= sec_s[k + 1] && k < P.v.K - 1) ++k;
      const int sk = sec_s[k];
      PropInterval iv;
      iv.n = sec_s[k + 1] - sk + 1;
      iv.off = (int64_t)sk + k;
      iv.ta = P.c.sec_tau[k];
      iv.w = P.c.sec_tau[k + 1] - iv.ta;
      iv.ca = 2.0 * (P.tau[j] - iv.ta) / iv.w - 1.0;
      iv.cb = 2.0 * (P.tau[j + 1] - iv.ta) / iv.w - 1.0;
      iv.g = stretch * (0.5 * iv.w);
      auto steps = [&](auto fixed_) {   // a loop per mode: the attempt knows the mode at compile time
        if (fixed_) ctl.start_fixed(iv.ca, iv.cb, P.substeps);
        else ctl.start_adaptive(iv.ca, iv.cb);
        while (ctl.more(P.max_steps)) {
          const double c = ctl.c, h = ctl.h, ce = ctl.end();
          double err = 0.0;
          bool bad = false;
          const bool newton_ok = mth.template attempt<decltype(fixed_)::value>(iv, v, y, c, h, ce, ynew, err, bad);
          ctl.report(newton_ok, bad, err, [&]() {
            mth.accept(iv, y, ynew, c, h, ce);
            static_for<0, NY>([&](auto a_) { y[decltype(a_)::value] = ynew[decltype(a_)::value]; });
          });
        }
      };
      if (P.substeps > 0) steps(std::true_type{});
      else steps(std::false_type{});
      if (ctl.failed()) status = j;
    }
    P.accepted[j + 1] = ctl.n_acc;
    P.rejected[j + 1] = ctl.n_rej;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      P.y_arrive[(int64_t)a * N + j + 1] = status >= 0 ? __builtin_nan("") : y[a];
    });
    mth.arrive(j, ctl, status >= 0);
  }
  P.seg_status[i] = status;
}

// pc_sol_propagate: prop_stages without integrals; the seventh stage and the error norm in adaptive mode only.
template <class M>
struct PropDopri5 {
  using Control = StepDopri5;
  static constexpr int NY = S<M>::NY, NY1 = NY > 0 ? NY : 1;
  const PcSolPropCommon& P;
  __device__ __forceinline__ void start(bool, const double*) {}
  __device__ __forceinline__ void open(int) {}
  template <bool FIXED>
  __device__ __forceinline__ bool attempt(const PropInterval& iv, double* v, const double* y, double c, double h, double,
                                          double* ynew, double& err, bool& bad) {
    double Ks[7][NY1], Gs[7][1];
    prop_stages<M, !FIXED, 0>(P, v, y, nullptr, iv.off, iv.n, c, h, iv.g, false, Ks, Gs, ynew, nullptr);
    if constexpr (!FIXED) prop_err<NY, NY1>(Ks, y, ynew, h, P.atol, P.rtol, err, bad);
    return true;
  }
  __device__ __forceinline__ void accept(const PropInterval&, const double*, const double*, double, double, double) {}
  __device__ __forceinline__ void arrive(int, const StepControl<Control>&, bool) {}
};

template <class M>
__device__ __forceinline__ void sol_propagate(const PcSolPropagateArgs& A) {
  PropDopri5<M> mth{A.p};
  prop_walk<M>(A.p, mth);
}

// ---------------------------------------------------------------------------------------------
// Propagation with integrals and dense output.  pc_sol_propagate_dense_p<i>: the lane of pc_sol_propagate,
// with the same steps, carries the phase's NQ integrals I (dI_m/dc = g g_m at the stage arguments of f, I = 0 at the
// segment's first node) and, after every accepted step, answers the sorted queries of its node interval that the step
// reaches: Shampine's interpolant for a query inside the step, the new state itself for a query at its end.  The
// interval that ends at node j owns the sorted queries node_q0[j] .. node_q0[j+1] (slot 0: the queries at tau_0, answered
// with y(0) and 0 by the lane that starts there); a query's c is formed as the nodes' is.  Answers are scattered to
// column q_order[k]: the lane's own columns only.  Without integral_atol the integrals take no part in the error norm,
// and the steps are pc_sol_propagate's to the bit.  No LDS, no atomics; the query cursor is bounded by Q.
// ---------------------------------------------------------------------------------------------
template <class M>
struct PropDense {
  using Control = StepDopri5;
  static constexpr int NY = S<M>::NY, NQ = S<M>::NQ, NY1 = NY > 0 ? NY : 1, NQ1 = NQ > 0 ? NQ : 1;
  const PcSolPropagateDenseArgs& A;
  double I[NQ1], Inew[NQ1], Ks[7][NY1], Gs[7][NQ1];
  int kq, kq1;   // the sorted queries of the interval that no step has answered yet
  bool hit;      // a query falls into the attempt

  __device__ __forceinline__ explicit PropDense(const PcSolPropagateDenseArgs& a) : A(a) {}
  __device__ __forceinline__ void start(bool first, const double* y) {
    const int N = A.p.v.N;
    const int64_t Q = A.Q;
    static_for<0, NQ>([&](auto m_) {
      constexpr int m = decltype(m_)::value;
      I[m] = 0.0;
      if (first) A.q_arrive[(int64_t)m * N] = 0.0;
    });
    if (first)
      for (int q = A.node_q0[0]; q < A.node_q0[1] && q < Q; ++q) {   // the queries at tau_0
        const int64_t col = A.q_order[q];
        static_for<0, NY>([&](auto a_) { A.y_dense[(int64_t) decltype(a_)::value * Q + col] = y[decltype(a_)::value]; });
        static_for<0, NQ>([&](auto m_) { A.q_dense[(int64_t) decltype(m_)::value * Q + col] = 0.0; });
      }
  }
  __device__ __forceinline__ void open(int j) {
    kq = A.node_q0[j + 1];
    kq1 = A.node_q0[j + 2] < A.Q ? A.node_q0[j + 2] : (int)A.Q;
  }
  template <bool FIXED>
  __device__ __forceinline__ bool attempt(const PropInterval& iv, double* v, const double* y, double c, double h, double ce,
                                          double* ynew, double& err, bool& bad) {
    if constexpr (FIXED) {   // the seventh stage only where a query falls into the step
      hit = kq < kq1 && 2.0 * (A.tau_q[kq] - iv.ta) / iv.w - 1.0 <= ce;
      prop_stages<M, false, NQ>(A.p, v, y, I, iv.off, iv.n, c, h, iv.g, hit, Ks, Gs, ynew, Inew);
    } else {
      hit = true;
      prop_stages<M, true, NQ>(A.p, v, y, I, iv.off, iv.n, c, h, iv.g, true, Ks, Gs, ynew, Inew);
      prop_err<NY, NY1>(Ks, y, ynew, h, A.p.atol, A.p.rtol, err, bad);
      if (A.integral_atol) prop_err<NQ, NQ1>(Gs, I, Inew, h, A.integral_atol, A.p.rtol, err, bad);
    }
    return true;
  }
  // the queries the step from c of width h to ce reaches (ynew, Inew, Ks, Gs are its own), then the integrals advance
  __device__ __forceinline__ void accept(const PropInterval& iv, const double* y, const double* ynew, double c, double h, double ce) {
    const int64_t Q = A.Q;
    while (hit && kq < kq1) {
      const double cq = 2.0 * (A.tau_q[kq] - iv.ta) / iv.w - 1.0;
      if (!(cq <= ce)) break;
      const int64_t col = A.q_order[kq];
      if (cq == ce) {
        static_for<0, NY>([&](auto a_) { A.y_dense[(int64_t) decltype(a_)::value * Q + col] = ynew[decltype(a_)::value]; });
        static_for<0, NQ>([&](auto m_) { A.q_dense[(int64_t) decltype(m_)::value * Q + col] = Inew[decltype(m_)::value]; });
      } else {
        const double th = fmax((cq - c) / h, 0.0);
        double b[7];
        static_for<0, 7>([&](auto i_) {
          constexpr int ii = decltype(i_)::value;
          b[ii] = th * (dp_p(ii, 0) + th * (dp_p(ii, 1) + th * (dp_p(ii, 2) + th * dp_p(ii, 3))));
        });
        static_for<0, NY>([&](auto a_) {
          constexpr int a = decltype(a_)::value;
          double acc = 0.0;
          static_for<0, 7>([&](auto i_) {
            constexpr int ii = decltype(i_)::value;
            if constexpr (dp_p_row(ii)) acc += Ks[ii][a] * b[ii];
          });
          A.y_dense[(int64_t)a * Q + col] = y[a] + h * acc;
        });
        static_for<0, NQ>([&](auto m_) {
          constexpr int m = decltype(m_)::value;
          double acc = 0.0;
          static_for<0, 7>([&](auto i_) {
            constexpr int ii = decltype(i_)::value;
            if constexpr (dp_p_row(ii)) acc += Gs[ii][m] * b[ii];
          });
          A.q_dense[(int64_t)m * Q + col] = I[m] + h * acc;
        });
      }
      ++kq;
    }
    static_for<0, NQ>([&](auto m_) { I[decltype(m_)::value] = Inew[decltype(m_)::value]; });
  }
  __device__ __forceinline__ void arrive(int j, const StepControl<Control>&, bool failed) {
    const int N = A.p.v.N;
    const int64_t Q = A.Q;
    const double nan = __builtin_nan("");
    static_for<0, NQ>([&](auto m_) {
      constexpr int m = decltype(m_)::value;
      A.q_arrive[(int64_t)m * N + j + 1] = failed ? nan : I[m];
    });
    for (; kq < kq1; ++kq) {   // the queries no accepted step has reached: behind the failure
      const int64_t col = A.q_order[kq];
      static_for<0, NY>([&](auto a_) { A.y_dense[(int64_t) decltype(a_)::value * Q + col] = nan; });
      static_for<0, NQ>([&](auto m_) { A.q_dense[(int64_t) decltype(m_)::value * Q + col] = nan; });
    }
  }
};

template <class M>
__device__ __forceinline__ void sol_propagate_dense(const PcSolPropagateDenseArgs& A) {
  PropDense<M> mth(A);
  prop_walk<M>(A.p, mth);
}

// ---------------------------------------------------------------------------------------------
// ph mesh-error estimate (pycollo/mesh_refinement.py:63-240 + solution/solution_abc.py:60-107)
// pc_mesh_err_p<i>: one workgroup per run of sections; section k owns n_k + 1 consecutive lanes = its nodes on the
// "ph mesh" (one node more per section).  Lane j < n_k also evaluates solution node j of the section.
//   1. f at the solution nodes                      (casadi_solution.py:71)
//   2. states / controls at the interior ph nodes from the section's interpolants, as two small
//      table contractions:  y_ph = y_start + stretch h_k B f,   u_ph = E u   (solution_abc.py:70-100)
//   3. f at the ph nodes, Y_ph = y_start + stretch h_k A_(n+1) f_ph          (mesh_refinement.py:199-210)
//   4. |Y_ph - y_ph| relative to 1 + (1 + max|y_ph|) per state, section maximum (mesh_refinement.py:211-233)
// ---------------------------------------------------------------------------------------------
// maximum that keeps a NaN from either side, as np.max does (fmax returns the other operand)
__device__ __forceinline__ double nan_max(double m, double x) { return (x > m || x != x) ? x : m; }

template <class M>
__device__ __forceinline__ void mesh_error(const PcRefineArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  const PcPhaseView& V = A.v;
  double* s_B = smem;
  double* s_E = s_B + A.tab_total_BE;
  double* s_A = s_E + A.tab_total_BE;
  double* s_fs = s_A + A.tab_total_A;          // [NY][TB] f at solution nodes
  double* s_ys = s_fs + NY * TB;               // [NY][TB] y at solution nodes
  double* s_us = s_ys + NY * TB;               // [NU][TB]
  double* s_yp = s_us + (NU > 0 ? NU : 1) * TB;  // [NY][TB] y on the ph mesh
  double* s_fp = s_yp + NY * TB;               // [NY][TB] f on the ph mesh
  double* s_re = s_fp + NY * TB;               // [TB] row maxima of the relative error
  double* s_ae = s_re + TB;                    // [NY][TB] absolute errors
  int* s_sec = reinterpret_cast<int*>(s_ae + NY * TB);   // [TB] section of every lane
  for (int i = tid; i < A.tab_total_BE; i += TB) {
    s_B[i] = A.tabB[i];
    s_E[i] = A.tabE[i];
  }
  for (int i = tid; i < A.tab_total_A; i += TB) s_A[i] = A.tabA[i];
  const SolLane L = sol_lane_map(V, A.tile_k0[blockIdx.x], A.tile_k0[blockIdx.x + 1], A.lane0, 1, s_sec);
  const bool active = L.active;
  const int k = L.k, n = L.n, j = L.j, l0 = L.l0;
  double t0, tF;
  sol_times<M>(V, t0, tF);
  const double stretch = 0.5 * (tF - t0);
  double h = 0.0;
  double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1];
  if (active) {
    h = A.sec_h[k];
    sol_params<M>(V, v);
    if (j < n) {   // this lane doubles as solution node j of its section
      sol_node<M>(V, L.sk + j, v);
      M::eval_f(v, F);
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        s_fs[a * TB + tid] = F[a];
        s_ys[a * TB + tid] = v[a];
      });
      static_for<0, NU>([&](auto b_) { s_us[decltype(b_)::value * TB + tid] = v[NY + decltype(b_)::value]; });
    }
  }
  __syncthreads();
  if (active) {
    if (j == 0 || j == n) {   // section boundaries keep the solution's values (mesh_refinement.py:164-166,176-178)
      const int src = l0 + (j == 0 ? 0 : n - 1);
      static_for<0, NY>([&](auto a_) { v[decltype(a_)::value] = s_ys[decltype(a_)::value * TB + src]; });
      static_for<0, NU>([&](auto b_) { v[NY + decltype(b_)::value] = s_us[decltype(b_)::value * TB + src]; });
    } else {
      const int row = A.offBE[n] + (j - 1) * n;
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        v[a] = s_ys[a * TB + l0] + stretch * (h * sol_row_dot(s_B + row, s_fs + a * TB + l0, n));
      });
      static_for<0, NU>([&](auto b_) {
        constexpr int b = decltype(b_)::value;
        v[NY + b] = sol_row_dot(s_E + row, s_us + b * TB + l0, n);
      });
    }
    M::eval_f(v, F);
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      s_yp[a * TB + tid] = v[a];
      s_fp[a * TB + tid] = F[a];
    });
  }
  __syncthreads();
  double rel = 0.0;
  if (active && j >= 1) {
    const double* At = s_A + A.offA[n] + (j - 1) * (n + 1);
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      const double Yph = s_yp[a * TB + l0] + stretch * (h * sol_row_dot(At, s_fp + a * TB + l0, n + 1));
      const double err = fabs(Yph - s_yp[a * TB + tid]);
      double mx = 0.0;
      for (int i = 1; i <= n; ++i) mx = nan_max(mx, fabs(s_yp[a * TB + l0 + i]));
      rel = nan_max(rel, err / (1.0 + (mx + 1.0)));
      s_ae[a * TB + tid] = err;
    });
    s_re[tid] = rel;
  }
  __syncthreads();
  if (active && j == 0) {
    double m = 0.0;
    for (int i = 1; i <= n; ++i) m = nan_max(m, s_re[l0 + i]);
    A.max_rel[k] = m;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      double ma = 0.0;
      for (int i = 1; i <= n; ++i) ma = nan_max(ma, s_ae[a * TB + l0 + i]);
      A.max_abs[(int64_t)k * NY + a] = ma;
    });
  }
}

// ---------------------------------------------------------------------------------------------
// Implicit propagation: the setting of pc_sol_propagate (segments, node intervals, the section variable c,
// dy/dc = g f(y, u(c), ...), g = stretch w_k / 2, no step astride a node), integrated by the five-stage SDIRK method of
// Hairer & Wanner (Solving ODEs II, IV.6): order 4, gamma = 1/4, stiffly accurate, L-stable, embedded weights of order 3.
//
// pc_sol_propagate_stiff_p<i>: one lane per segment, one wave per workgroup.  One attempt of width h from (c, y):
//   J = g df/dy from one M::eval_fj at (y, u(c)) (the entries with row and column below NY); W = I - h gamma J factored
//   by LU with partial pivoting (largest |entry| of the column, the lowest row on ties), once, for the five stages and
//   the error filter; a pivot that is zero or not finite is a Newton failure.
//   Stage i: u_i = u(c + c_i h) once; K starts as K_{i-1} (g f(y, u(c)) for stage 1); up to newton_max times
//     Y = y + h (sum_{l<i} a_il K_l + gamma K),  r = g f(Y, u_i) - K,  dK = W^-1 r,  K += dK,
//     theta = max_a |h gamma dK_a| / (atol_a + rtol max(|y_a|, |Y_a|));  theta <= 0.01 ends the stage; a theta that is
//     not finite, or newton_max used up, is a Newton failure.
//   ynew = y + h sum_i b_i K_i;  e = W^-1 (h sum_i (b_i - b^_i) K_i);  err = max_a |e_a| / (atol_a + rtol max(|y_a|, |ynew_a|)).
//   adaptive (substeps = 0): as pc_sol_propagate with factor = clamp(0.9 err^(-1/4), 0.2, 5); a Newton failure rejects
//     with factor 0.25 and counts in rejected and in newton_rejected.
//   fixed (substeps = m): m steps as pc_sol_propagate places them; a Newton failure ends the lane at that interval as
//     the cap does (the failed attempt is the interval's one rejected step).
// The five stage vectors and y live in registers, fully unrolled.  The factors and the row swaps live in LDS, element e
// of the lane's column at [e * PC_SOL_PROP_TB + lane]: lanes that read the same element read consecutive words, no lane
// reads another lane's column, so there is no barrier and no atomic.  Every loop is bounded by max_steps, substeps,
// newton_max, NY or N.  A phase with NY > PC_SOL_STIFF_MAX_NY gets an empty kernel; the host call refuses it.
// ---------------------------------------------------------------------------------------------
__host__ __device__ constexpr double sd_a(int s, int i) {
  constexpr double t[5][5] = {{1.0 / 4.0, 0.0, 0.0, 0.0, 0.0},
                              {1.0 / 2.0, 1.0 / 4.0, 0.0, 0.0, 0.0},
                              {17.0 / 50.0, -1.0 / 25.0, 1.0 / 4.0, 0.0, 0.0},
                              {371.0 / 1360.0, -137.0 / 2720.0, 15.0 / 544.0, 1.0 / 4.0, 0.0},
                              {25.0 / 24.0, -49.0 / 48.0, 125.0 / 16.0, -85.0 / 12.0, 1.0 / 4.0}};   // row 5 = b
  return t[s][i];
}
__host__ __device__ constexpr double sd_c(int s) {
  constexpr double t[5] = {1.0 / 4.0, 3.0 / 4.0, 11.0 / 20.0, 1.0 / 2.0, 1.0};
  return t[s];
}
__host__ __device__ constexpr double sd_e(int s) {   // b - b^
  constexpr double t[5] = {-3.0 / 16.0, -27.0 / 32.0, 25.0 / 32.0, 0.0, 1.0 / 4.0};
  return t[s];
}
constexpr double SD_GAMMA = 1.0 / 4.0;
constexpr double SD_NEWTON_TOL = 0.01;

// the lane's column of LDS: element (r, c) of its NY x NY block, and row swap k
#define PC_SD_LU(r, c) lu[((r) * NY + (c)) * PC_SOL_PROP_TB + lane]
#define PC_SD_PIV(k) piv[(k) * PC_SOL_PROP_TB + lane]

// LU with partial pivoting in place: rows swapped whole, unit lower factor below the diagonal.  false: a pivot is zero
// or not finite.
template <int NY>
__device__ __forceinline__ bool stiff_factor(double* lu, int32_t* piv, int lane) {
#pragma unroll 1
  for (int k = 0; k < NY; ++k) {
    int p = k;
    double best = fabs(PC_SD_LU(k, k));
    for (int r = k + 1; r < NY; ++r) {
      const double m = fabs(PC_SD_LU(r, k));
      if (m > best) {
        best = m;
        p = r;
      }
    }
    PC_SD_PIV(k) = p;
    if (p != k)
      for (int c = 0; c < NY; ++c) {
        const double t = PC_SD_LU(k, c);
        PC_SD_LU(k, c) = PC_SD_LU(p, c);
        PC_SD_LU(p, c) = t;
      }
    const double d = PC_SD_LU(k, k);
    if (!(best <= 1.7976931348623157e308) || d == 0.0) return false;
#pragma unroll 1
    for (int r = k + 1; r < NY; ++r) {
      const double l = PC_SD_LU(r, k) / d;
      PC_SD_LU(r, k) = l;
      for (int c = k + 1; c < NY; ++c) PC_SD_LU(r, c) = PC_SD_LU(r, c) - l * PC_SD_LU(k, c);
    }
  }
  return true;
}

// r <- W^-1 r from the factors: all row swaps first, then the unit lower and the upper triangle.  r stays in registers:
// a swap with a run-time row is a chain of selects.
template <int NY>
__device__ __forceinline__ void stiff_solve(const double* lu, const int32_t* piv, int lane, double* r) {
  static_for<0, NY>([&](auto k_) {
    constexpr int k = decltype(k_)::value;
    const int p = PC_SD_PIV(k);
    static_for<k + 1, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      const double rk = r[k], ra = r[a];
      r[k] = p == a ? ra : rk;
      r[a] = p == a ? rk : ra;
    });
  });
  static_for<0, NY>([&](auto k_) {
    constexpr int k = decltype(k_)::value;
    static_for<k + 1, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      r[a] = r[a] - PC_SD_LU(a, k) * r[k];
    });
  });
  static_for<0, NY>([&](auto q_) {
    constexpr int k = NY - 1 - decltype(q_)::value;
    static_for<k + 1, NY>([&](auto c_) {
      constexpr int c = decltype(c_)::value;
      r[k] = r[k] - PC_SD_LU(k, c) * r[c];
    });
    r[k] = r[k] / PC_SD_LU(k, k);
  });
}

// One attempt of width h from (c, y).  false: a Newton failure (ynew and err are then not set).  iters counts the
// Newton iterations made.  err is the scaled norm of the filtered estimate (bad: it is not finite).
template <class M>
__device__ __forceinline__ bool stiff_step(const PcSolPropagateStiffArgs& A, double* lu, int32_t* piv, int lane, double* v,
                                           const double* y, int64_t off, int n, double c, double h, double g, double* ynew,
                                           double& err, bool& bad, int& iters) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU, NY1 = NY > 0 ? NY : 1, NJ = St::NJ, NFN = St::NFN;
  double Ks[5][NY1], Kc[NY1];
  const double hg = h * SD_GAMMA;
  {
    double F[NFN > 0 ? NFN : 1], Jv[NJ > 0 ? NJ : 1];
    static_for<0, NY>([&](auto a_) { v[decltype(a_)::value] = y[decltype(a_)::value]; });
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      v[NY + b] = sol_legendre(A.p.c.coef_u + (int64_t)b * A.p.c.NC + off, n, c);
    });
    M::eval_fj(v, F, Jv);
    static_for<0, NY>([&](auto a_) { Kc[decltype(a_)::value] = g * F[decltype(a_)::value]; });
    for (int e = 0; e < NY * NY; ++e) lu[e * PC_SOL_PROP_TB + lane] = 0.0;
    static_for<0, NY>([&](auto a_) { PC_SD_LU(decltype(a_)::value, decltype(a_)::value) = 1.0; });
    static_for<0, NJ>([&](auto e_) {
      constexpr int e = decltype(e_)::value;
      if constexpr (M::jr(e) < NY && M::jc(e) < NY)
        PC_SD_LU(M::jr(e), M::jc(e)) = (M::jr(e) == M::jc(e) ? 1.0 : 0.0) - hg * (g * Jv[e]);
    });
  }
  if (!stiff_factor<NY>(lu, piv, lane)) return false;
  bool ok = true;
  static_for<0, 5>([&](auto s_) {
    constexpr int s = decltype(s_)::value;
    // (no branch around a stage: a failed stage leaves the Newton loops of the later ones empty)
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      v[NY + b] = sol_legendre(A.p.c.coef_u + (int64_t)b * A.p.c.NC + off, n, c + sd_c(s) * h);
    });
    double base[NY1];   // sum_{l<s} a_sl K_l, l ascending, zero entries of the tableau left out
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      double acc = 0.0;
      static_for<0, s>([&](auto l_) {
        constexpr int l = decltype(l_)::value;
        constexpr double w = sd_a(s, l);
        if constexpr (w != 0.0) acc += w * Ks[l][a];
      });
      base[a] = acc;
    });
    bool conv = false;
    for (int it = 0; it < A.newton_max && !conv && ok; ++it) {
      ++iters;
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        v[a] = y[a] + h * (base[a] + SD_GAMMA * Kc[a]);
      });
      double F[NY1], r[NY1];
      M::eval_f(v, F);
      static_for<0, NY>([&](auto a_) { r[decltype(a_)::value] = g * F[decltype(a_)::value] - Kc[decltype(a_)::value]; });
      stiff_solve<NY>(lu, piv, lane, r);
      double theta = 0.0;
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        Kc[a] += r[a];
        const double q = fabs(hg * r[a]) / (A.p.atol[a] + A.p.rtol * fmax(fabs(y[a]), fabs(v[a])));
        if (!(q <= 1.7976931348623157e308)) ok = false;   // NaN or inf (fmax would drop a NaN)
        theta = fmax(theta, q);
      });
      conv = ok && theta <= SD_NEWTON_TOL;
    }
    if (!conv) ok = false;
    static_for<0, NY>([&](auto a_) { Ks[s][decltype(a_)::value] = Kc[decltype(a_)::value]; });
  });
  if (!ok) return false;
  double e[NY1];
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    double acc = 0.0, ace = 0.0;
    static_for<0, 5>([&](auto i_) {
      constexpr int i = decltype(i_)::value;
      constexpr double w = sd_a(4, i), we = sd_e(i);
      if constexpr (w != 0.0) acc += w * Ks[i][a];
      if constexpr (we != 0.0) ace += we * Ks[i][a];
    });
    ynew[a] = y[a] + h * acc;
    e[a] = h * ace;
  });
  stiff_solve<NY>(lu, piv, lane, e);
  err = 0.0;
  bad = false;
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    const double q = fabs(e[a]) / (A.p.atol[a] + A.p.rtol * fmax(fabs(y[a]), fabs(ynew[a])));
    if (!(q <= 1.7976931348623157e308)) bad = true;
    err = fmax(err, q);
  });
  return true;
}

// (This kernel is not yet a method of prop_walk: as one, it took two more VGPRs on many models and lost a wave per SIMD
// on the tumour and the double-pendulum models, and what kept the pair live was not found.  Its walk and its step
// control below are pc_sol_propagate's, restated; StepControl<StepSdirk4> states the same control and is tested.)
template <class M>
__device__ __forceinline__ void sol_propagate_stiff(const PcSolPropagateStiffArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NY1 = NY > 0 ? NY : 1;
  if constexpr (NY <= PC_SOL_STIFF_MAX_NY) {
    __shared__ double lu[NY1 * NY1 * PC_SOL_PROP_TB];
    __shared__ int32_t piv[NY1 * PC_SOL_PROP_TB];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.p.n_seg || lane >= PC_SOL_PROP_TB) return;
    const int N = A.p.v.N;
    const int32_t* sec_s = A.p.v.sec_s;
    const int j0 = A.p.seg_node[i], j1 = A.p.seg_node[i + 1];
    int k = A.p.seg_sec[i];
    double t0, tF;
    sol_times<M>(A.p.v, t0, tF);
    const double stretch = 0.5 * (tF - t0);
    double v[St::NV > 0 ? St::NV : 1], y[NY1], ynew[NY1];
    sol_params<M>(A.p.v, v);
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      y[a] = A.p.c.node_y[(int64_t)a * N + j0];
      if (j0 == 0) A.p.y_arrive[(int64_t)a * N] = y[a];
    });
    if (j0 == 0) A.p.accepted[0] = A.p.rejected[0] = A.newton_rejected[0] = A.newton_iterations[0] = 0;
    const bool fixed = A.p.substeps > 0;
    int status = -1;
    for (int j = j0; j < j1; ++j) {
      if (status >= 0) {   // behind the interval that failed
        static_for<0, NY>([&](auto a_) { A.p.y_arrive[(int64_t) decltype(a_)::value * N + j + 1] = __builtin_nan(""); });
        A.p.accepted[j + 1] = A.p.rejected[j + 1] = A.newton_rejected[j + 1] = A.newton_iterations[j + 1] = 0;
        continue;
      }
      if (j >= sec_s[k + 1] && k < A.p.v.K - 1) ++k;
      const int sk = sec_s[k], n = sec_s[k + 1] - sk + 1;
      const int64_t off = (int64_t)sk + k;
      const double ta = A.p.c.sec_tau[k], w = A.p.c.sec_tau[k + 1] - ta;
      const double ca = 2.0 * (A.p.tau[j] - ta) / w - 1.0, cb = 2.0 * (A.p.tau[j + 1] - ta) / w - 1.0;
      const double g = stretch * (0.5 * w);
      int n_acc = 0, n_rej = 0, n_newt = 0, iters = 0;
      const double h0 = fixed ? (cb - ca) / (double)A.p.substeps : cb - ca;
      double c = ca, h = h0;
      bool last = true, after_reject = false, done = false;
      while (!done && (fixed || n_acc + n_rej < A.p.max_steps)) {
        if (fixed) {   // step q starts at ca + q h0 (computed, not accumulated); the last one ends at cb
          c = ca + (double)n_acc * h0;
          h = n_acc == A.p.substeps - 1 ? cb - c : h0;
        }
        double err = 0.0;
        bool bad = false;
        const bool newton = stiff_step<M>(A, lu, piv, lane, v, y, off, n, c, h, g, ynew, err, bad, iters);
        if (fixed) {
          if (!newton) {
            ++n_rej;
            ++n_newt;
            break;
          }
          ++n_acc;
          static_for<0, NY>([&](auto a_) { y[decltype(a_)::value] = ynew[decltype(a_)::value]; });
          done = n_acc == A.p.substeps;
          continue;
        }
        double factor = newton ? 0.2 : 0.25;
        if (newton && !bad) factor = err == 0.0 ? 5.0 : fmin(5.0, fmax(0.2, 0.9 * pow(err, -0.25)));
        if (newton && !bad && err <= 1.0) {
          ++n_acc;
          static_for<0, NY>([&](auto a_) { y[decltype(a_)::value] = ynew[decltype(a_)::value]; });
          c = last ? cb : c + h;
          if (after_reject) factor = fmin(factor, 1.0);
          after_reject = false;
          const double rest = cb - c;
          if (last || !(rest > 0.0)) {
            done = true;
          } else {
            h *= factor;
            last = h >= rest;
            if (last) h = rest;
          }
        } else {
          ++n_rej;
          if (!newton) ++n_newt;
          h *= factor;
          last = false;
          after_reject = true;
        }
      }
      if (!done) status = j;
      A.p.accepted[j + 1] = n_acc;
      A.p.rejected[j + 1] = n_rej;
      A.newton_rejected[j + 1] = n_newt;
      A.newton_iterations[j + 1] = iters;
      static_for<0, NY>([&](auto a_) {
        constexpr int a = decltype(a_)::value;
        A.p.y_arrive[(int64_t)a * N + j + 1] = status >= 0 ? __builtin_nan("") : y[a];
      });
    }
    A.p.seg_status[i] = status;
  }
}
#undef PC_SD_LU
#undef PC_SD_PIV

}  // namespace pc

// the seven entry points of phase I, instantiated by the generated source once per phase (pc_mesh_err_p<i> is emitted by
// the generator itself)
#define PC_SOL_ENTRY_POINTS(I)                                                                               \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_fit_p##I(PcSolFitArgs a) {                        \
    pc::sol_fit<gen::Phase##I>(a);                                                                           \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_sample_p##I(PcSolSampleArgs a) {                  \
    pc::sol_sample<gen::Phase##I>(a);                                                                        \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_costate_p##I(PcSolCostateArgs a) {                \
    pc::sol_costate<gen::Phase##I>(a);                                                                       \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_sample_costate_p##I(PcSolCostateSampleArgs a) {   \
    pc::sol_sample_costate<gen::Phase##I>(a);                                                                \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(PC_SOL_PROP_TB) pc_sol_propagate_p##I(PcSolPropagateArgs a) { \
    pc::sol_propagate<gen::Phase##I>(a);                                                                     \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(PC_SOL_PROP_TB) pc_sol_propagate_dense_p##I(PcSolPropagateDenseArgs a) { \
    pc::sol_propagate_dense<gen::Phase##I>(a);                                                               \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(PC_SOL_PROP_TB) pc_sol_propagate_stiff_p##I(PcSolPropagateStiffArgs a) { \
    pc::sol_propagate_stiff<gen::Phase##I>(a);                                                               \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_multipliers_p##I(PcSolMultiplierArgs a) {         \
    pc::sol_multipliers<gen::Phase##I>(a);                                                                   \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_sample_optimality_p##I(PcSolOptimalitySampleArgs a) { \
    pc::sol_sample_optimality<gen::Phase##I>(a);                                                             \
  }

#endif  // PC_SOLUTION_HPP
