// Dense output of an NLP point (pycollo/solution/solution_abc.py:60-142, casadi_solution.py:15-86): device side.
// Included by the generated code object after pc_kernels.hpp (S<M>, static_for, M::eval_f).
//
// Per section k (n nodes, section variable c in [-1, 1]):
//   ydot(c) = sum_m a_m P_m(c),  a = tabD_n . f(nodes)      (Lobatto: degree n-1; Radau: degree n-2, last row of tabD zero)
//   u(c)    = sum_m e_m P_m(c),  e = tabU_n . u(nodes)      (degree n-1 through all n nodes)
//   y(c)    = y(tau_k) + stretch (h_k / 2) sum_m a_m int_{-1}^{c} P_m,   int P_m = (P_{m+1} - P_{m-1}) / (2m + 1)
// Both sums are evaluated by Clenshaw's recurrence.
#ifndef PC_SOLUTION_HPP
#define PC_SOLUTION_HPP

namespace pc {

template <class M>
__device__ __forceinline__ void sol_times(const double* __restrict__ x, const double* sc, int64_t x_off, int N,
                                          const double* t_fixed, double& t0, double& tF) {
  using St = S<M>;
  t0 = t_fixed[0];
  tF = t_fixed[1];
  const int64_t t_off = x_off + (int64_t)St::NZ * N + St::NQ;
  int j = 0;
  if constexpr (M::T0_FREE) { t0 = sc[St::O_VT + j] * x[t_off + j] + sc[St::O_RT + j]; ++j; }
  if constexpr (M::TF_FREE) { tF = sc[St::O_VT + j] * x[t_off + j] + sc[St::O_RT + j]; }
}

// the q / t / s arguments of f, unscaled, into v[NZ ..]
template <class M>
__device__ __forceinline__ void sol_params(const double* __restrict__ x, const double* sc, int64_t x_off, int64_t s_off,
                                           int N, double* v) {
  using St = S<M>;
  static_for<0, St::NS>([&](auto l_) {
    constexpr int l = decltype(l_)::value;
    constexpr int kind = M::wk(l), idx = M::wi(l);   // static parameter, or this phase's q / free t
    const int64_t col = kind == 0 ? s_off + idx : x_off + (int64_t)St::NZ * N + (kind == 1 ? idx : St::NQ + idx);
    v[St::NZ + l] = sc[St::O_VS + l] * x[col] + sc[St::O_RS + l];
  });
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
  constexpr int NY = St::NY, NU = St::NU, NZ = St::NZ;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, TB = blockDim.x;
  double* s_D = smem;
  double* s_U = s_D + A.tab_total;
  double* s_f = s_U + A.tab_total;                  // [NY][TB]
  double* s_u = s_f + (NY > 0 ? NY : 1) * TB;       // [NU][TB]
  int* s_sec = reinterpret_cast<int*>(s_u + (NU > 0 ? NU : 1) * TB);   // [TB] section of every lane
  const int k0 = A.tile_k0[blockIdx.x], k1 = A.tile_k0[blockIdx.x + 1];
  for (int i = tid; i < A.tab_total; i += TB) {
    s_D[i] = A.tabD[i];
    s_U[i] = A.tabU[i];
  }
  s_sec[tid] = -1;
  __syncthreads();
  for (int k = k0 + tid; k < k1; k += TB) {
    const int n = A.sec_s[k + 1] - A.sec_s[k] + 1, l0 = A.lane0[k];
    for (int j = 0; j < n; ++j)
      if (l0 + j < TB) s_sec[l0 + j] = k;
  }
  __syncthreads();
  const int k = s_sec[tid];
  const bool active = k >= 0;
  const double* sc = A.scal;
  double t0, tF;
  sol_times<M>(A.x, sc, A.x_off, A.N, A.t_fixed, t0, tF);
  int n = 2, j = 0, l0 = 0, sk = 0;
  if (active) {
    sk = A.sec_s[k];
    n = A.sec_s[k + 1] - sk + 1;
    l0 = A.lane0[k];
    j = tid - l0;
    const int node = sk + j;
    double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1];
    sol_params<M>(A.x, sc, A.x_off, A.s_off, A.N, v);
    static_for<0, NZ>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      v[b] = sc[St::O_VZ + b] * A.x[A.x_off + (int64_t)b * A.N + node] + sc[St::O_RZ + b];
    });
    M::eval_f(v, F);
    // a node shared by two sections is written by the section it opens (the last node: by the last section)
    const bool owner = j < n - 1 || k == A.K - 1;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      s_f[a * TB + tid] = F[a];
      if (owner) {
        A.node_y[(int64_t)a * A.N + node] = v[a];
        A.node_f[(int64_t)a * A.N + node] = F[a];
      }
    });
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      s_u[b * TB + tid] = v[NY + b];
      if (owner) A.node_u[(int64_t)b * A.N + node] = v[NY + b];
    });
    if (owner) A.node_t[node] = A.tau[node] * (0.5 * (tF - t0)) + 0.5 * (t0 + tF);   // casadi_solution.py:80-83
  }
  __syncthreads();
  if (active) {
    const double* Dr = s_D + A.offC[n] + j * n;
    const double* Ur = s_U + A.offC[n] + j * n;
    const int64_t slot = (int64_t)sk + k + j;
    static_for<0, NY>([&](auto a_) {
      constexpr int a = decltype(a_)::value;
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += Dr[i] * s_f[a * TB + l0 + i];
      A.coef_dy[(int64_t)a * A.NC + slot] = acc;
    });
    static_for<0, NU>([&](auto b_) {
      constexpr int b = decltype(b_)::value;
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += Ur[i] * s_u[b * TB + l0 + i];
      A.coef_u[(int64_t)b * A.NC + slot] = acc;
    });
  }
}

// ---------------------------------------------------------------------------------------------
// pc_sol_sample_p<i>: one lane per query.  The lane maps its time to tau, finds its section by bisection over the
// K + 1 section boundaries (a boundary belongs to the section on its right, tau = +1 to the last section) and reads
// the section's coefficients from high to low degree -- one pass feeds the Clenshaw recurrences of ydot and of its
// integral.  Outputs are variable-major [var][Q]: neighbouring lanes write neighbouring doubles.
// ---------------------------------------------------------------------------------------------
template <class M>
__device__ __forceinline__ void sol_sample(const PcSolSampleArgs& A) {
  using St = S<M>;
  constexpr int NY = St::NY, NU = St::NU;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.Q) return;
  const double* sc = A.scal;
  double t0, tF;
  sol_times<M>(A.x, sc, A.x_off, A.N, A.t_fixed, t0, tF);
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
  const double nan = __builtin_nan("");
  if (!(inside || ((A.flags & PC_SOL_EXTRAPOLATE) && tau == tau))) {
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
  // the last boundary <= tau, kept inside [0, K - 1]
  int lo = 0, hi = A.K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.sec_tau[mid] <= tau) lo = mid; else hi = mid;
  }
  const int k = lo;
  const int sk = A.sec_s[k], n = A.sec_s[k + 1] - sk + 1;
  const double ta = A.sec_tau[k], w = A.sec_tau[k + 1] - ta;
  const double c = 2.0 * (tau - ta) / w - 1.0;
  const int64_t off = (int64_t)sk + k;
  double v[St::NV > 0 ? St::NV : 1], F[NY > 0 ? NY : 1];
  static_for<0, NY>([&](auto a_) {
    constexpr int a = decltype(a_)::value;
    const double* cf = A.coef_dy + (int64_t)a * A.NC + off;
    // j = n .. 0: b_j = a_(j-1) / (2j - 1) - a_(j+1) / (2j + 3) are the coefficients of int_{-1}^{c} ydot
    // (b_0 = a_0 - a_1 / 3); ydot's own Clenshaw step j uses a_j
    double a_hi = 0.0, a_mid = 0.0;
    double y1 = 0.0, y2 = 0.0, d1 = 0.0, d2 = 0.0;
    for (int j = n; j >= 0; --j) {
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
    const double y = A.node_y[(int64_t)a * A.N + sk] + stretch * ((0.5 * w) * y1);
    v[a] = y;
    if (A.out_y) A.out_y[(int64_t)a * A.Q + i] = y;
    if (A.out_dy) A.out_dy[(int64_t)a * A.Q + i] = d1;
  });
  static_for<0, NU>([&](auto b_) {
    constexpr int b = decltype(b_)::value;
    const double* cf = A.coef_u + (int64_t)b * A.NC + off;
    double u1 = 0.0, u2 = 0.0;
    for (int j = n - 1; j >= 0; --j) {
      const double al = (double)(2 * j + 1) / (double)(j + 1) * c, be = (double)(j + 1) / (double)(j + 2);
      const double un = cf[j] + (al * u1 - be * u2);
      u2 = u1;
      u1 = un;
    }
    v[NY + b] = u1;
    if (A.out_u) A.out_u[(int64_t)b * A.Q + i] = u1;
  });
  if (A.out_f) {
    sol_params<M>(A.x, sc, A.x_off, A.s_off, A.N, v);
    M::eval_f(v, F);
    static_for<0, NY>([&](auto a_) { A.out_f[(int64_t) decltype(a_)::value * A.Q + i] = F[decltype(a_)::value]; });
  }
}

}  // namespace pc

// the two entry points of phase I, instantiated by the generated source once per phase
#define PC_SOL_ENTRY_POINTS(I)                                                                               \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_fit_p##I(PcSolFitArgs a) {                        \
    pc::sol_fit<gen::Phase##I>(a);                                                                           \
  }                                                                                                          \
  extern "C" __global__ void __launch_bounds__(256) pc_sol_sample_p##I(PcSolSampleArgs a) {                  \
    pc::sol_sample<gen::Phase##I>(a);                                                                        \
  }

#endif  // PC_SOLUTION_HPP
