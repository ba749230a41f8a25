// Dense output of an NLP point: the exported calls (include/pycollo_amd.h: pc_solution_*).  Included at the end of
// pc_engine.hip (same translation unit: it uses the handle, find_fn and DevBuf).  The index arithmetic is
// pc_solution_plan.hpp; the kernels are pc_solution.hpp, compiled into the model's code object.
//
// A solution owns a copy of the point it was made from and everything derived from it; it reads the handle's scaling
// constants once, at creation (fill_phase_view), and launches on the handle's stream.  The one thing it does not copy is
// the section-start table: its kernels read the handle's device copy (sec_s, which a handle never changes), so a solution
// must be destroyed before its handle, as the stream already demands.  The handle's staged point, its callback caches and
// its outputs are not touched: an evaluation after any of these calls returns what it returned before.
//
// Costates (pc_solution_set_multipliers): the index arithmetic is pc_costate_plan.hpp.  The multipliers belong to the
// constraint and objective scaling the handle holds when they are set, which are read then.
//
// Propagation (pc_solution_propagate, _dense, _stiff): the index arithmetic is pc_propagate_plan.hpp.  The segment list,
// the first sections and atol are staged in buffers the solution keeps, so a device call may return before the kernel
// has run; the three kernels share them, as every launch waits for the stream before it uploads
// (solution_stage_propagate).  pc_solution_propagate_dense stages integral_atol and the sorted queries the same way.
//
// Path and bound multipliers (pc_solution_set_bound_multipliers): the index arithmetic is pc_optimality_plan.hpp.  The
// solution keeps its own device copy of the constraint multipliers, the tables and the scaling they were set under, so
// this call may come any time after pc_solution_set_multipliers.
#include "pc_costate_plan.hpp"
#include "pc_optimality_plan.hpp"
#include "pc_propagate_plan.hpp"

struct pc_solution {
  pc_handle* h = nullptr;
  DevBuf<double> d_x;
  DevBuf<double> d_U;       // the C_u tables (the costate kernel forms its coefficients with them)
  DevBuf<double> d_D;       // the ydot tables (the multiplier kernel: the phase's last section)
  DevBuf<double> d_lam;     // the multiplier vector's device copy
  DevBuf<double> d_W, d_z;  // the node-weight rows of the A tables; the bound multipliers' device copy
  std::vector<int32_t> orders;   // as of pc_solution_set_multipliers
  std::vector<double> tabA;
  double wJ = 0.0;          // the objective scaling the multipliers were set under
  double int_scale = 1.0;   // pcs::integral_weight_scale of the handle's tables
  bool has_costate = false, has_optimality = false, has_z = false;
  struct Phase {
    pcs::FitPlan plan;
    DevBuf<int32_t> tile_k0, lane0;
    DevBuf<double> sec_tau, node_tau, node_t, node_y, node_u, node_f, coef_dy, coef_u;
    DevBuf<double> node_p, node_H, coef_p, nu;   // costates: allocated by pc_solution_set_multipliers
    DevBuf<double> node_mu, node_zeta, end_z, node_Hz, coef_mu, coef_zeta;   // by pc_solution_set_bound_multipliers
    hipFunction_t fn_sample_optimality = nullptr;
    PcPhaseView view_w;     // view with the constraint scaling the multipliers were set under
    DevBuf<int32_t> prop_seg, prop_sec;          // propagation, all three kernels: the staged segment list and first
    DevBuf<double> prop_atol;                    // sections, and atol
    DevBuf<int32_t> dense_order, dense_q0;       // dense propagation besides: the sorted queries, their order and slots,
    DevBuf<double> dense_iatol, dense_tau_q;     // and integral_atol
    std::vector<double> h_tau;                   // the node abscissae on the host (the queries' slots are found in them)
    hipFunction_t fn_sample = nullptr, fn_sample_costate = nullptr, fn_propagate = nullptr, fn_propagate_dense = nullptr,
                  fn_propagate_stiff = nullptr;
    PcPhaseView view;       // the phase as of creation: what sampling, the costates and propagation unscale with
    PcSolCurves curves;     // the polynomials the fit kernel made
    int NY = 0, NU = 0, NQ = 0;
  };
  std::vector<std::unique_ptr<Phase>> ph;
};

namespace {

void solution_build(pc_solution* s, int n_orders, const int32_t* orders, const double* tabD, const double* tabU,
                    const double* tau) {
  pc_handle* h = s->h;
  auto& Q = h->Q;
  if (!tabD || !tabU || !tau) throw std::runtime_error("solution: null table");
  DevBuf<double>& d_D = s->d_D;
  int32_t offC[PC_MAX_ORDER + 1];
  const int32_t tab_total = pcs::table_offsets(n_orders, orders, offC);
  d_D.upload(std::vector<double>(tabD, tabD + tab_total));
  s->d_U.upload(std::vector<double>(tabU, tabU + tab_total));
  size_t tau_off = 0;
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    auto& P = Q.ph[ip];
    auto S = std::make_unique<pc_solution::Phase>();
    S->NY = P.n_y;
    S->NU = P.n_u;
    S->NQ = P.n_q;
    S->plan = pcs::build_fit_plan(P.K, P.n_k.data(), n_orders, orders, P.n_y, P.n_u, 256, h->lds_limit);
    const pcs::FitPlan& F = S->plan;
    if (F.N != P.N) throw std::runtime_error("solution: the plan's node count differs from the handle's");
    if (F.sec_s != P.sec_s) throw std::runtime_error("solution: the plan's section starts differ from the handle's");
    S->view = fill_phase_view(h, (int)ip, s->d_x.p);
    const std::vector<double> edges = pcs::section_edges(F, tau + tau_off);
    S->tile_k0.upload(F.tile_k0);
    S->lane0.upload(F.lane0);
    S->h_tau.assign(tau + tau_off, tau + tau_off + P.N);
    S->node_tau.upload(S->h_tau);
    tau_off += (size_t)P.N;
    S->sec_tau.upload(edges);
    const size_t ny = (size_t)std::max(1, P.n_y), nu = (size_t)std::max(1, P.n_u);
    S->node_t.alloc((size_t)F.N);
    S->node_y.alloc(ny * F.N);
    S->node_u.alloc(nu * F.N);
    S->node_f.alloc(ny * F.N);
    S->coef_dy.alloc(ny * F.NC);
    S->coef_u.alloc(nu * F.NC);
    S->curves = PcSolCurves{S->sec_tau.p, S->node_y.p, S->coef_dy.p, S->coef_u.p, F.NC, 0};
    hipFunction_t fn_fit = nullptr;
    HIP_OK(find_fn(h, &fn_fit, ("pc_sol_fit_p" + std::to_string(ip)).c_str()));
    HIP_OK(find_fn(h, &S->fn_sample, ("pc_sol_sample_p" + std::to_string(ip)).c_str()));
    PcSolFitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = S->view;
    a.tau = S->node_tau.p;
    a.tile_k0 = S->tile_k0.p;
    a.lane0 = S->lane0.p;
    a.tabD = d_D.p;
    a.tabU = s->d_U.p;
    a.node_t = S->node_t.p;
    a.node_y = S->node_y.p;
    a.node_u = S->node_u.p;
    a.node_f = S->node_f.p;
    a.coef_dy = S->coef_dy.p;
    a.coef_u = S->coef_u.p;
    a.NC = F.NC;
    a.tab_total = F.tab_total;
    std::memcpy(a.offC, F.offC, sizeof(a.offC));
    launch_block(fn_fit, F.n_tiles(), F.TB, F.lds_bytes, h->stream, a);
    HIP_OK(hipStreamSynchronize(h->stream));
    s->ph.push_back(std::move(S));
  }
}

void solution_launch_sample(pc_solution* s, int phase, const double* d_t, int64_t n_t, int flags, double* d_y, double* d_dy,
                            double* d_u, double* d_f) {
  auto& S = *s->ph[phase];
  if (n_t == 0) return;
  PcSolSampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.v = S.view;
  a.c = S.curves;
  a.t = d_t;
  a.Q = n_t;
  a.flags = flags;
  a.out_y = S.NY > 0 ? d_y : nullptr;
  a.out_dy = S.NY > 0 ? d_dy : nullptr;
  a.out_u = S.NU > 0 ? d_u : nullptr;
  a.out_f = S.NY > 0 ? d_f : nullptr;
  launch_block(S.fn_sample, (unsigned)pcs::sample_blocks(n_t, 256), 256, 0, s->h->stream, a);
}

// the costates of every phase from the device vector d_lam (pc_sol_costate_p<i>), then the arguments of the sampling calls
void solution_costate(pc_solution* s, const double* d_lam, int n_orders, const int32_t* orders, const double* tabA) {
  pc_handle* h = s->h;
  auto& Q = h->Q;
  int32_t offA[PC_MAX_ORDER + 1];
  const int32_t a_total = pcs::a_table_offsets(n_orders, orders, offA);
  DevBuf<double> d_A;
  d_A.upload(std::vector<double>(tabA, tabA + a_total));
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    auto& P = Q.ph[ip];
    const std::vector<double>& scal = h->scal.phase[ip];
    auto& S = *s->ph[ip];
    const pcs::FitPlan& F = S.plan;
    const pcs::CostatePlan C =
        pcs::build_costate_plan(F, n_orders, orders, P.n_y, P.n_q, P.c_off, P.c_int_off, Q.num_c, h->lds_limit);
    if (scal.size() > PC_MAX_SCAL) throw std::runtime_error("too many scaling constants for the kernel argument block");
    const size_t ny = (size_t)std::max(1, P.n_y);
    if (!S.node_p.p) {
      S.node_p.alloc(ny * F.N);
      S.node_H.alloc((size_t)F.N);
      S.coef_p.alloc(ny * F.NC);
      S.nu.alloc((size_t)std::max(1, P.n_q));
    }
    hipFunction_t fn = nullptr;
    HIP_OK(find_fn(h, &fn, ("pc_sol_costate_p" + std::to_string(ip)).c_str()));
    HIP_OK(find_fn(h, &S.fn_sample_costate, ("pc_sol_sample_costate_p" + std::to_string(ip)).c_str()));
    PcSolCostateArgs a;
    std::memset(&a, 0, sizeof(a));
    // the variables are unscaled as the solution's node values were (the view of creation); the rows are scaled as of
    // now: the multipliers belong to the constraint scaling the handle holds when they are set (scal's tail: Wd Wp Wi)
    a.v = S.view;
    const size_t o_w = scal.size() - (size_t)(P.n_y + P.n_p + P.n_q);
    for (size_t i = o_w; i < scal.size(); ++i) a.v.scal[i] = scal[i];
    a.lam = d_lam;
    a.tile_k0 = S.tile_k0.p;
    a.lane0 = S.lane0.p;
    a.sec_tau = S.sec_tau.p;
    a.tabA = d_A.p;
    a.tabU = s->d_U.p;
    a.node_p = S.node_p.p;
    a.node_H = S.node_H.p;
    a.coef_p = S.coef_p.p;
    a.nu = S.nu.p;
    a.c_off = P.c_off;
    a.c_int_off = P.c_int_off;
    a.wJ = h->scal.wJ;
    a.NC = F.NC;
    a.tab_total = F.tab_total;
    a.a_total = a_total;
    std::memcpy(a.offC, F.offC, sizeof(a.offC));
    std::memcpy(a.offA, C.offA, sizeof(a.offA));
    launch_block(fn, F.n_tiles(), F.TB, C.lds_bytes, h->stream, a);
    S.view_w = a.v;
  }
  HIP_OK(hipStreamSynchronize(h->stream));   // d_A is released on return
  s->orders.assign(orders, orders + n_orders);
  s->tabA.assign(tabA, tabA + a_total);
  s->wJ = h->scal.wJ;
  s->has_costate = true;
  s->has_optimality = s->has_z = false;       // (they belong to the multipliers that were just replaced)
}

int solution_set_multipliers(pc_solution* s, const double* lam, int64_t n_lam, bool on_device, int n_orders, const int32_t* orders,
                             const double* tabA) {
  return guarded(g_err, [&] {
    if (!s) throw std::runtime_error("null solution");
    require_device(s->h);
    pcs::check_multiplier_args(lam, n_lam, s->h->Q.num_c, tabA, s->h->scal.wJ);
    HIP_OK(hipSetDevice(s->h->device));
    // the solution's own copy: the path multipliers are read from it later (pc_solution_set_bound_multipliers)
    if (s->d_lam.n != (size_t)n_lam) s->d_lam.alloc((size_t)n_lam);
    HIP_OK(hipMemcpyAsync(s->d_lam.p, lam, (size_t)n_lam * sizeof(double),
                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->h->stream));
    solution_costate(s, s->d_lam.p, n_orders, orders, tabA);
  });
}

void solution_launch_sample_costate(pc_solution* s, int phase, const double* d_t, int64_t n_t, int flags, double* d_p, double* d_H) {
  auto& S = *s->ph[phase];
  if (n_t == 0) return;
  PcSolCostateSampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.s.v = S.view;
  a.s.c = S.curves;
  a.s.t = d_t;
  a.s.Q = n_t;
  a.s.flags = flags;
  a.coef_p = S.coef_p.p;
  a.nu = S.nu.p;
  a.out_p = d_p;
  a.out_H = d_H;
  launch_block(S.fn_sample_costate, (unsigned)pcs::sample_blocks(n_t, 256), 256, 0, s->h->stream, a);
}

// mu, zeta and the node gradients of every phase (pc_sol_multipliers_p<i>) from the solution's multipliers and d_z (or
// null), then the arguments of the sampling call
void solution_optimality(pc_solution* s, const double* d_z) {
  pc_handle* h = s->h;
  auto& Q = h->Q;
  const int n_orders = (int)s->orders.size();
  int32_t offA[PC_MAX_ORDER + 1], offW[PC_MAX_ORDER + 1];
  (void)pcs::a_table_offsets(n_orders, s->orders.data(), offA);
  const int32_t w_total = pcs::w_table_offsets(n_orders, s->orders.data(), offW);
  s->d_W.upload(pcs::pack_weight_rows(n_orders, s->orders.data(), s->tabA.data(), offA, offW, w_total));
  s->int_scale = pcs::integral_weight_scale(n_orders, s->orders.data(), s->tabA.data(), offA, h->qw.data(), h->qw_off);
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    auto& P = Q.ph[ip];
    auto& S = *s->ph[ip];
    const pcs::FitPlan& F = S.plan;
    const pcs::OptimalityPlan O = pcs::build_optimality_plan(F, n_orders, s->orders.data(), P.n_y, P.n_u, P.n_p, P.c_path_off,
                                                             P.c_int_off, Q.num_c, P.x_off, Q.num_x, h->lds_limit);
    const size_t nz = (size_t)std::max(1, P.n_y + P.n_u), np = (size_t)std::max(1, P.n_p);
    if (!S.node_mu.p) {
      S.node_mu.alloc(np * F.N);
      S.coef_mu.alloc(np * F.NC);
      S.node_Hz.alloc(nz * F.N);
    }
    if (d_z && !S.node_zeta.p) {
      S.node_zeta.alloc(nz * F.N);
      S.coef_zeta.alloc(nz * F.NC);
      S.end_z.alloc(2 * (size_t)std::max(1, P.n_y));
    }
    hipFunction_t fn = nullptr;
    HIP_OK(find_fn(h, &fn, ("pc_sol_multipliers_p" + std::to_string(ip)).c_str()));
    HIP_OK(find_fn(h, &S.fn_sample_optimality, ("pc_sol_sample_optimality_p" + std::to_string(ip)).c_str()));
    PcSolMultiplierArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = S.view_w;
    a.lam = s->d_lam.p;
    a.z = d_z;
    a.tile_k0 = S.tile_k0.p;
    a.lane0 = S.lane0.p;
    a.sec_tau = S.sec_tau.p;
    a.tabW = s->d_W.p;
    a.tabU = s->d_U.p;
    a.tabD = s->d_D.p;
    a.node_p = S.node_p.p;
    a.nu = S.nu.p;
    a.node_mu = S.node_mu.p;
    a.node_zeta = S.node_zeta.p;
    a.end_z = S.end_z.p;
    a.node_Hz = S.node_Hz.p;
    a.coef_mu = S.coef_mu.p;
    a.coef_zeta = S.coef_zeta.p;
    a.c_path_off = P.c_path_off;
    a.wJ = s->wJ;
    a.int_scale = s->int_scale;
    a.NC = F.NC;
    a.tab_total = F.tab_total;
    a.w_total = w_total;
    std::memcpy(a.offC, F.offC, sizeof(a.offC));
    std::memcpy(a.offW, O.offW, sizeof(a.offW));
    launch_block(fn, F.n_tiles(), F.TB, O.lds_bytes, h->stream, a);
  }
  HIP_OK(hipStreamSynchronize(h->stream));   // a caller's device vector is free again
  s->has_optimality = true;
  s->has_z = d_z != nullptr;
}

int solution_set_bound_multipliers(pc_solution* s, const double* z, int64_t n_z, bool on_device) {
  return guarded(g_err, [&] {
    if (!s) throw std::runtime_error("null solution");
    require_device(s->h);
    pcs::check_bound_multiplier_args(s->has_costate, z, n_z, s->h->Q.num_x);
    HIP_OK(hipSetDevice(s->h->device));
    const double* d_z = z;
    if (z && !on_device) {
      if (s->d_z.n != (size_t)n_z) s->d_z.alloc((size_t)n_z);
      HIP_OK(hipMemcpyAsync(s->d_z.p, z, (size_t)n_z * sizeof(double), hipMemcpyHostToDevice, s->h->stream));
      d_z = s->d_z.p;
    }
    solution_optimality(s, d_z);
  });
}

void solution_launch_sample_optimality(pc_solution* s, int phase, const double* d_t, int64_t n_t, int flags, double* d_Hy,
                                       double* d_Hu, double* d_dp, double* d_mu, double* d_zeta) {
  auto& S = *s->ph[phase];
  if (n_t == 0) return;
  PcSolOptimalitySampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.s.v = S.view;
  a.s.c = S.curves;
  a.s.t = d_t;
  a.s.Q = n_t;
  a.s.flags = flags;
  a.coef_p = S.coef_p.p;
  a.nu = S.nu.p;
  a.coef_mu = S.coef_mu.p;
  a.coef_zeta = s->has_z ? S.coef_zeta.p : nullptr;
  a.int_scale = s->int_scale;
  a.out_Hy = d_Hy;
  a.out_Hu = d_Hu;
  a.out_dp = d_dp;
  a.out_mu = d_mu;
  a.out_zeta = d_zeta;
  launch_block(S.fn_sample_optimality, (unsigned)pcs::sample_blocks(n_t, 256), 256, 0, s->h->stream, a);
}

int solution_create(pc_handle* h, const double* x, bool x_on_device, int n_orders, const int32_t* orders, const double* tabD,
                    const double* tabU, const double* tau, pc_solution** out) {
  return guarded(g_err, [&] {
    require_device(h);
    if (!x || !out) throw std::runtime_error("solution: null argument");
    *out = nullptr;
    auto s = std::make_unique<pc_solution>();
    s->h = h;
    s->d_x.alloc((size_t)h->Q.num_x);
    HIP_OK(hipMemcpyAsync(s->d_x.p, x, h->Q.num_x * sizeof(double), x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    solution_build(s.get(), n_orders, orders, tabD, tabU, tau);
    *out = s.release();
  });
}

pc_solution::Phase& solution_phase(pc_solution* s, int phase) {
  if (!s) throw std::runtime_error("null solution");
  if (phase < 0 || phase >= (int)s->ph.size()) throw std::runtime_error("solution: phase out of range");
  HIP_OK(hipSetDevice(s->h->device));
  return *s->ph[phase];
}

// The four outputs every propagation kernel has
struct PropOutputs {
  double* y;
  int32_t *acc, *rej, *status;
};

// What the three propagation launches share once their checks are through and the plan P is made: the kernel (found
// once), the wait for the stream (an earlier call may still read the staged lists), the staged lists and the prefix of
// the argument block.
void solution_stage_propagate(pc_solution* s, int phase, const pcs::PropagatePlan& P, hipFunction_t* fn, const char* kernel,
                              int64_t substeps, double rtol, const double* atol, int64_t max_steps, const PropOutputs& o,
                              PcSolPropCommon& p) {
  auto& S = *s->ph[phase];
  if (!*fn) HIP_OK(find_fn(s->h, fn, (kernel + std::to_string(phase)).c_str()));
  HIP_OK(hipStreamSynchronize(s->h->stream));
  S.prop_seg.upload(P.seg_node);
  S.prop_sec.upload(P.seg_sec);
  S.prop_atol.upload(std::vector<double>(atol, atol + S.NY));
  p.v = S.view;
  p.c = S.curves;
  p.tau = S.node_tau.p;
  p.seg_node = S.prop_seg.p;
  p.seg_sec = S.prop_sec.p;
  p.atol = S.prop_atol.p;
  p.y_arrive = o.y;
  p.accepted = o.acc;
  p.rejected = o.rej;
  p.seg_status = o.status;
  p.rtol = rtol;
  p.n_seg = P.n_seg;
  p.substeps = (int32_t)substeps;
  p.max_steps = (int32_t)max_steps;
}

// pc_sol_propagate_p<phase> on the handle's stream; the outputs are device arrays ([n_y][N], [N], [N], [n_seg])
void solution_launch_propagate(pc_solution* s, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps, double rtol,
                               const double* atol, int64_t max_steps, double* d_y, int32_t* d_acc, int32_t* d_rej, int32_t* d_status) {
  auto& S = *s->ph[phase];
  pcs::check_propagate_tolerances(substeps, rtol, atol, S.NY, max_steps);
  const pcs::PropagatePlan P = pcs::build_propagate_plan(S.plan, n_seg, seg_nodes);
  if (!d_acc || !d_rej || !d_status || (S.NY > 0 && !d_y)) throw std::runtime_error("propagate: null output");
  PcSolPropagateArgs a;
  std::memset(&a, 0, sizeof(a));
  solution_stage_propagate(s, phase, P, &S.fn_propagate, "pc_sol_propagate_p", substeps, rtol, atol, max_steps,
                           {d_y, d_acc, d_rej, d_status}, a.p);
  launch_block(S.fn_propagate, (unsigned)P.blocks, (unsigned)P.TB, 0, s->h->stream, a);
}

// pc_sol_propagate_stiff_p<phase> on the handle's stream; the outputs are device arrays ([n_y][N], [N], [N], [n_seg],
// [N], [N])
void solution_launch_propagate_stiff(pc_solution* s, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps,
                                     double rtol, const double* atol, int64_t max_steps, int64_t newton_max, double* d_y,
                                     int32_t* d_acc, int32_t* d_rej, int32_t* d_status, int32_t* d_newton_rej,
                                     int32_t* d_newton_it) {
  auto& S = *s->ph[phase];
  pcs::check_propagate_stiff_options(substeps, rtol, atol, S.NY, max_steps, newton_max);
  const pcs::PropagatePlan P = pcs::build_propagate_plan(S.plan, n_seg, seg_nodes);
  if (!d_acc || !d_rej || !d_status || !d_newton_rej || !d_newton_it || (S.NY > 0 && !d_y))
    throw std::runtime_error("propagate: null output");
  PcSolPropagateStiffArgs a;
  std::memset(&a, 0, sizeof(a));
  solution_stage_propagate(s, phase, P, &S.fn_propagate_stiff, "pc_sol_propagate_stiff_p", substeps, rtol, atol, max_steps,
                           {d_y, d_acc, d_rej, d_status}, a.p);
  a.newton_rejected = d_newton_rej;
  a.newton_iterations = d_newton_it;
  a.newton_max = (int32_t)newton_max;
  launch_block(S.fn_propagate_stiff, (unsigned)P.blocks, (unsigned)P.TB, 0, s->h->stream, a);
}

// pc_sol_propagate_dense_p<phase> on the handle's stream; the outputs are device arrays ([n_y][N], [N], [N], [n_seg],
// [n_q][N], [n_y][n_query], [n_q][n_query]); the queries are tau, a host array
void solution_launch_propagate_dense(pc_solution* s, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps,
                                     double rtol, const double* atol, const double* integral_atol, int64_t max_steps,
                                     int64_t n_query, const double* tau_q, double* d_y, int32_t* d_acc, int32_t* d_rej,
                                     int32_t* d_status, double* d_q, double* d_yd, double* d_qd) {
  auto& S = *s->ph[phase];
  pcs::check_propagate_tolerances(substeps, rtol, atol, S.NY, max_steps);
  pcs::check_integral_atol(integral_atol, S.NQ);
  const pcs::PropagatePlan P = pcs::build_propagate_plan(S.plan, n_seg, seg_nodes);
  const pcs::DenseQueryPlan D = pcs::build_dense_query_plan(S.plan.N, S.h_tau.data(), n_query, tau_q);
  if (!d_acc || !d_rej || !d_status || (S.NY > 0 && !d_y) || (S.NQ > 0 && !d_q) ||
      (D.Q > 0 && ((S.NY > 0 && !d_yd) || (S.NQ > 0 && !d_qd))))
    throw std::runtime_error("propagate: null output");
  PcSolPropagateDenseArgs a;
  std::memset(&a, 0, sizeof(a));
  solution_stage_propagate(s, phase, P, &S.fn_propagate_dense, "pc_sol_propagate_dense_p", substeps, rtol, atol, max_steps,
                           {d_y, d_acc, d_rej, d_status}, a.p);
  if (integral_atol) S.dense_iatol.upload(std::vector<double>(integral_atol, integral_atol + S.NQ));
  S.dense_tau_q.upload(D.tau_sorted);
  S.dense_order.upload(D.q_order);
  S.dense_q0.upload(D.node_q0);
  a.integral_atol = integral_atol && S.NQ > 0 ? S.dense_iatol.p : nullptr;
  a.tau_q = S.dense_tau_q.p;
  a.q_order = S.dense_order.p;
  a.node_q0 = S.dense_q0.p;
  a.q_arrive = d_q;
  a.y_dense = d_yd;
  a.q_dense = d_qd;
  a.Q = D.Q;
  launch_block(S.fn_propagate_dense, (unsigned)P.blocks, (unsigned)P.TB, 0, s->h->stream, a);
}

pc_solution::Phase& solution_costate_phase(pc_solution* s, int phase) {
  auto& S = solution_phase(s, phase);
  if (!s->has_costate) throw std::runtime_error("solution: no multipliers were set");
  return S;
}

void solution_down(double* dst, const DevBuf<double>& src, size_t count) {
  if (dst && count) HIP_OK(hipMemcpy(dst, src.p, count * sizeof(double), hipMemcpyDeviceToHost));
}

void check_segment_count(const pc_solution::Phase& S, int64_t n_seg) {
  if (n_seg < 1 || n_seg > (int64_t)S.plan.N - 1) throw std::runtime_error("propagate: the number of segments must be in [1, N - 1]");
}

// The host-pointer variant of a propagation call, behind the caller's checks: the device arrays of the four outputs every
// method has, launch (on them and on the caller's further arrays), the wait for the stream and the copies down of the
// four.  The caller copies its further outputs down behind it.
template <class Launch>
void solution_propagate_to_host(pc_solution* sol, pc_solution::Phase& S, int64_t n_seg, double* y_arrive, int32_t* accepted,
                                int32_t* rejected, int32_t* seg_status, Launch launch) {
  const size_t N = (size_t)S.plan.N;
  DevBuf<double> d_y;
  DevBuf<int32_t> d_acc, d_rej, d_st;
  d_y.alloc(N * (size_t)std::max(1, S.NY));
  d_acc.alloc(N);
  d_rej.alloc(N);
  d_st.alloc((size_t)n_seg);
  launch(d_y.p, d_acc.p, d_rej.p, d_st.p);
  HIP_OK(hipStreamSynchronize(sol->h->stream));
  solution_down(y_arrive, d_y, N * S.NY);
  HIP_OK(hipMemcpy(accepted, d_acc.p, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(rejected, d_rej.p, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(seg_status, d_st.p, (size_t)n_seg * sizeof(int32_t), hipMemcpyDeviceToHost));
}

pc_solution::Phase& solution_optimality_phase(pc_solution* s, int phase) {
  auto& S = solution_phase(s, phase);
  if (!s->has_optimality) throw std::runtime_error("optimality: pc_solution_set_bound_multipliers has not run");
  return S;
}

}  // namespace

extern "C" {

int pc_solution_create(pc_handle* h, const double* x, int n_orders, const int32_t* orders, const double* tabD,
                       const double* tabU, const double* tau, pc_solution** sol) {
  return solution_create(h, x, false, n_orders, orders, tabD, tabU, tau, sol);
}

int pc_solution_create_device(pc_handle* h, const double* d_x, int n_orders, const int32_t* orders, const double* tabD,
                              const double* tabU, const double* tau, pc_solution** sol) {
  return solution_create(h, d_x, true, n_orders, orders, tabD, tabU, tau, sol);
}

void pc_solution_destroy(pc_solution* sol) {
  if (!sol) return;
  (void)hipSetDevice(sol->h->device);
  (void)hipStreamSynchronize(sol->h->stream);
  delete sol;
}

int pc_solution_sizes(pc_solution* sol, int phase, int32_t* N, int32_t* K, int32_t* NC, int32_t* n_y, int32_t* n_u) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    if (N) *N = S.plan.N;
    if (K) *K = S.plan.K;
    if (NC) *NC = S.plan.NC;
    if (n_y) *n_y = S.NY;
    if (n_u) *n_u = S.NU;
  });
}

int pc_solution_nodes(pc_solution* sol, int phase, double* time, double* y, double* dy, double* u) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    const size_t N = (size_t)S.plan.N;
    solution_down(time, S.node_t, N);
    solution_down(y, S.node_y, N * S.NY);
    solution_down(dy, S.node_f, N * S.NY);
    solution_down(u, S.node_u, N * S.NU);
  });
}

int pc_solution_coefficients(pc_solution* sol, int phase, double* dy_coef, double* u_coef) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    solution_down(dy_coef, S.coef_dy, (size_t)S.plan.NC * S.NY);
    solution_down(u_coef, S.coef_u, (size_t)S.plan.NC * S.NU);
  });
}

int pc_solution_sample(pc_solution* sol, int phase, const double* t, int64_t n_t, int flags, double* y, double* dy, double* u,
                       double* f) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, t, n_t, flags);
    auto& S = solution_phase(sol, phase);
    if (n_t == 0) return;
    const size_t Qn = (size_t)n_t;
    DevBuf<double> d_t, d_y, d_dy, d_u, d_f;
    d_t.upload(std::vector<double>(t, t + Qn));
    if (y && S.NY) d_y.alloc(Qn * S.NY);
    if (dy && S.NY) d_dy.alloc(Qn * S.NY);
    if (u && S.NU) d_u.alloc(Qn * S.NU);
    if (f && S.NY) d_f.alloc(Qn * S.NY);
    solution_launch_sample(sol, phase, d_t.p, n_t, flags, d_y.p, d_dy.p, d_u.p, d_f.p);
    HIP_OK(hipStreamSynchronize(sol->h->stream));
    if (d_y.p) solution_down(y, d_y, Qn * S.NY);
    if (d_dy.p) solution_down(dy, d_dy, Qn * S.NY);
    if (d_u.p) solution_down(u, d_u, Qn * S.NU);
    if (d_f.p) solution_down(f, d_f, Qn * S.NY);
  });
}

int pc_solution_sample_device(pc_solution* sol, int phase, const double* d_t, int64_t n_t, int flags, double* d_y, double* d_dy,
                              double* d_u, double* d_f) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, d_t, n_t, flags);
    (void)solution_phase(sol, phase);
    solution_launch_sample(sol, phase, d_t, n_t, flags, d_y, d_dy, d_u, d_f);
  });
}

int pc_solution_set_multipliers(pc_solution* sol, const double* lam, int64_t n_lam, int n_orders, const int32_t* orders,
                                const double* tabA) {
  return solution_set_multipliers(sol, lam, n_lam, false, n_orders, orders, tabA);
}

int pc_solution_set_multipliers_device(pc_solution* sol, const double* d_lam, int64_t n_lam, int n_orders, const int32_t* orders,
                                       const double* tabA) {
  return solution_set_multipliers(sol, d_lam, n_lam, true, n_orders, orders, tabA);
}

int pc_solution_costate_nodes(pc_solution* sol, int phase, double* p, double* H, double* nu) {
  return guarded(g_err, [&] {
    auto& S = solution_costate_phase(sol, phase);
    const size_t N = (size_t)S.plan.N;
    solution_down(p, S.node_p, N * S.NY);
    solution_down(H, S.node_H, N);
    solution_down(nu, S.nu, (size_t)S.NQ);
  });
}

int pc_solution_costate_coefficients(pc_solution* sol, int phase, double* p_coef) {
  return guarded(g_err, [&] {
    auto& S = solution_costate_phase(sol, phase);
    solution_down(p_coef, S.coef_p, (size_t)S.plan.NC * S.NY);
  });
}

int pc_solution_sample_costate(pc_solution* sol, int phase, const double* t, int64_t n_t, int flags, double* p, double* H) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, t, n_t, flags);
    auto& S = solution_costate_phase(sol, phase);
    if (n_t == 0) return;
    const size_t Qn = (size_t)n_t;
    DevBuf<double> d_t, d_p, d_H;
    d_t.upload(std::vector<double>(t, t + Qn));
    d_p.alloc(Qn * (size_t)std::max(1, S.NY));
    d_H.alloc(Qn);
    solution_launch_sample_costate(sol, phase, d_t.p, n_t, flags, d_p.p, d_H.p);
    HIP_OK(hipStreamSynchronize(sol->h->stream));
    solution_down(p, d_p, Qn * S.NY);
    solution_down(H, d_H, Qn);
  });
}

int pc_solution_sample_costate_device(pc_solution* sol, int phase, const double* d_t, int64_t n_t, int flags, double* d_p,
                                      double* d_H) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, d_t, n_t, flags);
    auto& S = solution_costate_phase(sol, phase);
    if (n_t > 0 && (!d_H || (S.NY > 0 && !d_p))) throw std::runtime_error("solution: null output");
    solution_launch_sample_costate(sol, phase, d_t, n_t, flags, d_p, d_H);
  });
}

int pc_solution_set_bound_multipliers(pc_solution* sol, const double* z, int64_t n_z) {
  return solution_set_bound_multipliers(sol, z, n_z, false);
}

int pc_solution_set_bound_multipliers_device(pc_solution* sol, const double* d_z, int64_t n_z) {
  return solution_set_bound_multipliers(sol, d_z, n_z, true);
}

int pc_solution_multiplier_nodes(pc_solution* sol, int phase, double* mu, double* zeta, double* end_z, double* H_y, double* H_u) {
  return guarded(g_err, [&] {
    auto& S = solution_optimality_phase(sol, phase);
    const size_t N = (size_t)S.plan.N, NP = (size_t)sol->h->Q.ph[(size_t)phase].n_p;
    if ((zeta || end_z) && !sol->has_z) throw std::runtime_error("optimality: no bound multipliers were given");
    solution_down(mu, S.node_mu, N * NP);
    solution_down(zeta, S.node_zeta, N * (size_t)(S.NY + S.NU));
    solution_down(end_z, S.end_z, 2 * (size_t)S.NY);
    solution_down(H_y, S.node_Hz, N * S.NY);
    if (H_u && S.NU) HIP_OK(hipMemcpy(H_u, S.node_Hz.p + N * S.NY, N * S.NU * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int pc_solution_defect_multipliers(pc_solution* sol, int phase, double* Lam) {
  return guarded(g_err, [&] {
    auto& S = solution_costate_phase(sol, phase);
    const auto& P = sol->h->Q.ph[(size_t)phase];
    const size_t rows = (size_t)S.plan.N - 1, o_wd = sol->h->scal.phase[(size_t)phase].size() - (size_t)(P.n_y + P.n_p + P.n_q);
    if (!Lam || !S.NY) return;
    HIP_OK(hipMemcpy(Lam, sol->d_lam.p + P.c_off, rows * S.NY * sizeof(double), hipMemcpyDeviceToHost));
    for (int a = 0; a < S.NY; ++a)   // (the operation order of pc_sol_costate)
      for (size_t r = 0; r < rows; ++r) Lam[(size_t)a * rows + r] = S.view_w.scal[o_wd + (size_t)a] * Lam[(size_t)a * rows + r] / sol->wJ;
  });
}

int pc_solution_multiplier_coefficients(pc_solution* sol, int phase, double* mu_coef, double* zeta_coef) {
  return guarded(g_err, [&] {
    auto& S = solution_optimality_phase(sol, phase);
    if (zeta_coef && !sol->has_z) throw std::runtime_error("optimality: no bound multipliers were given");
    solution_down(mu_coef, S.coef_mu, (size_t)S.plan.NC * (size_t)sol->h->Q.ph[(size_t)phase].n_p);
    solution_down(zeta_coef, S.coef_zeta, (size_t)S.plan.NC * (size_t)(S.NY + S.NU));
  });
}

int pc_solution_sample_optimality(pc_solution* sol, int phase, const double* t, int64_t n_t, int flags, double* H_y, double* H_u,
                                  double* dp, double* mu, double* zeta) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, t, n_t, flags);
    auto& S = solution_optimality_phase(sol, phase);
    if (n_t == 0) return;
    const size_t Qn = (size_t)n_t, NP = (size_t)sol->h->Q.ph[(size_t)phase].n_p, NZ = (size_t)(S.NY + S.NU);
    DevBuf<double> d_t, d_Hy, d_Hu, d_dp, d_mu, d_zeta;
    d_t.upload(std::vector<double>(t, t + Qn));
    d_Hy.alloc(Qn * (size_t)std::max(1, S.NY));
    d_Hu.alloc(Qn * (size_t)std::max(1, S.NU));
    d_dp.alloc(Qn * (size_t)std::max(1, S.NY));
    d_mu.alloc(Qn * std::max<size_t>(1, NP));
    d_zeta.alloc(Qn * std::max<size_t>(1, NZ));
    solution_launch_sample_optimality(sol, phase, d_t.p, n_t, flags, d_Hy.p, d_Hu.p, d_dp.p, d_mu.p, d_zeta.p);
    HIP_OK(hipStreamSynchronize(sol->h->stream));
    solution_down(H_y, d_Hy, Qn * S.NY);
    solution_down(H_u, d_Hu, Qn * S.NU);
    solution_down(dp, d_dp, Qn * S.NY);
    solution_down(mu, d_mu, Qn * NP);
    if (sol->has_z) solution_down(zeta, d_zeta, Qn * NZ);
  });
}

int pc_solution_sample_optimality_device(pc_solution* sol, int phase, const double* d_t, int64_t n_t, int flags, double* d_H_y,
                                         double* d_H_u, double* d_dp, double* d_mu, double* d_zeta) {
  return guarded(g_err, [&] {
    if (!sol) throw std::runtime_error("null solution");
    pcs::check_sample_args((int)sol->ph.size(), phase, d_t, n_t, flags);
    auto& S = solution_optimality_phase(sol, phase);
    const int NP = sol->h->Q.ph[(size_t)phase].n_p;
    if (n_t > 0 && ((S.NY > 0 && (!d_H_y || !d_dp)) || (S.NU > 0 && !d_H_u) || (NP > 0 && !d_mu) ||
                    (sol->has_z && S.NY + S.NU > 0 && !d_zeta)))
      throw std::runtime_error("optimality: null output");
    solution_launch_sample_optimality(sol, phase, d_t, n_t, flags, d_H_y, d_H_u, d_dp, d_mu, d_zeta);
  });
}

int pc_solution_propagate(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps, double rtol,
                          const double* atol, int64_t max_steps, double* y_arrive, int32_t* accepted, int32_t* rejected,
                          int32_t* seg_status) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    if (!accepted || !rejected || !seg_status || (S.NY > 0 && !y_arrive)) throw std::runtime_error("propagate: null output");
    check_segment_count(S, n_seg);
    solution_propagate_to_host(sol, S, n_seg, y_arrive, accepted, rejected, seg_status,
                               [&](double* d_y, int32_t* d_acc, int32_t* d_rej, int32_t* d_st) {
                                 solution_launch_propagate(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, max_steps, d_y, d_acc,
                                                           d_rej, d_st);
                               });
  });
}

int pc_solution_propagate_device(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps, double rtol,
                                 const double* atol, int64_t max_steps, double* d_y_arrive, int32_t* d_accepted,
                                 int32_t* d_rejected, int32_t* d_seg_status) {
  return guarded(g_err, [&] {
    (void)solution_phase(sol, phase);
    solution_launch_propagate(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, max_steps, d_y_arrive, d_accepted, d_rejected,
                              d_seg_status);
  });
}

int pc_solution_propagate_stiff(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps, double rtol,
                                const double* atol, int64_t max_steps, int64_t newton_max, double* y_arrive, int32_t* accepted,
                                int32_t* rejected, int32_t* seg_status, int32_t* newton_rejected, int32_t* newton_iterations) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    if (!accepted || !rejected || !seg_status || !newton_rejected || !newton_iterations || (S.NY > 0 && !y_arrive))
      throw std::runtime_error("propagate: null output");
    check_segment_count(S, n_seg);
    const size_t N = (size_t)S.plan.N;
    DevBuf<int32_t> d_nr, d_ni;
    d_nr.alloc(N);
    d_ni.alloc(N);
    solution_propagate_to_host(sol, S, n_seg, y_arrive, accepted, rejected, seg_status,
                               [&](double* d_y, int32_t* d_acc, int32_t* d_rej, int32_t* d_st) {
                                 solution_launch_propagate_stiff(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, max_steps,
                                                                 newton_max, d_y, d_acc, d_rej, d_st, d_nr.p, d_ni.p);
                               });
    HIP_OK(hipMemcpy(newton_rejected, d_nr.p, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(newton_iterations, d_ni.p, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

int pc_solution_propagate_stiff_device(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps,
                                       double rtol, const double* atol, int64_t max_steps, int64_t newton_max, double* d_y_arrive,
                                       int32_t* d_accepted, int32_t* d_rejected, int32_t* d_seg_status,
                                       int32_t* d_newton_rejected, int32_t* d_newton_iterations) {
  return guarded(g_err, [&] {
    (void)solution_phase(sol, phase);
    solution_launch_propagate_stiff(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, max_steps, newton_max, d_y_arrive,
                                    d_accepted, d_rejected, d_seg_status, d_newton_rejected, d_newton_iterations);
  });
}

int pc_solution_propagate_dense(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps, double rtol,
                                const double* atol, const double* integral_atol, int64_t max_steps, int64_t n_query,
                                const double* tau_q, double* y_arrive, int32_t* accepted, int32_t* rejected, int32_t* seg_status,
                                double* q_arrive, double* y_dense, double* q_dense) {
  return guarded(g_err, [&] {
    auto& S = solution_phase(sol, phase);
    if (!accepted || !rejected || !seg_status || (S.NY > 0 && !y_arrive) || (S.NQ > 0 && !q_arrive) ||
        (n_query > 0 && ((S.NY > 0 && !y_dense) || (S.NQ > 0 && !q_dense))))
      throw std::runtime_error("propagate: null output");
    check_segment_count(S, n_seg);
    if (n_query < 0 || n_query > (int64_t)INT32_MAX) throw std::runtime_error("propagate: the number of queries must be in [0, 2^31)");
    const size_t N = (size_t)S.plan.N, Qn = (size_t)n_query;
    DevBuf<double> d_q, d_yd, d_qd;
    d_q.alloc(N * (size_t)std::max(1, S.NQ));
    d_yd.alloc(Qn * (size_t)S.NY);
    d_qd.alloc(Qn * (size_t)S.NQ);
    solution_propagate_to_host(sol, S, n_seg, y_arrive, accepted, rejected, seg_status,
                               [&](double* d_y, int32_t* d_acc, int32_t* d_rej, int32_t* d_st) {
                                 solution_launch_propagate_dense(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, integral_atol,
                                                                 max_steps, n_query, tau_q, d_y, d_acc, d_rej, d_st, d_q.p, d_yd.p,
                                                                 d_qd.p);
                               });
    solution_down(q_arrive, d_q, N * S.NQ);
    solution_down(y_dense, d_yd, Qn * S.NY);
    solution_down(q_dense, d_qd, Qn * S.NQ);
  });
}

int pc_solution_propagate_dense_device(pc_solution* sol, int phase, int64_t n_seg, const int32_t* seg_nodes, int64_t substeps,
                                       double rtol, const double* atol, const double* integral_atol, int64_t max_steps,
                                       int64_t n_query, const double* tau_q, double* d_y_arrive, int32_t* d_accepted,
                                       int32_t* d_rejected, int32_t* d_seg_status, double* d_q_arrive, double* d_y_dense,
                                       double* d_q_dense) {
  return guarded(g_err, [&] {
    (void)solution_phase(sol, phase);
    solution_launch_propagate_dense(sol, phase, n_seg, seg_nodes, substeps, rtol, atol, integral_atol, max_steps, n_query, tau_q,
                                    d_y_arrive, d_accepted, d_rejected, d_seg_status, d_q_arrive, d_y_dense, d_q_dense);
  });
}

}  // extern "C"
