// C-ABI engine: owns device memory, the per-problem code object and the launch sequence.
// See include/pycollo_amd.h for the contract and the reference interfaces each entry point replaces.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pycollo_amd.h"
#include "pc_args.h"
#include "pc_host.hpp"
#include "pc_pattern.hpp"
#include "pc_desc.hpp"
#include "pc_eval_shape.hpp"
#include "pc_eval_launch.hpp"
#include "pc_callback_cache.hpp"
#include "pc_deriv.hpp"
#include "pc_solution_plan.hpp"

struct pc_deriv_dev;   // (pc_deriv_check.hpp: the derivative check's device buffers)
struct pc_kkt;   // (pc_kkt.hip; the interior-point state below drives it through the exported calls)

namespace {

thread_local std::string g_err;

void set_err(const std::string& s) { g_err = s; }

// what the device holds for a phase
struct PhaseDev {
  DevBuf<int32_t> tile_k0, tile_n0, sec_s;
  DevBuf<double> sec_h, scal, partials, tab;
  DevBuf<int64_t> sec_E, hslot0, hslotN, hsum_slot;
  DevBuf<int32_t> hsum_local;
  DevBuf<unsigned long long> gran;   // resident tail: the per-tile partial sums as granules, [n_tiles][nred][2]
  hipFunction_t fn = nullptr;        // the phase's bulk kernel (pcl::BULK)
};

// generic kernel: 2-norm of every CSR row (scaling.py:392-395 without densifying)
__global__ void row_norms_kernel(const int64_t* __restrict__ indptr, const double* __restrict__ val,
                                 double* __restrict__ out, int64_t m) {
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= m) return;
  double acc = 0.0;
  for (int64_t i = indptr[wave] + lane; i < indptr[wave + 1]; i += 64) acc += val[i] * val[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) out[wave] = sqrt(acc);
}

// generic kernel: piecewise-linear interpolation of every row of vals_prev[n_vars][n_prev] from the
// abscissae tau_prev onto tau_new, extrapolating with the end segments -- the arithmetic of
// scipy.interpolate.interp1d(kind="linear", fill_value="extrapolate") that the reference uses to carry a
// guess / solution to the next mesh (pycollo/iteration.py:96-137): slope * (x - x_lo) + y_lo.
__global__ void interp_linear_kernel(const double* __restrict__ tau_prev, int n_prev, const double* __restrict__ vals_prev,
                                     int n_vars, const double* __restrict__ tau_new, int n_new, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_new) return;
  const double x = tau_new[i];
  // searchsorted(tau_prev, x, side="left") clipped to [1, n_prev-1]
  int lo = 0, hi = n_prev;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tau_prev[mid] < x) lo = mid + 1; else hi = mid;
  }
  int idx = lo < 1 ? 1 : (lo > n_prev - 1 ? n_prev - 1 : lo);
  const double x_lo = tau_prev[idx - 1], x_hi = tau_prev[idx];
  for (int v = 0; v < n_vars; ++v) {
    const double y_lo = vals_prev[(size_t)v * n_prev + idx - 1], y_hi = vals_prev[(size_t)v * n_prev + idx];
    const double slope = (y_hi - y_lo) / (x_hi - x_lo);
    out[(size_t)v * n_new + i] = slope * (x - x_lo) + y_lo;
  }
}

// Copy a list of contiguous runs between two device buffers: the pack / unpack step around the all-gather of the
// section-sharded evaluation (one rank's share of c~, G~, H~ is a handful of CSR runs per state / variable).
// One workgroup per chunk of at most PC_RUN_CHUNK doubles; chunks[3*i .. 3*i+2] = (src offset, dst offset, length).
#define PC_RUN_CHUNK 2048
__global__ void copy_runs_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                 const int64_t* __restrict__ chunks) {
  const int64_t so = chunks[3 * (int64_t)blockIdx.x], d0 = chunks[3 * (int64_t)blockIdx.x + 1];
  const int len = (int)chunks[3 * (int64_t)blockIdx.x + 2];
  for (int i = threadIdx.x; i < len; i += blockDim.x) dst[d0 + i] = src[so + i];
}

}  // namespace

struct pc_handle : pce::Shape {   // the launch shape pc_create decided (pc_eval_shape.hpp), and what runs it
  pcp::Problem Q;
  int device = -1;
  bool scaling_set = false;
  std::vector<double> qa, qw;   // quadrature tables
  // device
  hipStream_t stream = nullptr;
  hipModule_t module = nullptr;
  std::vector<hipModule_t> more_modules;   // a heavy model's code object comes in parts (<base>.p<k>.hsaco, codegen.n_parts)
  // what the kernels are handed and how they are launched (pc_eval_launch.hpp)
  hipFunction_t fn[pcl::N_KERNELS] = {};   // the kernels of the code object but the phases' own (PhaseDev::fn); null: absent
  pcl::Have have;                          // ... which of them a plan may name
  pcl::Range rg[PC_MAX_PHASES];            // launched tile range and caller-owned partial-sum buffer of every phase
  pcl::Scaling scal;                       // host copies of the scaling: it travels by value in the argument blocks
  pcl::Blocks blocks;                      // the argument blocks, kept filled between calls
  bool blocks_dirty = true;                // scaling / tile range / partials buffer changed since they were built
  DevBuf<char> d_phase_args;               // [n_phases] PcPhaseArgs read by pc_bulk_all: copy of blocks.merged
  DevBuf<PcTileRec> d_trec;                // records of the launched tile ranges, in launch order
  std::vector<std::unique_ptr<PhaseDev>> pd;
  DevBuf<double> d_qa, d_pointV, d_pointr, d_Wend, d_norms;
  // the packed input and output blocks (Shape::o_lam ...), pinned on the host and mirrored on the device: one copy
  // up, one copy down
  DevBuf<double> d_in, d_out;
  PinBuf<double> h_in, h_out;
  pcc::Cache cache;   // what the blocks hold for the host-pointer callbacks, the host mode and the prefetch setting
  hipEvent_t ev_small = nullptr, ev_G = nullptr;               // completion of [J | grad | c~] and of G~ at the cached x
  DevBuf<int64_t> d_point_x, d_tail_owned, d_pt_hslot, d_g_indptr;
  DevBuf<int32_t> d_pt_hlocal;
  // resident tail (pc_kernels.hpp, RES): one launch per evaluation, the tail runs as block 0 beside the tiles
  DevBuf<unsigned long long> d_erec;         // granules of the edge-node Hessian entries endpoint terms are added to
  DevBuf<int64_t> d_rec_slot;                // [n_rec] H slot of every record (-1: site absent)
  DevBuf<int32_t> d_rec_term;                // [n_rec] endpoint Hessian entry added to the record, or -1
  PinBuf<unsigned> h_timeout;                // host-visible: set by a tail whose granules never arrived
  int spin_us = 500;                         // host-pointer calls poll the stream this long before blocking (PYCOLLO_AMD_SPIN_US)
  DevBuf<unsigned long long> d_hb_gran;      // endpoint Hessian terms handed between the tail's workgroups
  PinBuf<double> h_norms;
  std::vector<double> V_ocp, r_ocp, W_ocp;
  int n_launches = 0;
  int last_launch = 0;                       // pc_info.last_launch: the builds the last evaluation launched
  // derivative check (pc_deriv.hpp, pc_deriv_check.hpp): colouring plan and scratch, built on first use
  mutable std::shared_ptr<pcd::Plan> deriv_plan;
  std::shared_ptr<pc_deriv_dev> deriv_dev;
};

namespace {

// one kernel whose parameters are the argument block `args` of `bytes` bytes, passed by value
void launch_block(hipFunction_t fn, unsigned grid, unsigned block, size_t lds, hipStream_t stream, void* args, size_t bytes) {
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
  HIP_OK(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, (unsigned)lds, stream, nullptr, cfg));
}
template <class Args>
void launch_block(hipFunction_t fn, unsigned grid, unsigned block, size_t lds, hipStream_t stream, Args& args) {
  launch_block(fn, grid, block, lds, stream, &args, sizeof(args));
}

// the device addresses the argument blocks hold (pc_eval_launch.hpp::Addr)
pcl::Addr device_addresses(const pc_handle* h) {
  pcl::Addr A;
  A.qa = h->d_qa.p;
  A.point_x = h->d_point_x.p;
  A.point_V = h->d_pointV.p;
  A.point_r = h->d_pointr.p;
  A.W_end = h->d_Wend.p;
  A.tail_owned = h->d_tail_owned.p;
  A.pt_hslot = h->d_pt_hslot.p;
  A.pt_hlocal = h->d_pt_hlocal.p;
  A.erec = h->d_erec.p;
  A.hb_gran = h->d_hb_gran.p;
  A.rec_slot = h->d_rec_slot.p;
  A.rec_term = h->d_rec_term.p;
  A.timeout = h->h_timeout.p;
  A.phase_args = reinterpret_cast<const PcPhaseArgs*>(h->d_phase_args.p);
  A.trec = h->d_trec.p;
  for (size_t ip = 0; ip < h->pd.size(); ++ip) {
    const PhaseDev& D = *h->pd[ip];
    A.ph[ip] = pcl::PhaseAddr{D.tile_k0.p, D.tile_n0.p, D.sec_s.p, D.sec_h.p, D.sec_E.p, D.hslot0.p, D.hslotN.p, D.hsum_slot.p,
                              D.hsum_local.p, D.scal.p, D.tab.p, D.partials.p, D.gran.p};
  }
  return A;
}

PcPhaseView fill_phase_view(pc_handle* h, int phase, const double* d_x) {
  return pcl::phase_view(h->Q, h->scal, device_addresses(h), phase, d_x);
}

// The scaling, a tile range or a partials buffer changed: the argument blocks, the device copy of the merged launch's
// phase blocks and the uploaded tile records are rebuilt by the next launch.  The caller has synchronised the device.
void invalidate_blocks(pc_handle* h) { h->blocks_dirty = true; }

void refresh_blocks(pc_handle* h) {
  const size_t n = h->Q.ph.size();
  pcl::Records rec;
  if (h->mixed) {
    rec = pcl::launched_records(*h, h->rg, n);
    HIP_OK(hipDeviceSynchronize());   // no launch in flight may still read the old records
    h->d_trec.upload(rec.recs);
  }
  pcl::build_blocks(h->blocks, h->Q, *h, h->scal, h->rg, device_addresses(h), rec);
  if (h->have.k[pcl::BULK_ALL]) {
    HIP_OK(hipDeviceSynchronize());   // no launch in flight may still read the old blocks
    HIP_OK(hipMemcpy(h->d_phase_args.p, h->blocks.merged.data(), n * sizeof(PcPhaseArgs), hipMemcpyHostToDevice));
  }
  h->blocks_dirty = false;
}

hipFunction_t kernel_of(const pc_handle* h, const pcl::Launch& l) {
  return l.kernel == pcl::BULK ? h->pd[l.phase]->fn : h->fn[l.kernel];
}

// One evaluation, or its tiles' or its tail's part: refresh what a change invalidated, plan the call, launch.  The one
// launch site: a call that is not the callback cache's `own` and writes into the handle's result block invalidates it.
void launch_all(pc_handle* h, const pcl::Call& call, hipStream_t st, bool own = false) {
  const double* const out[5] = {call.c, call.G, call.H, call.fobj, call.grad_nz};
  pcc::launched(h->cache, own, pcc::writes_result_block(out, h->d_out.p, h->h_out.p, h->out_total));
  if (h->blocks_dirty) refresh_blocks(h);
  const pcl::Plan p = pcl::plan(h->blocks, *h, h->have, call);
  for (int i = 0; i < p.n; ++i)
    launch_block(kernel_of(h, p.l[i]), p.l[i].grid, p.l[i].block, p.l[i].lds, st, p.l[i].args, p.l[i].arg_bytes);
  h->last_launch = p.last_launch;
}

void upload_scaling(pc_handle* h) {
  auto& Q = h->Q;
  pcc::input_overwritten(h->cache);   // (first: an upload that fails half-way leaves nothing to reuse either)
  for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
    auto& P = Q.ph[ip];
    auto& D = *h->pd[ip];
    const int NZ = P.n_z, NQ = P.n_q, NS = P.n_w, NY = P.n_y, NP = P.n_p;
    std::vector<double> s(2 * NZ + 2 * NQ + 4 + 2 * NS + NY + NP + NQ, 0.0);
    const double* V = h->V_ocp.data() + P.ocp_x_off;
    const double* r = h->r_ocp.data() + P.ocp_x_off;
    int o = 0;
    for (int b = 0; b < NZ; ++b) s[o++] = V[b];
    for (int b = 0; b < NZ; ++b) s[o++] = r[b];
    for (int m = 0; m < NQ; ++m) s[o++] = V[NZ + m];
    for (int m = 0; m < NQ; ++m) s[o++] = r[NZ + m];
    for (int j = 0; j < 2; ++j) s[o++] = j < P.n_t ? V[NZ + NQ + j] : 1.0;
    for (int j = 0; j < 2; ++j) s[o++] = j < P.n_t ? r[NZ + NQ + j] : 0.0;
    for (int l = 0; l < NS; ++l) s[o++] = h->V_ocp[P.wocp(l, Q.ocp_s_off)];   // parameters: q, t or s (pc_pattern.hpp)
    for (int l = 0; l < NS; ++l) s[o++] = h->r_ocp[P.wocp(l, Q.ocp_s_off)];
    const double* W = h->W_ocp.data() + P.ocp_c_off;
    for (int a = 0; a < NY + NP + NQ; ++a) s[o++] = W[a];
    h->scal.phase[ip] = s;
    if (h->device >= 0) {
      if (D.scal.n != s.size()) D.scal.alloc(s.size());
      HIP_OK(hipMemcpy(D.scal.p, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
      // scal | goff | hoff as one table (pc::bulk stages it into LDS for models with many variables)
      std::vector<double> tab(s);
      auto append = [&](const std::vector<int64_t>& v) {
        for (int64_t e : v) {
          double d;
          std::memcpy(&d, &e, sizeof(d));
          tab.push_back(d);
        }
      };
      append(P.goff);
      append(P.hoff);
      if (D.tab.n != tab.size()) D.tab.alloc(tab.size());
      HIP_OK(hipMemcpy(D.tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  if (h->device >= 0) {
    const size_t np = Q.point_x.size();
    std::vector<double> pv(np), pr(np), we(Q.n_b);
    for (size_t i = 0; i < np; ++i) {
      pv[i] = h->V_ocp[Q.point_ocp[i]];
      pr[i] = h->r_ocp[Q.point_ocp[i]];
    }
    for (int r = 0; r < Q.n_b; ++r) we[r] = h->W_ocp[Q.ocp_c_end_off + r];
    h->d_pointV.upload(pv);
    h->d_pointr.upload(pr);
    h->d_Wend.upload(we);
    h->scal.pointV = pv;
    h->scal.pointr = pr;
    h->scal.Wend = we;
  }
}

void require_device(pc_handle* h) {
  if (!h) throw std::runtime_error("null handle");
  if (h->device < 0)
    throw std::runtime_error("handle was created with device = -1 (structure only): no evaluation is possible "
                             "without a GPU; this library has no CPU fallback");
  if (!h->scaling_set) throw std::runtime_error("pc_set_scaling must be called before evaluating");
  HIP_OK(hipSetDevice(h->device));
}

// ---- host-pointer staging ---------------------------------------------------------------------------
// The resident tail spins (bounded) for values of the other workgroups; a tail that gave up says so here.
void check_timeout(pc_handle* h) {
  if (h->h_timeout.p && h->h_timeout.p[0]) {
    const unsigned code = h->h_timeout.p[0];
    h->h_timeout.p[0] = 0;
    throw std::runtime_error("resident tail: granules of " + std::string(code >= 100 ? "an edge-node Hessian entry" : "a phase's partial sums") +
                             " never arrived (code " + std::to_string(code) + "); the results of this evaluation are invalid");
  }
}

// Wait for the handle's stream (poll_then_block), then hear a tail that gave up.
void wait_stream(pc_handle* h) {
  wait_for(h->stream, h->spin_us);
  check_timeout(h);
}
// what the kernels are handed for x~, lambda and the outputs: the device mirror, or the pinned host block itself
const double* kx(pc_handle* h) { return (h->cache.mode & 1) ? h->h_in.p : h->d_in.p; }
const double* klam(pc_handle* h) { return kx(h) + h->o_lam; }
double* kout(pc_handle* h, size_t off) { return ((h->cache.mode & 2) ? h->h_out.p : h->d_out.p) + off; }
// a device-pointer call: the caller's vectors, J into the handle's own output block; every flag unless the caller says
pcl::Call device_call(pc_handle* h, const double* d_x, const double* d_lambda, double* d_g, double* d_jac, double* d_hess) {
  pcl::Call call;
  call.x = d_x; call.lam = d_lambda; call.c = d_g; call.G = d_jac; call.H = d_hess;
  call.fobj = h->d_out.p + h->o_f;
  call.flags = PC_FLAG_C | PC_FLAG_G | PC_FLAG_H;
  return call;
}
// a host-pointer call that computes `flags`: the staged x~ (and lambda with PC_FLAG_H) in, the packed output block out
pcl::Call host_call(pc_handle* h, int flags) {
  pcl::Call call;
  call.x = kx(h);
  call.lam = (flags & PC_FLAG_H) ? klam(h) : nullptr;
  call.c = (flags & PC_FLAG_C) ? kout(h, h->o_c) : nullptr;
  call.G = (flags & PC_FLAG_G) ? kout(h, h->o_G) : nullptr;
  call.H = (flags & PC_FLAG_H) ? kout(h, h->o_H) : nullptr;
  call.fobj = kout(h, h->o_f);
  call.grad_nz = kout(h, h->o_gn);
  call.flags = flags;
  return call;
}

// [begin, begin + count) of the input block into its pinned copy unless it is there, and up unless the kernels read that
void stage(pc_handle* h, const double* src, size_t begin, size_t count) {
  if (!src) throw std::runtime_error(begin ? "null lambda" : "null x");
  double* dst = h->h_in.p + begin;
  if (src != dst) std::memcpy(dst, src, count * sizeof(double));
  if (!(h->cache.mode & 1))
    HIP_OK(hipMemcpyAsync(h->d_in.p + begin, dst, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
}
void stage_x(pc_handle* h, const double* x) { stage(h, x, 0, h->Q.num_x); }
void stage_lambda(pc_handle* h, const double* lambda) { stage(h, lambda, h->o_lam, h->Q.num_c); }

void copy_down(pc_handle* h, size_t begin, size_t end) {   // [begin, end) of the output block, device -> pinned host
  if (h->cache.mode & 2) return;                            // the kernels wrote there themselves
  HIP_OK(hipMemcpyAsync(h->h_out.p + begin, h->d_out.p + begin, (end - begin) * sizeof(double), hipMemcpyDeviceToHost,
                        h->stream));
}
void copy_down(pc_handle* h, size_t begin, size_t end, hipEvent_t done) {
  copy_down(h, begin, end);
  HIP_OK(hipEventRecord(done, h->stream));
}

// the body of a host-pointer call that stages or fills: a failure on the way leaves nothing to reuse
template <class F>
void or_forget(pc_handle* h, F&& body) {
  try {
    body();
  } catch (...) {
    pcc::input_overwritten(h->cache);
    throw;
  }
}

// A host-pointer callback (pc_callback_cache.hpp): stage, fill, queue the copies and wait as the cache says.
void callback(pc_handle* h, const double* x, int new_x, pcc::Want want) {
  require_device(h);
  or_forget(h, [&] {
    const pcc::Todo t = pcc::callback(h->cache, new_x, want);
    if (t.stage_x) stage_x(h, x);
    if (t.launch) launch_all(h, host_call(h, PC_FLAG_C | PC_FLAG_G), h->stream, true);
    if (t.queue_small) copy_down(h, 0, h->o_c + h->Q.num_c, h->ev_small);
    if (t.queue_G) copy_down(h, h->o_G, h->o_G + h->Q.g_row.size(), h->ev_G);
    if (t.wait == pcc::NO_WAIT) return;
    wait_for(t.wait == pcc::EV_G ? h->ev_G : h->ev_small, h->spin_us);
    check_timeout(h);
  });
}

// a device-pointer entry point: the caller's stream or the handle's, the caller's vectors, the entry's own settings
template <class Tweak>
hipStream_t launch_device(pc_handle* h, const double* d_x, const double* d_lambda, double* d_g, double* d_jac, double* d_hess,
                          void* stream, Tweak&& tweak) {
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  pcl::Call call = device_call(h, d_x, d_lambda, d_g, d_jac, d_hess);
  tweak(call);
  launch_all(h, call, st);
  return st;
}

// grad J of the pinned result block, scattered from its structural non-zeros
void scatter_grad(pc_handle* h, double* grad) {
  const auto& Q = h->Q;
  std::memset(grad, 0, Q.num_x * sizeof(double));
  for (size_t e = 0; e < Q.jgrad_col.size(); ++e) grad[Q.point_x[Q.jgrad_col[e]]] = h->h_out.p[h->o_gn + e];
}

// a kernel of the handle's code object, whichever of its modules holds it
hipError_t find_fn(pc_handle* h, hipFunction_t* fn, const char* name) {
  *fn = nullptr;
  hipError_t e = hipModuleGetFunction(fn, h->module, name);
  for (size_t i = 0; e != hipSuccess && i < h->more_modules.size(); ++i) {
    (void)hipGetLastError();
    e = hipModuleGetFunction(fn, h->more_modules[i], name);
  }
  if (e != hipSuccess) *fn = nullptr;
  return e;
}

// The one reader of the launch shape's knobs (pc_eval_shape.hpp::Knobs): the environment, and the LDS a workgroup of
// `device` may request.
pce::Knobs read_knobs(int device) {
  pce::Knobs kn;
  auto env_int = [](const char* name, auto& dst) {
    if (const char* env = std::getenv(name)) dst = std::atoi(env);
  };
  auto env_i64 = [](const char* name, int64_t& dst) {
    if (const char* env = std::getenv(name)) dst = std::atoll(env);
  };
  auto env_flag = [](const char* name, bool& dst) {
    if (const char* env = std::getenv(name)) dst = std::atoi(env) != 0;
  };
  env_int("PYCOLLO_AMD_TB", kn.tb);
  env_int("PYCOLLO_AMD_WPT", kn.wpt);
  env_int("PYCOLLO_AMD_TILE_NODES", kn.tile_nodes);
  env_flag("PYCOLLO_AMD_TWO_WAVE", kn.two_wave);
  env_i64("PYCOLLO_AMD_TWO_WAVE_MAX_TILES", kn.two_wave_max_tiles);
  env_i64("PYCOLLO_AMD_TWO_WAVE_TILES", kn.two_wave_tiles);
  env_i64("PYCOLLO_AMD_TWO_WAVE_MAX_WAVES", kn.two_wave_max_waves);
  env_int("PYCOLLO_AMD_MIX_MIN_RUN_ROWS", kn.mix_min_run_rows);
  env_int("PYCOLLO_AMD_MIX_CAP_ROWS", kn.mix_cap_rows);
  env_flag("PYCOLLO_AMD_RESIDENT", kn.resident);
  env_int("PYCOLLO_AMD_TAIL_BLOCKS", kn.tail_blocks);
  env_flag("PYCOLLO_AMD_MERGE", kn.merge);
  int v = 0;
  if (device >= 0 && hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0)
    kn.lds_limit = v;
  return kn;
}

}  // namespace

extern "C" {

const char* pc_last_error(void) { return g_err.c_str(); }

int pc_create(const pc_problem_desc* d, pc_handle** out) {
  if (out) *out = nullptr;
  std::unique_ptr<pc_handle> h;
  const int ok = guarded(g_err, [&] {
    if (!d || !out) throw std::runtime_error("null descriptor or output pointer");
    if (d->n_phases < 1 || d->n_phases > PC_MAX_PHASES) throw std::runtime_error("n_phases must be in [1, 8]");
    h.reset(new pc_handle());
    auto& Q = h->Q;
    pcp::from_desc(*d, Q);   // pc_desc.hpp: plain C++, also compiled (with sanitizers) by the CPU test harness
    const pce::Knobs kn = read_knobs(d->device);
    static_cast<pce::Shape&>(*h) = pce::build_shape(*d, Q, kn);   // pc_eval_shape.hpp: plain C++, tested on the CPU
    h->pd.resize(Q.ph.size());
    h->scal.phase.resize(Q.ph.size());
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      h->pd[ip].reset(new PhaseDev());
      h->rg[ip].tile_end = h->ph[ip].n_tiles;
    }
    if (d->plan_only) return;   // the tiling alone (a rank of the section-sharded evaluation asks for its range, sharding.py)
    h->qa.assign(d->quad_A, d->quad_A + h->qa_n);
    h->qw.assign(d->quad_w, d->quad_w + h->qw_n);
    h->device = d->device;
    h->V_ocp.assign(Q.num_ocp_x, 1.0);
    h->r_ocp.assign(Q.num_ocp_x, 0.0);
    h->W_ocp.assign(Q.num_ocp_c, 1.0);
    if (const char* env = std::getenv("PYCOLLO_AMD_SPIN_US")) h->spin_us = std::atoi(env);
    h->n_launches = pcl::launches_per_evaluation(*h, h->have, Q.ph.size());   // again once the module is loaded
    if (h->device < 0) return;  // structure-only handle

    // ---- device side ----------------------------------------------------------------------------
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= h->device)
      throw std::runtime_error("requested HIP device is not available (no GPU visible?)");
    HIP_OK(hipSetDevice(h->device));
    if (!d->code_object || !d->tail_kernel) throw std::runtime_error("code_object and tail_kernel are required");
    HIP_OK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIP_OK(hipModuleLoad(&h->module, d->code_object));
    {
      const std::string path = d->code_object, ext = ".hsaco";
      const std::string base = path.size() > ext.size() && path.compare(path.size() - ext.size(), ext.size(), ext) == 0
                                   ? path.substr(0, path.size() - ext.size()) : path;
      for (int k = 1; k < 16; ++k) {
        const std::string part = base + ".p" + std::to_string(k) + ext;
        FILE* f = std::fopen(part.c_str(), "rb");
        if (!f) break;
        std::fclose(f);
        hipModule_t m = nullptr;
        HIP_OK(hipModuleLoad(&m, part.c_str()));
        h->more_modules.push_back(m);
      }
    }
    // the kernels, by their names in pc_eval_launch.hpp; a code object without an optional one falls back (pcl::Have)
    auto name = [&](pcl::Kernel k, int phase, int wpt) { return pcl::kernel_name(Q, d->tail_kernel, k, phase, wpt); };
    auto optional = [&](pcl::Kernel k, int wpt) {
      if (find_fn(h.get(), &h->fn[k], name(k, 0, wpt).c_str()) != hipSuccess) {
        (void)hipGetLastError();
        h->fn[k] = nullptr;
      }
      return h->have.k[k] = h->fn[k] != nullptr;
    };
    HIP_OK(find_fn(h.get(), &h->fn[pcl::TAIL], name(pcl::TAIL, 0, 1).c_str()));
    optional(pcl::TAIL_BIG, 1);
    if (Q.ph.size() > 1) {
      if (kn.merge && optional(pcl::BULK_ALL, 1)) {
        h->d_phase_args.alloc(Q.ph.size() * sizeof(PcPhaseArgs));
        if (optional(pcl::BULK_ALL_RES, 1) && h->wpt_all > 1) optional(pcl::BULK_ALL_RES_W, h->wpt_all);
      }
    } else if (optional(pcl::BULK_RES, 1) && h->ph[0].wpt > 1) {
      optional(pcl::BULK_RES_W, h->ph[0].wpt);   // the same kernel with the replica index compiled in (codegen: light / medium models)
    }
    {   // one buffer: the weight tables right behind the A tables (the kernels address both from `qa`)
      std::vector<double> both(h->qa);
      both.insert(both.end(), h->qw.begin(), h->qw.end());
      h->d_qa.upload(both);
    }
    for (size_t ip = 0; ip < Q.ph.size(); ++ip) {
      auto& P = Q.ph[ip];
      auto& D = *h->pd[ip];
      HIP_OK(find_fn(h.get(), &D.fn, name(pcl::BULK, (int)ip, 1).c_str()));
      D.tile_k0.upload(P.tile_k0);
      {
        std::vector<int32_t> tn(P.tile_k0.size());
        for (size_t i = 0; i < tn.size(); ++i) tn[i] = P.sec_s[P.tile_k0[i]];
        D.tile_n0.upload(tn);
      }
      D.sec_s.upload(P.sec_s);
      D.sec_h.upload(P.h_k);
      D.sec_E.upload(P.sec_E);
      D.hslot0.upload(P.hslot0);
      D.hslotN.upload(P.hslotN);
      D.hsum_slot.upload(P.hsum_slot);
      D.hsum_local.upload(P.hsum_local);
      D.partials.alloc((size_t)std::max(1, P.nred) * h->ph[ip].n_tiles);
      D.gran.upload(std::vector<unsigned long long>((size_t)2 * std::max(1, P.nred) * h->ph[ip].n_tiles, 0ull));   // tag 0: never written
    }
    {   // the edge records (Shape::rec_slot): never an empty buffer
      std::vector<int64_t> rec_slot(h->rec_slot);
      std::vector<int32_t> rec_term(h->rec_term);
      if (rec_slot.empty()) { rec_slot.push_back(-1); rec_term.push_back(-1); }
      h->d_rec_slot.upload(rec_slot);
      h->d_rec_term.upload(rec_term);
      h->d_erec.upload(std::vector<unsigned long long>(2 * rec_slot.size(), 0ull));
    }
    h->d_hb_gran.upload(std::vector<unsigned long long>(2 * std::max<size_t>(1, Q.pthess_row.size()), 0ull));
    h->h_timeout.alloc(16);
    std::memset(h->h_timeout.p, 0, 16 * sizeof(unsigned));
    h->d_point_x.upload(Q.point_x);
    h->d_tail_owned.upload(Q.tail_owned);
    h->d_pt_hslot.upload(Q.pt_hslot);
    h->d_pt_hlocal.upload(Q.pt_hlocal);
    h->d_g_indptr.upload(Q.g_indptr);
    h->d_in.alloc(h->in_total); h->d_out.alloc(h->out_total);
    h->h_in.alloc(h->in_total); h->h_out.alloc(h->out_total);
    h->d_norms.alloc(Q.num_c); h->h_norms.alloc(Q.num_c);
    HIP_OK(hipMemset(h->d_in.p, 0, h->in_total * sizeof(double)));
    HIP_OK(hipMemset(h->d_out.p, 0, h->out_total * sizeof(double)));
    std::memset(h->h_in.p, 0, h->in_total * sizeof(double));
    std::memset(h->h_out.p, 0, h->out_total * sizeof(double));
    HIP_OK(hipEventCreateWithFlags(&h->ev_small, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&h->ev_G, hipEventDisableTiming));
    if (const char* env = std::getenv("PYCOLLO_AMD_HOST_MODE")) pcc::set_mode(h->cache, std::atoi(env) & 3);
    h->n_launches = pcl::launches_per_evaluation(*h, h->have, Q.ph.size());
  });
  if (!ok) return 0;
  *out = h.release();
  return 1;
}

void pc_destroy(pc_handle* h) {
  if (!h) return;
  if (h->device >= 0) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
  }
  h->pd.clear();
  if (h->ev_small) (void)hipEventDestroy(h->ev_small);
  if (h->ev_G) (void)hipEventDestroy(h->ev_G);
  for (hipModule_t m : h->more_modules) (void)hipModuleUnload(m);
  if (h->module) (void)hipModuleUnload(h->module);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int pc_get_info(const pc_handle* h, pc_info* info) {
  return guarded(g_err, [&] {
    if (!h || !info) throw std::runtime_error("null argument");
    const auto& Q = h->Q;
    info->n = (int32_t)Q.num_x;
    info->m = (int32_t)Q.num_c;
    info->nnz_jac = (int64_t)Q.g_row.size();
    info->nnz_hess = (int64_t)Q.h_row.size();
    info->algorithmic_bytes = 8 * (Q.num_x + Q.num_c) + 8 * (Q.num_c + info->nnz_jac + info->nnz_hess);
    int nt = 0;
    for (auto& D : h->ph) nt += D.n_tiles;
    info->n_tiles_total = nt;
    info->threads_per_block = h->TB;
    info->lds_bytes_max = (h->Q.ph.size() > 1 && h->lds_all > 0) ? h->lds_all : h->lds_max;   // the merged launch's when there is one
    info->n_launches = h->n_launches;
    info->waves_per_tile = 1;
    for (auto& D : h->ph) info->waves_per_tile = std::max(info->waves_per_tile, (int32_t)D.wpt);
    if (h->have.k[pcl::BULK_ALL]) info->waves_per_tile = h->wpt_all;
    info->last_launch = h->last_launch;
  });
}

int pc_sizes(const pc_handle* h, int32_t* n, int32_t* m, int64_t* nnz_jac, int64_t* nnz_hess) {
  return guarded(g_err, [&] {
    if (!h) throw std::runtime_error("null handle");
    if (n) *n = (int32_t)h->Q.num_x;
    if (m) *m = (int32_t)h->Q.num_c;
    if (nnz_jac) *nnz_jac = (int64_t)h->Q.g_row.size();
    if (nnz_hess) *nnz_hess = (int64_t)h->Q.h_row.size();
  });
}

int pc_jac_structure(const pc_handle* h, int32_t* iRow, int32_t* jCol) {
  return guarded(g_err, [&] {
    if (!h || !iRow || !jCol) throw std::runtime_error("null argument");
    std::memcpy(iRow, h->Q.g_row.data(), h->Q.g_row.size() * sizeof(int32_t));
    std::memcpy(jCol, h->Q.g_col.data(), h->Q.g_col.size() * sizeof(int32_t));
  });
}

int pc_hess_structure(const pc_handle* h, int32_t* iRow, int32_t* jCol) {
  return guarded(g_err, [&] {
    if (!h || !iRow || !jCol) throw std::runtime_error("null argument");
    std::memcpy(iRow, h->Q.h_row.data(), h->Q.h_row.size() * sizeof(int32_t));
    std::memcpy(jCol, h->Q.h_col.data(), h->Q.h_col.size() * sizeof(int32_t));
  });
}

int pc_set_scaling(pc_handle* h, const double* V, const double* r, const double* W, double w_J) {
  return guarded(g_err, [&] {
    if (!h || !V || !r || !W) throw std::runtime_error("null argument");
    if (h->device >= 0) {
      // evaluations may be in flight on a caller's stream (pc_eval_all_device): none may still read the tables
      HIP_OK(hipSetDevice(h->device));
      HIP_OK(hipDeviceSynchronize());
    }
    h->V_ocp.assign(V, V + h->Q.num_ocp_x);
    h->r_ocp.assign(r, r + h->Q.num_ocp_x);
    h->W_ocp.assign(W, W + h->Q.num_ocp_c);
    h->scal.wJ = w_J;
    upload_scaling(h);
    h->scaling_set = true;
    invalidate_blocks(h);
  });
}

int pc_eval_all_device(pc_handle* h, const double* d_x, double obj_factor, const double* d_lambda, double* d_g,
                       double* d_jac, double* d_hess, void* stream) {
  return guarded(g_err, [&] {
    require_device(h);
    check_timeout(h);   // a previous device-API evaluation whose tail gave up: say so before queueing more work
    launch_device(h, d_x, d_lambda, d_g, d_jac, d_hess, stream, [&](pcl::Call& call) { call.sigma = obj_factor; });
  });
}

int pc_check(pc_handle* h) {
  return guarded(g_err, [&] {
    require_device(h);
    check_timeout(h);
  });
}

int pc_launch_bulk_device(pc_handle* h, const double* d_x, const double* d_lambda, double* d_g, double* d_jac,
                          double* d_hess, void* stream) {
  return guarded(g_err, [&] {
    require_device(h);
    launch_device(h, d_x, d_lambda, d_g, d_jac, d_hess, stream, [](pcl::Call& call) { call.tail = false; });
  });
}

int pc_launch_bulk_flags_device(pc_handle* h, const double* d_x, const double* d_lambda, double* d_g, double* d_jac,
                                double* d_hess, int flags, void* stream) {
  return guarded(g_err, [&] {
    require_device(h);
    if (flags & ~(PC_FLAG_C | PC_FLAG_G | PC_FLAG_H)) throw std::runtime_error("flags must be a combination of 1 (g), 2 (jac_g), 4 (hess)");
    launch_device(h, d_x, d_lambda, d_g, d_jac, d_hess, stream, [&](pcl::Call& call) {
      call.flags = flags;
      call.tail = false;
    });
  });
}

int pc_launch_tail_device(pc_handle* h, const double* d_x, double obj_factor, const double* d_lambda, double* d_g,
                          double* d_jac, double* d_hess, void* stream) {
  return guarded(g_err, [&] {
    require_device(h);
    launch_device(h, d_x, d_lambda, d_g, d_jac, d_hess, stream, [&](pcl::Call& call) {
      call.sigma = obj_factor;
      call.bulk = false;
    });
  });
}

// The tail launch of a sharded evaluation that also delivers the objective and its gradient (host): what a solver's
// objective / gradient callbacks need from a rank that never runs the whole evaluation (pycollo_amd/ipm_sharded.py).
// Synchronises `stream`.
int pc_launch_tail_objective_device(pc_handle* h, const double* d_x, double obj_factor, const double* d_lambda, double* d_g,
                                    double* d_jac, double* d_hess, void* stream, double* f, double* grad) {
  return guarded(g_err, [&] {
    require_device(h);
    hipStream_t st = launch_device(h, d_x, d_lambda, d_g, d_jac, d_hess, stream, [&](pcl::Call& call) {
      call.grad_nz = h->d_out.p + h->o_gn;
      call.sigma = obj_factor;
      call.bulk = false;
    });
    HIP_OK(hipMemcpyAsync(h->h_out.p, h->d_out.p, (1 + h->Q.jgrad_col.size()) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (f) *f = h->h_out.p[h->o_f];
    if (grad) scatter_grad(h, grad);
  });
}

int pc_set_tile_range(pc_handle* h, int phase, int tile_begin, int tile_end) {
  return guarded(g_err, [&] {
    if (!h || phase < 0 || phase >= (int)h->pd.size()) throw std::runtime_error("phase out of range");
    if (tile_begin < 0 || tile_end < tile_begin || tile_end > h->ph[phase].n_tiles) throw std::runtime_error("tile range out of range");
    if (h->device >= 0) {
      HIP_OK(hipSetDevice(h->device));
      HIP_OK(hipDeviceSynchronize());   // launches in flight on any stream still use the old range
    }
    h->rg[phase].tile_begin = tile_begin;
    h->rg[phase].tile_end = tile_end;
    pcc::range_changed(h->cache);
    invalidate_blocks(h);
  });
}

int pc_phase_tiles(const pc_handle* h, int phase, int32_t* n_tiles, int32_t* nred, int32_t* tile_k0) {
  return guarded(g_err, [&] {
    if (!h || phase < 0 || phase >= (int)h->pd.size()) throw std::runtime_error("phase out of range");
    const auto& P = h->Q.ph[phase];
    if (n_tiles) *n_tiles = (int32_t)P.tile_k0.size() - 1;
    if (nred) *nred = P.nred;
    if (tile_k0) std::memcpy(tile_k0, P.tile_k0.data(), P.tile_k0.size() * sizeof(int32_t));
  });
}

int pc_phase_tile_orders(const pc_handle* h, int phase, int32_t* tile_order) {
  return guarded(g_err, [&] {
    if (!h || phase < 0 || phase >= (int)h->Q.ph.size() || !tile_order) throw std::runtime_error("phase out of range or null output");
    auto& P = h->Q.ph[phase];
    for (size_t t = 0; t + 1 < P.tile_k0.size(); ++t) tile_order[t] = t < P.tile_order.size() ? P.tile_order[t] : 0;
  });
}

int pc_set_partials_buffer(pc_handle* h, int phase, double* d_partials) {
  return guarded(g_err, [&] {
    if (!h || phase < 0 || phase >= (int)h->pd.size()) throw std::runtime_error("phase out of range");
    if (h->device >= 0) {
      HIP_OK(hipSetDevice(h->device));
      HIP_OK(hipDeviceSynchronize());
    }
    h->rg[phase].partials_ext = d_partials;
    invalidate_blocks(h);
  });
}

int pc_eval_all(pc_handle* h, const double* x, double obj_factor, const double* lambda, double* g, double* jac,
                double* hess) {
  return guarded(g_err, [&] {
    require_device(h);
    auto& Q = h->Q;
    if (!x || !lambda || !g || !jac || !hess) throw std::runtime_error("null argument");
    or_forget(h, [&] {
      // one block up: [x~ | lambda] (contiguous in the pinned block, gap included)
      if (x != h->h_in.p) std::memcpy(h->h_in.p, x, Q.num_x * sizeof(double));
      if (lambda != h->h_in.p + h->o_lam) std::memcpy(h->h_in.p + h->o_lam, lambda, Q.num_c * sizeof(double));
      if (!(h->cache.mode & 1))
        HIP_OK(hipMemcpyAsync(h->d_in.p, h->h_in.p, h->in_total * sizeof(double), hipMemcpyHostToDevice, h->stream));
      pcl::Call call = host_call(h, PC_FLAG_C | PC_FLAG_G | PC_FLAG_H);
      call.sigma = obj_factor;
      launch_all(h, call, h->stream, true);
      // one block down: [J | grad J | c~ | G~ | H~]
      copy_down(h, 0, h->o_H + Q.h_row.size());
      wait_stream(h);
    });
    if (g != h->h_out.p + h->o_c) std::memcpy(g, h->h_out.p + h->o_c, Q.num_c * sizeof(double));
    if (jac != h->h_out.p + h->o_G) std::memcpy(jac, h->h_out.p + h->o_G, Q.g_row.size() * sizeof(double));
    if (hess != h->h_out.p + h->o_H) std::memcpy(hess, h->h_out.p + h->o_H, Q.h_row.size() * sizeof(double));
    pcc::filled_all(h->cache);
  });
}

int pc_host_buffers(pc_handle* h, double** x, double** lambda, double** g, double** jac, double** hess) {
  return guarded(g_err, [&] {
    require_device(h);
    if (x) *x = h->h_in.p;
    if (lambda) *lambda = h->h_in.p + h->o_lam;
    if (g) *g = h->h_out.p + h->o_c;
    if (jac) *jac = h->h_out.p + h->o_G;
    if (hess) *hess = h->h_out.p + h->o_H;
  });
}

int pc_set_prefetch_jac(pc_handle* h, int on) {
  return guarded(g_err, [&] {
    require_device(h);
    pcc::set_prefetch(h->cache, on != 0);
  });
}

uint64_t pc_cache_generation(const pc_handle* h) { return h ? h->cache.generation : 0; }

int pc_set_host_mode(pc_handle* h, int mode) {
  return guarded(g_err, [&] {
    require_device(h);
    if (mode < 0 || mode > 3) throw std::runtime_error("host mode must be 0..3");
    HIP_OK(hipStreamSynchronize(h->stream));
    pcc::set_mode(h->cache, mode);
  });
}

// J, grad J, c~ and G~ are produced together by the first callback at a new x and kept for the companion calls
// (IPOPT evaluates f, grad f, g, jac g at the same x, passing new_x = 1 to the first of them only;
// pycollo/nlp.py:47-57).  The small results [J | grad J | c~] and the large one, G~, come down as two copies so that
// eval_f / eval_g of a line-search trial point wait for the small one only (callback, pc_callback_cache.hpp).
int pc_eval_f(pc_handle* h, const double* x, int new_x, double* f) {
  return guarded(g_err, [&] {
    callback(h, x, new_x, pcc::SMALL);
    *f = h->h_out.p[h->o_f];
  });
}

int pc_eval_grad_f(pc_handle* h, const double* x, int new_x, double* grad) {
  return guarded(g_err, [&] {
    callback(h, x, new_x, pcc::SMALL);
    scatter_grad(h, grad);
  });
}

int pc_eval_g(pc_handle* h, const double* x, int new_x, double* g) {
  return guarded(g_err, [&] {
    callback(h, x, new_x, pcc::SMALL);
    if (g != h->h_out.p + h->o_c) std::memcpy(g, h->h_out.p + h->o_c, h->Q.num_c * sizeof(double));
  });
}

int pc_eval_jac_g(pc_handle* h, const double* x, int new_x, double* values) {
  return guarded(g_err, [&] {
    callback(h, x, new_x, pcc::G);
    if (values != h->h_out.p + h->o_G) std::memcpy(values, h->h_out.p + h->o_G, h->Q.g_row.size() * sizeof(double));
  });
}

int pc_eval_h(pc_handle* h, const double* x, int new_x, double obj_factor, const double* lambda, int new_lambda,
              double* values) {
  (void)new_lambda;   // sigma and lambda are cheap to restage; H~ is always re-evaluated
  return guarded(g_err, [&] {
    require_device(h);
    auto& Q = h->Q;
    or_forget(h, [&] {
      if (pcc::hessian(h->cache, new_x).stage_x) stage_x(h, x);
      stage_lambda(h, lambda);
      pcl::Call call = host_call(h, PC_FLAG_H);
      call.grad_nz = nullptr;
      call.sigma = obj_factor;
      launch_all(h, call, h->stream, true);
      copy_down(h, h->o_H, h->o_H + Q.h_row.size());
      wait_stream(h);
    });
    // the stream has drained: earlier copies are complete too -- G~'s only if it was ever queued (prefetch off and
    // kernels not writing host memory: G~ is still on the device and pc_eval_jac_g must fetch it)
    pcc::drained(h->cache);
    if (values != h->h_out.p + h->o_H) std::memcpy(values, h->h_out.p + h->o_H, Q.h_row.size() * sizeof(double));
  });
}

int pc_eval_resident(pc_handle* h, const double* x, double obj_factor, const double* lambda, double* f, double* grad,
                     double* g) {
  return guarded(g_err, [&] {
    require_device(h);
    auto& Q = h->Q;
    if (!x) throw std::runtime_error("null x");
    pcc::input_overwritten(h->cache);   // (the callback cache describes the host copies; G~ is not copied)
    {
      pcc::ThroughMirror mirror(h->cache);   // results stay in (and are read from) the device mirror
      std::memcpy(h->h_in.p, x, Q.num_x * sizeof(double));
      if (lambda) std::memcpy(h->h_in.p + h->o_lam, lambda, Q.num_c * sizeof(double));
      HIP_OK(hipMemcpyAsync(h->d_in.p, h->h_in.p, (lambda ? h->in_total : (size_t)Q.num_x) * sizeof(double),
                            hipMemcpyHostToDevice, h->stream));
      pcl::Call call = host_call(h, PC_FLAG_C | PC_FLAG_G | (lambda ? PC_FLAG_H : 0));
      call.sigma = obj_factor;
      launch_all(h, call, h->stream, true);
      copy_down(h, 0, h->o_c + Q.num_c);
      wait_stream(h);
    }
    if (f) *f = h->h_out.p[h->o_f];
    if (grad) scatter_grad(h, grad);
    if (g) std::memcpy(g, h->h_out.p + h->o_c, Q.num_c * sizeof(double));
  });
}

int pc_device_results(pc_handle* h, const double** d_g, const double** d_jac, const double** d_hess) {
  return guarded(g_err, [&] {
    require_device(h);
    if (d_g) *d_g = h->d_out.p + h->o_c;
    if (d_jac) *d_jac = h->d_out.p + h->o_G;
    if (d_hess) *d_hess = h->d_out.p + h->o_H;
  });
}

// ---- IPOPT's callback types (include/pycollo_amd.h) ------------------------------------------------------
static bool ipopt_sizes_ok(pc_handle* h, int n, int m, int64_t nele, int which) {
  if (!h) { set_err("null user_data"); return false; }
  const auto& Q = h->Q;
  const int64_t want = which == 1 ? (int64_t)Q.g_row.size() : (which == 2 ? (int64_t)Q.h_row.size() : -1);
  if (n != (int)Q.num_x || (m >= 0 && m != (int)Q.num_c) || (which && nele != want)) {
    set_err("IPOPT callback: n / m / number of non-zeros do not match the handle");
    return false;
  }
  return true;
}

int pc_ipopt_eval_f(int n, double* x, int new_x, double* obj_value, void* user_data) {
  pc_handle* h = static_cast<pc_handle*>(user_data);
  if (!ipopt_sizes_ok(h, n, -1, 0, 0)) return 0;
  return pc_eval_f(h, x, new_x, obj_value);
}

int pc_ipopt_eval_grad_f(int n, double* x, int new_x, double* grad_f, void* user_data) {
  pc_handle* h = static_cast<pc_handle*>(user_data);
  if (!ipopt_sizes_ok(h, n, -1, 0, 0)) return 0;
  return pc_eval_grad_f(h, x, new_x, grad_f);
}

int pc_ipopt_eval_g(int n, double* x, int new_x, int m, double* g, void* user_data) {
  pc_handle* h = static_cast<pc_handle*>(user_data);
  if (!ipopt_sizes_ok(h, n, m, 0, 0)) return 0;
  return pc_eval_g(h, x, new_x, g);
}

int pc_ipopt_eval_jac_g(int n, double* x, int new_x, int m, int nele_jac, int* iRow, int* jCol, double* values,
                        void* user_data) {
  pc_handle* h = static_cast<pc_handle*>(user_data);
  if (!ipopt_sizes_ok(h, n, m, nele_jac, 1)) return 0;
  if (!values) return pc_jac_structure(h, iRow, jCol);   // IPOPT's structure query (x may be NULL)
  return pc_eval_jac_g(h, x, new_x, values);
}

int pc_ipopt_eval_h(int n, double* x, int new_x, double obj_factor, int m, double* lambda, int new_lambda,
                    int nele_hess, int* iRow, int* jCol, double* values, void* user_data) {
  pc_handle* h = static_cast<pc_handle*>(user_data);
  if (!ipopt_sizes_ok(h, n, m, nele_hess, 2)) return 0;
  if (!values) return pc_hess_structure(h, iRow, jCol);
  return pc_eval_h(h, x, new_x, obj_factor, lambda, new_lambda, values);
}

int pc_row_norms_jac(pc_handle* h, const double* x, double* norms) {
  return guarded(g_err, [&] {
    require_device(h);
    // always through the device mirror: the row reduction reads G~ back
    pcc::input_overwritten(h->cache);
    {
      pcc::ThroughMirror mirror(h->cache);
      callback(h, x, 1, pcc::NOTHING);
    }
    const int64_t m = h->Q.num_c;
    const int64_t threads = m * 64;
    const int blocks = (int)((threads + 255) / 256);
    or_forget(h, [&] {
      hipLaunchKernelGGL(row_norms_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_g_indptr.p, h->d_out.p + h->o_G,
                         h->d_norms.p, m);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(h->h_norms.p, h->d_norms.p, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_OK(hipStreamSynchronize(h->stream));
    });
    std::memcpy(norms, h->h_norms.p, m * sizeof(double));
    pcc::row_norms_done(h->cache);
  });
}

int pc_interp_linear(int device, const double* tau_prev, int n_prev, const double* vals_prev, int n_vars,
                     const double* tau_new, int n_new, double* out) {
  return guarded(g_err, [&] {
    if (n_prev < 2 || n_new < 1 || n_vars < 0) throw std::runtime_error("interpolation needs at least two abscissae");
    int ndev = 0;
    if (device < 0 || hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device)
      throw std::runtime_error("requested HIP device is not available (no GPU visible?); this library has no CPU fallback");
    HIP_OK(hipSetDevice(device));
    DevBuf<double> d_tp, d_vp, d_tn, d_out;
    d_tp.upload(std::vector<double>(tau_prev, tau_prev + n_prev));
    d_vp.upload(std::vector<double>(vals_prev, vals_prev + (size_t)n_vars * n_prev));
    d_tn.upload(std::vector<double>(tau_new, tau_new + n_new));
    d_out.alloc((size_t)std::max(1, n_vars) * n_new);
    hipLaunchKernelGGL(interp_linear_kernel, dim3((n_new + 255) / 256), dim3(256), 0, 0, d_tp.p, n_prev, d_vp.p, n_vars,
                       d_tn.p, n_new, d_out.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out, d_out.p, sizeof(double) * (size_t)n_vars * n_new, hipMemcpyDeviceToHost));
  });
}

int pc_copy_runs(const double* d_src, double* d_dst, const int64_t* d_chunks, int64_t n_chunks, void* stream) {
  return guarded(g_err, [&] {
    if (n_chunks <= 0) return;
    if (!d_src || !d_dst || !d_chunks) throw std::runtime_error("null argument");
    hipLaunchKernelGGL(copy_runs_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, d_src, d_dst, d_chunks);
    HIP_OK(hipGetLastError());
  });
}

int pc_run_chunk(void) { return PC_RUN_CHUNK; }

int pc_mesh_error(pc_handle* h, int phase, const double* x, int n_orders, const int32_t* orders, const double* tabB,
                  const double* tabE, const double* tabA, double* max_rel, double* max_abs) {
  return guarded(g_err, [&] {
    require_device(h);
    if (phase < 0 || phase >= (int)h->pd.size()) throw std::runtime_error("phase out of range");
    auto& Q = h->Q;
    auto& P = Q.ph[phase];
    auto& D = *h->pd[phase];
    hipFunction_t fn = nullptr;
    const std::string name = "pc_mesh_err_p" + std::to_string(phase);
    HIP_OK(find_fn(h, &fn, name.c_str()));
    const pcs::MeshErrorPlan M =
        pcs::build_mesh_error_plan(P.K, P.n_k.data(), n_orders, orders, P.n_y, P.n_u, 256, h->lds_limit);
    DevBuf<int32_t> d_tile, d_lane;
    DevBuf<double> d_B, d_E, d_A, d_rel, d_abs;
    d_tile.upload(M.tile_k0);
    d_lane.upload(M.lane0);
    d_B.upload(std::vector<double>(tabB, tabB + M.tab_total_BE));
    d_E.upload(std::vector<double>(tabE, tabE + M.tab_total_BE));
    d_A.upload(std::vector<double>(tabA, tabA + M.tab_total_A));
    d_rel.alloc(P.K);
    d_abs.alloc((size_t)P.K * std::max(1, P.n_y));
    // (always through the device mirror; the callback cache no longer describes it afterwards)
    pcc::input_overwritten(h->cache);
    std::memcpy(h->h_in.p, x, Q.num_x * sizeof(double));
    HIP_OK(hipMemcpyAsync(h->d_in.p, h->h_in.p, Q.num_x * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PcRefineArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = fill_phase_view(h, phase, h->d_in.p);
    a.tile_k0 = d_tile.p;
    a.lane0 = d_lane.p;
    a.sec_h = D.sec_h.p;
    a.tabB = d_B.p;
    a.tabE = d_E.p;
    a.tabA = d_A.p;
    a.max_rel = d_rel.p;
    a.max_abs = d_abs.p;
    a.tab_total_BE = M.tab_total_BE;
    a.tab_total_A = M.tab_total_A;
    std::memcpy(a.offBE, M.offBE, sizeof(a.offBE));
    std::memcpy(a.offA, M.offA, sizeof(a.offA));
    launch_block(fn, M.n_tiles(), M.TB, M.lds_bytes, h->stream, a);
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipMemcpy(max_rel, d_rel.p, sizeof(double) * P.K, hipMemcpyDeviceToHost));
    if (max_abs && P.n_y > 0) HIP_OK(hipMemcpy(max_abs, d_abs.p, sizeof(double) * (size_t)P.K * P.n_y, hipMemcpyDeviceToHost));
  });
}

int pc_synchronize(pc_handle* h) {
  return guarded(g_err, [&] {
    require_device(h);
    HIP_OK(hipStreamSynchronize(h->stream));
    check_timeout(h);
  });
}

void* pc_stream(pc_handle* h) { return h ? (void*)h->stream : nullptr; }

int pc_read_symbol(pc_handle* h, const char* name, void* dst, size_t bytes) {
  return guarded(g_err, [&] {
    require_device(h);
    if (!name || !dst) throw std::runtime_error("null symbol name or destination");
    hipDeviceptr_t p = nullptr;
    size_t sz = 0;
    // "symbol@k": the copy in part k of a code object that comes in parts (every part has its own device globals)
    std::string sym(name);
    hipModule_t mod = h->module;
    if (const size_t at = sym.find('@'); at != std::string::npos) {
      const int k = std::atoi(sym.c_str() + at + 1);
      sym.resize(at);
      if (k < 0 || k > (int)h->more_modules.size()) throw std::runtime_error("no such part of the code object");
      if (k > 0) mod = h->more_modules[k - 1];
    }
    HIP_OK(hipModuleGetGlobal(&p, &sz, mod, sym.c_str()));
    if (bytes > sz) throw std::runtime_error("symbol is smaller than the requested read");
    HIP_OK(hipStreamSynchronize(h->stream));
    HIP_OK(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"

#include "pc_ipm.hpp"   // the device-resident interior-point state (same translation unit: it uses launch_all)
#include "pc_deriv_check.hpp"   // the derivative check (same translation unit: it uses launch_all)
#include "pc_solution_host.hpp"   // dense output of an NLP point (same translation unit: it uses find_fn and DevBuf)
