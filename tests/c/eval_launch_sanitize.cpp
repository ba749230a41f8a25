// CPU-only sanitizer harness for the evaluation's argument blocks and launch plan (TEST INFRASTRUCTURE).
//
// Compiles pc_eval_launch.hpp -- what the evaluation's kernels are handed and how they are launched -- with
// g++ -fsanitize=address,undefined, reads a descriptor in the text format of desc_reader.hpp, builds problem and shape,
// invents distinct device addresses, and follows a script of steps: which optional kernels the code object has, tile
// ranges, partials buffers, the epoch, (re)building the blocks, and calls.  For every launch of a call it prints the
// kernel, grid, block, LDS and argument size, the unpacked lead words, first_block, the tail-block fields, the epoch and
// last_launch, and reads every byte of the argument block it claims.  tests/test_eval_launch_cpu.py restates the rules
// and must arrive at the same lines.
//
//   usage: eval_launch_sanitize <desc.txt> <steps.txt> <out.txt>
//
// Made-up addresses: buffer number r starts at r << 32 (Addr's members in order from 1, then 13 per phase from 32 + 16 p);
// a caller's partials buffer of phase p is (0x700 + p) << 32; the call's x, lam, c, G, H, fobj, grad_nz are 0x100 .. 0x106
// << 32.  Pointers are printed as "<buffer>+<bytes>".
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "desc_reader.hpp"
#include "../../pycollo_amd/csrc/pc_eval_launch.hpp"

namespace {

template <class T>
T* fake(uint64_t region) {
  return reinterpret_cast<T*>(region << 32);
}
std::string show(const void* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  return std::to_string(v >> 32) + "+" + std::to_string(v & 0xffffffffull);
}

pcl::Addr addresses(size_t n_phases) {
  pcl::Addr A;
  A.qa = fake<double>(1);
  A.point_x = fake<int64_t>(2);
  A.point_V = fake<double>(3);
  A.point_r = fake<double>(4);
  A.W_end = fake<double>(5);
  A.tail_owned = fake<int64_t>(6);
  A.pt_hslot = fake<int64_t>(7);
  A.pt_hlocal = fake<int32_t>(8);
  A.erec = fake<unsigned long long>(9);
  A.hb_gran = fake<unsigned long long>(10);
  A.rec_slot = fake<int64_t>(11);
  A.rec_term = fake<int32_t>(12);
  A.timeout = fake<unsigned>(13);
  A.phase_args = fake<PcPhaseArgs>(14);
  A.trec = fake<PcTileRec>(15);
  for (size_t p = 0; p < n_phases; ++p) {
    const uint64_t b = 32 + 16 * p;
    A.ph[p] = pcl::PhaseAddr{fake<int32_t>(b), fake<int32_t>(b + 1), fake<int32_t>(b + 2), fake<double>(b + 3), fake<int64_t>(b + 4),
                             fake<int64_t>(b + 5), fake<int64_t>(b + 6), fake<int64_t>(b + 7), fake<int32_t>(b + 8), fake<double>(b + 9),
                             fake<double>(b + 10), fake<double>(b + 11), fake<unsigned long long>(b + 12)};
  }
  return A;
}

// every byte of the block a launch claims (an overrun of the storage behind it is the sanitizer's to report)
unsigned walk(const pcl::Launch& l) {
  unsigned sum = 0;
  const volatile unsigned char* p = static_cast<const unsigned char*>(l.args);
  for (size_t i = 0; i < l.arg_bytes; ++i) sum += p[i];
  return sum;
}

void print_phase_args(std::ostream& out, const char* tag, size_t ip, const PcPhaseArgs& a, const pcl::Addr& A) {
  out << tag << ' ' << ip << ' ' << a.tile_begin << ' ' << a.n_blocks << ' ' << a.wpt << ' ' << a.block_threads << ' ' << a.lds_out << ' '
      << show(a.partials) << ' ' << (a.tile_rec ? (long)(a.tile_rec - A.trec) : -1L) << ' ' << a.epoch << ' ' << a.flags << ' ' << a.uni_n
      << ' ' << a.spt << ' ' << a.n_tiles << ' ' << show(a.qa) << ' ' << show(a.qw) << ' ' << show(a.x) << ' ' << show(a.lam) << '\n';
}

void print_tail(std::ostream& out, const PcTailArgs& t, size_t n_phases) {
  out << "tail " << t.n_tail_blocks << ' ' << t.block_threads << ' ' << t.epoch << ' ' << t.flags << ' ' << t.sigma << ' ' << t.wJ << ' '
      << show(t.x) << ' ' << show(t.lam) << ' ' << show(t.c) << ' ' << show(t.G) << ' ' << show(t.H) << ' ' << show(t.fobj) << ' '
      << show(t.grad_nz);
  for (size_t ip = 0; ip < n_phases; ++ip) out << ' ' << show(t.ph[ip].partials) << ' ' << t.ph[ip].n_tiles;
  out << '\n';
}

void print_lead(std::ostream& out, const PcLead& l, const pcl::Call& c) {
  out << "lead " << (l.xz - c.x) << ' ' << (l.lamd ? (long)(l.lamd - c.lam) : -1L) << ' ' << show(l.qa) << ' ' << show(l.sec_h) << ' ' << l.N
      << ' ' << l.K << ' ' << l.tile_begin << ' ' << l.n_blocks << ' ' << pc_wa_flags(l.wa) << ' ' << pc_wa_wpt(l.wa) << ' '
      << pc_wa_block_threads(l.wa) << ' ' << pc_wa_spt(l.wa) << ' ' << pc_wa_tail_blocks(l.wa) << ' ' << pc_wb_qa_off(l.wb) << ' '
      << pc_wb_qw_abs(l.wb) << '\n';
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <desc.txt> <steps.txt> <out.txt>\n", argv[0]);
    return 2;
  }
  try {
    std::ifstream in(argv[1]);
    if (!in) throw std::runtime_error("cannot open descriptor");
    desc_reader::DescIn in_desc;
    desc_reader::read_desc(in, in_desc);
    pc_problem_desc& d = in_desc.d;
    std::vector<std::string> bulk_names;
    for (int ip = 0; ip < d.n_phases; ++ip) bulk_names.push_back("pc_bulk_p" + std::to_string(ip));
    for (int ip = 0; ip < d.n_phases; ++ip) in_desc.phases[ip].bulk_kernel = bulk_names[ip].c_str();
    d.tail_kernel = "pc_tail";
    pcp::Problem Q;
    pcp::from_desc(d, Q);
    const pce::Shape S = pce::build_shape(d, Q, in_desc.knobs);
    const size_t n = Q.ph.size();
    std::ofstream out(argv[3]);
    out << "shape " << S.TB << ' ' << S.wpt_all << ' ' << S.lds_all << ' ' << S.tail_blocks << ' ' << S.tail_blocks_all << ' '
        << S.tail_lds_bytes << ' ' << S.tail_big << ' ' << S.mixed << ' ' << S.resident << ' ' << S.qa_n << '\n';
    out << "sizes " << sizeof(PcLead) << ' ' << sizeof(PcPhaseArgs) << ' ' << sizeof(PcBulkArgs) << ' ' << sizeof(PcTailArgs) << ' '
        << sizeof(PcBulkTailArgs) << ' ' << sizeof(PcMultiArgs) << ' ' << sizeof(PcMultiTailArgs) << ' ' << sizeof(PcTailLead) << ' '
        << sizeof(PcTailLaunch) << '\n';
    for (size_t ip = 0; ip < n; ++ip)
      out << "phase " << S.ph[ip].n_tiles << ' ' << S.ph[ip].wpt << ' ' << S.ph[ip].lds_bytes << ' ' << S.ph[ip].lds_out << ' '
          << S.ph[ip].lds_out4 << ' ' << S.ph[ip].uni_n << ' ' << S.ph[ip].spt << ' ' << Q.ph[ip].x_off << ' ' << Q.ph[ip].c_off << ' '
          << S.qa_off[std::max(0, S.ph[ip].uni_n)] << ' ' << S.qw_off[std::max(0, S.ph[ip].uni_n)] << '\n';
    // scaling: distinct values, the sizes pc_set_scaling would give
    pcl::Scaling sc;
    sc.phase.resize(n);
    for (size_t ip = 0; ip < n; ++ip) {
      const auto& P = Q.ph[ip];
      sc.phase[ip].assign(2 * P.n_z + 2 * P.n_q + 4 + 2 * P.n_w + P.n_y + P.n_p + P.n_q, 1.0 + (double)ip);
    }
    sc.pointV.assign(Q.point_x.size(), 2.0);
    sc.pointr.assign(Q.point_x.size(), 0.5);
    sc.Wend.assign((size_t)Q.n_b, 3.0);
    sc.wJ = 0.25;
    pcl::Addr A = addresses(n);
    pcl::Range rg[PC_MAX_PHASES];
    for (size_t ip = 0; ip < n; ++ip) rg[ip].tile_end = S.ph[ip].n_tiles;
    pcl::Have hv;
    pcl::Blocks B;
    std::ifstream steps(argv[2]);
    if (!steps) throw std::runtime_error("cannot open steps");
    std::string line;
    while (std::getline(steps, line)) {
      std::istringstream ls(line);
      std::string op;
      if (!(ls >> op)) continue;
      if (op == "have") {   // BULK_RES BULK_RES_W BULK_ALL BULK_ALL_RES BULK_ALL_RES_W TAIL_BIG
        hv = pcl::Have{};
        for (pcl::Kernel k : {pcl::BULK_RES, pcl::BULK_RES_W, pcl::BULK_ALL, pcl::BULK_ALL_RES, pcl::BULK_ALL_RES_W, pcl::TAIL_BIG}) ls >> hv.k[k];
        out << "launches " << pcl::launches_per_evaluation(S, hv, n) << '\n';
      } else if (op == "range") {
        size_t ip = 0;
        ls >> ip;
        if (ip >= n) throw std::runtime_error("range: phase");
        ls >> rg[ip].tile_begin >> rg[ip].tile_end;
      } else if (op == "partials") {
        size_t ip = 0;
        int ext = 0;
        ls >> ip >> ext;
        if (ip >= n) throw std::runtime_error("partials: phase");
        rg[ip].partials_ext = ext ? fake<double>(0x700 + ip) : nullptr;
      } else if (op == "scal") {   // so many scaling doubles in phase 0 (the refusal)
        size_t count = 0;
        ls >> count;
        sc.phase[0].assign(count, 1.0);
      } else if (op == "epoch") {
        ls >> B.epoch;
      } else if (op == "build") {
        pcl::Records rec;
        if (S.mixed) {
          rec = pcl::launched_records(S, rg, n);
          out << "records " << rec.recs.size();
          for (size_t ip = 0; ip < n; ++ip) out << ' ' << rec.first[ip];
          out << '\n';
          for (const PcTileRec& r : rec.recs) out << "rec " << r.phase << ' ' << r.tile << ' ' << r.order << '\n';
        }
        try {
          pcl::build_blocks(B, Q, S, sc, rg, A, rec);
          out << "built\n";
        } catch (const std::runtime_error& e) {
          out << "refused " << e.what() << '\n';
        }
      } else if (op == "view") {   // PcPhaseView of a phase
        int ip = 0;
        ls >> ip;
        try {
          const PcPhaseView v = pcl::phase_view(Q, sc, A, ip, fake<double>(0x100));
          out << "view " << show(v.x) << ' ' << show(v.sec_s) << ' ' << v.x_off << ' ' << v.s_off << ' ' << v.N << ' ' << v.K << ' ' << v.scal[0] << '\n';
        } catch (const std::runtime_error& e) {
          out << "refused " << e.what() << '\n';
        }
      } else if (op == "call") {   // bulk tail flags with-lambda sigma
        pcl::Call c;
        int lam = 0;
        ls >> c.bulk >> c.tail >> c.flags >> lam >> c.sigma;
        c.x = fake<double>(0x100);
        c.lam = lam ? fake<double>(0x101) : nullptr;
        c.c = fake<double>(0x102); c.G = fake<double>(0x103); c.H = fake<double>(0x104);
        c.fobj = fake<double>(0x105); c.grad_nz = fake<double>(0x106);
        const pcl::Plan p = pcl::plan(B, S, hv, c);
        out << "call " << p.n << ' ' << p.last_launch << ' ' << B.epoch << '\n';
        if (p.n > PC_MAX_PHASES + 1) throw std::logic_error("plan past its capacity");
        for (int i = 0; i < p.n; ++i) {
          const pcl::Launch& l = p.l[i];
          const int wpt = (l.kernel == pcl::BULK_RES_W) ? S.ph[0].wpt : S.wpt_all;
          out << "launch " << pcl::kernel_name(Q, d.tail_kernel, l.kernel, l.phase, wpt) << ' ' << l.phase << ' ' << l.grid << ' ' << l.block
              << ' ' << l.lds << ' ' << l.arg_bytes << ' ' << (walk(l) >= 0u) << '\n';
          switch (l.kernel) {
            case pcl::BULK: {
              const PcBulkArgs& b = *static_cast<const PcBulkArgs*>(l.args);
              print_lead(out, b.lead, c);
              print_phase_args(out, "args", (size_t)l.phase, b.a, A);
              break;
            }
            case pcl::BULK_RES: case pcl::BULK_RES_W: {
              const PcBulkTailArgs& b = *static_cast<const PcBulkTailArgs*>(l.args);
              print_lead(out, b.b.lead, c);
              print_phase_args(out, "args", 0, b.b.a, A);
              print_tail(out, b.t, n);
              break;
            }
            case pcl::BULK_ALL: case pcl::BULK_ALL_RES: case pcl::BULK_ALL_RES_W: {
              const PcMultiArgs& m = *static_cast<const PcMultiArgs*>(l.args);
              out << "multi " << m.n_phases << ' ' << m.flags << ' ' << m.epoch << ' ' << m.tail_blocks << ' ' << show(m.trec) << ' ' << show(m.ph)
                  << ' ' << show(m.x) << ' ' << show(m.lam);
              for (int i2 = 0; i2 <= PC_MAX_PHASES; ++i2) out << ' ' << m.first_block[i2];
              out << '\n';
              for (size_t ip = 0; ip < n; ++ip) print_phase_args(out, "merged", ip, B.merged[ip], A);
              if (l.kernel != pcl::BULK_ALL) print_tail(out, static_cast<const PcMultiTailArgs*>(l.args)->t, n);
              break;
            }
            default: {
              const PcTailLaunch& t = *static_cast<const PcTailLaunch*>(l.args);
              out << "taillead " << show(t.lead.x) << ' ' << show(t.lead.partials0) << ' ' << show(t.lead.scal0) << ' ' << t.lead.x_off0 << ' '
                  << t.lead.n_tiles0 << ' ' << t.lead.N0 << ' ' << t.lead.flags << ' ' << t.lead.block_threads << '\n';
              print_tail(out, t.t, n);
            }
          }
        }
      } else if (op == "names") {   // every name the header can ask a code object for, given the shape's waves per tile
        for (size_t ip = 0; ip < n; ++ip) out << "name " << pcl::kernel_name(Q, d.tail_kernel, pcl::BULK, (int)ip, 1) << '\n';
        if (n == 1) out << "name " << pcl::kernel_name(Q, d.tail_kernel, pcl::BULK_RES, 0, 1) << '\n';
        if (n > 1)
          for (pcl::Kernel k : {pcl::BULK_ALL, pcl::BULK_ALL_RES}) out << "name " << pcl::kernel_name(Q, d.tail_kernel, k, 0, 1) << '\n';
        for (int w : {2, 4}) out << "name_w " << pcl::kernel_name(Q, d.tail_kernel, n > 1 ? pcl::BULK_ALL_RES_W : pcl::BULK_RES_W, 0, w) << '\n';
        for (pcl::Kernel k : {pcl::TAIL, pcl::TAIL_BIG}) out << "name " << pcl::kernel_name(Q, d.tail_kernel, k, 0, 1) << '\n';
      } else if (op == "words") {   // flags wpt block_threads spt tail_blocks qa_off qw_abs: pack, unpack, and the run-time check
        int f = 0, w = 0, bt = 0, spt = 0, ntb = 0, qa = 0, qw = 0;
        ls >> f >> w >> bt >> spt >> ntb >> qa >> qw;
        const bool fits = pc_lead_wa_fits(w, bt, spt, ntb) && pc_lead_wb_fits(qa, qw);
        out << "words " << fits;
        if (fits) {
          const int32_t wa = pc_lead_wa(f, w, bt, spt, ntb), wb = pc_lead_wb(qa, qw);
          out << ' ' << pc_wa_flags(wa) << ' ' << pc_wa_wpt(wa) << ' ' << pc_wa_block_threads(wa) << ' ' << pc_wa_spt(wa) << ' '
              << pc_wa_tail_blocks(wa) << ' ' << pc_wb_qa_off(wb) << ' ' << pc_wb_qw_abs(wb);
        }
        out << '\n';
      } else if (op == "check") {   // check_lead on phase 0's block with fields set beyond their range: wpt block_threads spt tail_blocks
        PcPhaseArgs a = B.bulk.at(0).a;
        int ntb = 0;
        ls >> a.wpt >> a.block_threads >> a.spt >> ntb;
        try {
          pcl::check_lead(a, ntb);
          out << "check ok\n";
        } catch (const std::runtime_error& e) {
          out << "check refused\n";
        }
      } else {
        throw std::runtime_error("unknown step " + op);
      }
    }
    out << "ok\n";
    return out ? 0 : 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "eval_launch_sanitize: %s\n", e.what());
    return 1;
  }
}
