// The host rule behind the per-replica kernels (pc_eval_launch.hpp: check_replica_block, pcl::plan): a _w<W> kernel is
// compiled for a block of exactly 64 W threads and is planned with no other.  Hand-made shapes, no descriptor, no device:
// every line of the output is one case, "<case> ok <kernel> <block>" or "<case> refused <message>".
#include <cstdio>
#include <cstring>
#include <string>

#include "../../pycollo_amd/csrc/pc_eval_launch.hpp"

static double X[4], LAM[4], OUT[4];

static pcl::Call call() {
  pcl::Call c;
  c.x = X; c.lam = LAM; c.c = OUT; c.G = OUT; c.H = OUT; c.fobj = OUT;
  c.flags = PC_FLAG_C | PC_FLAG_G | PC_FLAG_H;
  return c;
}

// one resident launch of n_phases phases in blocks of tb * wpt threads; args_wpt: the waves per tile the argument block names
static void plan_case(const char* name, int n_phases, int tb, int wpt, int args_wpt, bool have_w) {
  pce::Shape S;
  S.TB = tb;
  S.resident = true;
  S.ph.resize(n_phases);
  S.wpt_all = wpt;
  pcl::Blocks B;
  B.n_phases = n_phases;
  B.bulk.resize(n_phases);
  B.merged.resize(n_phases);
  std::memset(&B.res, 0, sizeof(B.res));
  std::memset(&B.multi, 0, sizeof(B.multi));
  std::memset(&B.tail, 0, sizeof(B.tail));
  for (int ip = 0; ip < n_phases; ++ip) {
    S.ph[ip].wpt = wpt;
    S.ph[ip].n_tiles = 3;
    B.rg[ip].tile_begin = 0;
    B.rg[ip].tile_end = 3;
    std::memset(&B.bulk[ip], 0, sizeof(B.bulk[ip]));
    std::memset(&B.merged[ip], 0, sizeof(B.merged[ip]));
  }
  B.res.b.a.wpt = args_wpt;
  B.res.b.a.block_threads = tb * wpt;
  B.res.b.a.spt = 12;
  B.multi.m.first_block[PC_MAX_PHASES] = 3 * n_phases;
  B.multi.m.tail_blocks = 1;
  pcl::Have hv;
  hv.k[pcl::BULK_RES] = hv.k[pcl::BULK_ALL] = hv.k[pcl::BULK_ALL_RES] = true;
  hv.k[pcl::BULK_RES_W] = hv.k[pcl::BULK_ALL_RES_W] = have_w;
  try {
    const pcl::Plan p = pcl::plan(B, S, hv, call());
    std::printf("%s ok %d %u\n", name, (int)p.l[0].kernel, p.l[0].block);
  } catch (const std::exception& e) {
    std::printf("%s refused %s\n", name, e.what());
  }
}

static void rule_case(int wpt, int block) {
  try {
    pcl::check_replica_block(wpt, block);
    std::printf("rule_%d_%d ok\n", wpt, block);
  } catch (const std::exception& e) {
    std::printf("rule_%d_%d refused %s\n", wpt, block, e.what());
  }
}

int main() {
  std::printf("kernels %d %d %d %d\n", (int)pcl::BULK_RES, (int)pcl::BULK_RES_W, (int)pcl::BULK_ALL_RES, (int)pcl::BULK_ALL_RES_W);
  // one phase
  plan_case("single_w4", 1, 64, 4, 4, true);
  plan_case("single_w2", 1, 64, 2, 2, true);
  plan_case("single_w2_tb128", 1, 128, 2, 2, true);          // a block of 256 threads is not two waves
  plan_case("single_w4_args_w2", 1, 64, 4, 2, true);         // the block the kernel reads names another W than the launch
  plan_case("single_w2_tb128_plain", 1, 128, 2, 2, false);   // no per-replica kernel: the run-time body takes any block
  // several phases, the merged launch
  plan_case("merged_w2", 2, 64, 2, 2, true);
  plan_case("merged_w2_tb256", 2, 256, 2, 2, true);
  plan_case("merged_w2_tb256_plain", 2, 256, 2, 2, false);
  // the rule itself
  rule_case(2, 128);
  rule_case(4, 256);
  rule_case(1, 64);
  rule_case(4, 128);
  rule_case(2, 256);
  rule_case(2, 64);
  rule_case(0, 0);
  return 0;
}
