// CPU check of the launch plan (csrc/tsamd_plan.h): which kernel family a context runs and on what geometry.
//   launch_plan_check            asserts the figures the GPU tests pin (tests/test_gpu_geometry.py and friends) on a
//                                device of 256 compute units where every kernel fits (first pass: 2 per unit at K <= 8)
//   launch_plan_check --replay   reads one line of plan inputs per context from stdin and prints what the ABI would
//                                report for it (tests/test_launch_plan_cpu.py compares that with the recorded fixture)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "tsamd_plan.h"

using namespace tsamd;

namespace {

int g_failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++g_failures;                                               \
    }                                                             \
  } while (0)

PlanInputs one_gpu(uint32_t n, uint32_t k) {
  PlanInputs in;
  in.n = n;
  in.k = k;
  in.max_inner = 10;
  in.cus = 256;
  if (k <= (uint32_t)TSAMD_SPECIALIZED_K) {
    in.occ.first[0] = in.occ.first[1] = k <= 8 ? 2 : 1;
    in.occ.resident = in.occ.schedule = in.occ.holblock = in.occ.hybrid = in.occ.hybhol = 1;
  }
  return in;
}

void pinned_figures() {
  // SHRUNK of tests/test_gpu_geometry.py: (n, k) -> workgroups x individuals per thread, one exchange level
  const uint32_t shrunk[][4] = {{10000, 6, 20, 2}, {10000, 8, 20, 2}, {16000, 8, 32, 2}, {20000, 3, 27, 3}};
  for (const auto &s : shrunk) {
    const LaunchPlan pl = plan_launch(one_gpu(s[0], s[1]));
    CHECK(pl.mode == TSAMD_LAUNCH_PER_SCHEDULE && pl.family == kFamSchedule);
    CHECK(pl.schedule.grid == s[2] && pl.schedule.indivs_per_thread == s[3] && pl.schedule.exchange_levels == 1u);
  }
  // ONE_WG: one workgroup exchanges nothing
  const uint32_t one_wg[][3] = {{1500, 8, 6}, {3000, 4, 12}, {200, 3, 2}};
  for (const auto &s : one_wg) {
    const LaunchPlan pl = plan_launch(one_gpu(s[0], s[1]));
    CHECK(pl.schedule.grid == 1u && pl.schedule.indivs_per_thread == s[2] && pl.schedule.exchange_levels == 0u);
  }
  {  // the register capacity at K = 8
    const LaunchPlan pl = plan_launch(one_gpu(1048576, 8));
    CHECK(pl.schedule.grid == 256u && pl.schedule.indivs_per_thread == 16u && pl.schedule.exchange_levels == 2u && pl.schedule.on_chip_per_thread == 16u);
    CHECK(pl.family == kFamSchedule && pl.batch_validation);
  }
  {
    const LaunchPlan pl = plan_launch(one_gpu(100000, 8));
    CHECK(pl.schedule.indivs_per_thread == 2u && pl.schedule.exchange_levels == 2u && pl.schedule.grid >= 190u && pl.schedule.grid <= 200u);
  }
  {  // the run-time-K fallback has no resident mode
    const LaunchPlan pl = plan_launch(one_gpu(100000, 40));
    CHECK(pl.wide && pl.qualified == TSAMD_LAUNCH_PER_PASS && !pl.qualifies(TSAMD_LAUNCH_PER_SNP) && !pl.qualifies(TSAMD_LAUNCH_PER_SCHEDULE));
  }
  // ts_resident has one level only up to 16 workgroups at K <= 8
  for (uint32_t k : {3u, 8u, 9u, 20u})
    for (uint32_t n : {2000u, 4000u, 8000u, 10000u, 16000u, 20000u, 60000u}) {
      const LaunchPlan pl = plan_launch(one_gpu(n, k));
      CHECK(pl.qualifies(TSAMD_LAUNCH_PER_SNP));
      if (pl.snp.exchange_levels == 1u) CHECK(k <= 8u && pl.snp.grid <= 16u && pl.snp.grid > 1u);
      if (pl.snp.grid > 16u || (k > 8u && pl.snp.grid > 1u)) CHECK(pl.snp.exchange_levels == 2u);
    }
  {  // TSAMD_SCHED_WORKGROUPS=64
    PlanInputs in = one_gpu(60000, 8);
    const LaunchPlan dflt = plan_launch(in);
    in.knobs.sched_workgroups = 64;
    const LaunchPlan pl = plan_launch(in);
    CHECK(pl.schedule.grid <= 64u && pl.schedule.indivs_per_thread > dflt.schedule.indivs_per_thread);
  }
  {  // a shard above the register capacity: ts_hybrid, no launch-per-SNP mode; its capacity and TSAMD_HYBRID=0
    PlanInputs in = one_gpu(400000, 20);
    LaunchPlan pl = plan_launch(in);
    CHECK(pl.family == kFamHybrid && pl.mode == TSAMD_LAUNCH_PER_SCHEDULE && !pl.qualifies(TSAMD_LAUNCH_PER_SNP));
    CHECK(pl.schedule.on_chip_per_thread == std::min<uint32_t>(pl.schedule.indivs_per_thread, (uint32_t)(hy_reg_items(20) + hy_lds_items(20))));
    in.knobs.hybrid = 0;
    CHECK(plan_launch(in).qualified == TSAMD_LAUNCH_PER_PASS);
  }
  {  // every rank of a world reaches the same verdict; too small a shard, more than 4 ranks for ts_hybrid, TSAMD_GRID stay per pass
    for (uint32_t world : {2u, 3u, 4u, 8u})
      for (uint32_t n : {1800u, 40000u, 1000000u, 3000000u}) {
        int verdict = -1, family = -1;
        for (uint32_t r = 0; r < world; ++r) {
          PlanInputs in = one_gpu(n, 20);
          in.world = world;
          in.rank = r;
          in.exchange = Exchange::kP2p;
          const LaunchPlan pl = plan_launch(in);
          if (r == 0) verdict = pl.qualified, family = pl.family;
          CHECK(pl.qualified == verdict && (int)pl.family == family && !pl.qualifies(TSAMD_LAUNCH_PER_SNP));
          CHECK(pl.qualified == TSAMD_LAUNCH_PER_PASS || pl.schedule.grid >= (uint32_t)kResGroups);
        }
        if (n == 1800u) CHECK(verdict == TSAMD_LAUNCH_PER_PASS);
        if (n == 40000u) CHECK(verdict == TSAMD_LAUNCH_PER_SCHEDULE && family == kFamSchedule);
        if (n == 3000000u) CHECK(world <= 4u ? (verdict == TSAMD_LAUNCH_PER_SCHEDULE && family == kFamHybrid) : verdict == TSAMD_LAUNCH_PER_PASS);
      }
    PlanInputs in = one_gpu(100000, 8);
    in.knobs.grid = 64;
    CHECK(plan_launch(in).qualified == TSAMD_LAUNCH_PER_PASS);
  }
}

int replay() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    PlanInputs in;
    int exchange = 0;
    long long kn[9];
    const int got = sscanf(line,
                           "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %lf %" SCNu32 " %d %" SCNu32 " %d %" SCNu32
                           " %d %d %d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld",
                           &in.n, &in.k, &in.world, &in.rank, &in.max_inner, &in.nodekappa, &in.flags, &in.cus, &in.device_share, &exchange,
                           &in.pass_grid_cap, &in.occ.first[0], &in.occ.first[1], &in.occ.resident, &in.occ.schedule, &in.occ.holblock,
                           &in.occ.hybrid, &in.occ.hybhol, &kn[0], &kn[1], &kn[2], &kn[3], &kn[4], &kn[5], &kn[6], &kn[7], &kn[8]);
    if (got != 27) {
      fprintf(stderr, "bad input line (%d fields): %s", got, line);
      return 2;
    }
    in.exchange = exchange == 2 ? Exchange::kP2p : exchange == 1 ? Exchange::kRccl : Exchange::kNone;
    uint32_t *knob[9] = {&in.knobs.block,      &in.knobs.grid,   &in.knobs.grid_first,       &in.knobs.first_vec,          &in.knobs.resident,
                         &in.knobs.persistent, &in.knobs.hybrid, &in.knobs.sched_workgroups, &in.knobs.test_max_workgroups};
    for (int i = 0; i < 9; ++i)
      if (kn[i] >= 0) *knob[i] = (uint32_t)kn[i];  // (negative: the variable is not set)
    const LaunchPlan pl = plan_launch(in);
    // batch: what tsamd_holblock_info reports in the mode in force (-1: ts_hybhol's, which its kernel header defines)
    const int batch = (pl.mode == TSAMD_LAUNCH_PER_SCHEDULE && pl.batch_validation) ? (pl.family == kFamHybrid ? -1 : hol_batch((int)in.k)) : 0;
    printf("%u %u %u", kernels_per_snp(pl.mode, in.max_inner), pl.grid, pl.grid_first);
    for (const ResidentGeometry *g : {&pl.snp, &pl.schedule})
      printf(" %u %u %u %u", g->grid, g->indivs_per_thread, g->exchange_levels, g->on_chip_per_thread);
    printf(" %d %d\n", batch, (int)pl.family);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--replay") == 0) return replay();
  pinned_figures();
  printf("launch plan: %d failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
