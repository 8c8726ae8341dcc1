// The launch plan: which kernel family a context runs and on what geometry, as ONE pure function of the facts it depends
// on.  Host-only C++17 without a HIP include (tests/launch_plan_check.cpp compiles it with g++); csrc/tsamd.hip gathers the
// facts -- configuration, device, occupancy answers, environment -- and keeps the LaunchPlan this returns.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "tsamd.h"
#include "tsamd_capacity.h"

namespace tsamd {

// [begin, begin + count) of `rank`'s shard (tsamd_shard_range of the ABI)
inline void shard_range(uint32_t n, uint32_t rank, uint32_t world, uint32_t *begin, uint32_t *count) {
  if (world == 0) world = 1;
  uint64_t per = ((uint64_t)n + world - 1) / world;
  per = (per + 3) / 4 * 4;
  uint64_t b = std::min<uint64_t>((uint64_t)rank * per, n);
  uint64_t e = std::min<uint64_t>(b + per, n);
  if (begin) *begin = (uint32_t)b;
  if (count) *count = (uint32_t)(e - b);
}
// every rank pads to the same width, so that all ranks run the same launch geometry
inline uint32_t padded_width(uint32_t n, uint32_t rank, uint32_t world) {
  uint32_t b = 0, cnt = 0, b0 = 0, width = 0;
  shard_range(n, rank, world, &b, &cnt);
  shard_range(n, 0, world, &b0, &width);
  return (std::max(width, cnt) + 511u) / 512u * 512u;
}

// Snapshot of the environment variables that shape the plan (read_knobs() in csrc/tsamd.hip is the only reader).
constexpr uint32_t kKnobUnset = 0xffffffffu;  // (a variable that is set parses to at most 2^31 - 1)
struct Knobs {
  uint32_t block = kKnobUnset;       // TSAMD_BLOCK
  uint32_t grid = kKnobUnset;        // TSAMD_GRID
  uint32_t grid_first = kKnobUnset;  // TSAMD_GRID_FIRST
  uint32_t first_vec = 1;            // TSAMD_FIRST_VEC
  uint32_t resident = 1;             // TSAMD_RESIDENT
  uint32_t persistent = 1;           // TSAMD_PERSISTENT
  uint32_t hybrid = 1;               // TSAMD_HYBRID
  uint32_t sched_workgroups = 0;     // TSAMD_SCHED_WORKGROUPS
  uint32_t test_max_workgroups = 0;  // TSAMD_TEST_MAX_WORKGROUPS (honoured with TSAMD_FLAG_TEST_HOOKS only)
};

// the exchange in force between the ranks' passes
enum class Exchange { kNone, kRccl, kP2p };
// whole-launch kernel families (index of the kernel table in csrc/tsamd.hip): a context's whole-schedule kernel is
// ts_schedule or ts_hybrid, its batched validation form ts_holblock or ts_hybhol
enum Family { kFamSchedule = 0, kFamHolblock = 1, kFamHybrid = 2, kFamHybhol = 3, kFamilies = 4 };
constexpr Family batched_form(Family f) { return f == kFamHybrid ? kFamHybhol : kFamHolblock; }

// workgroups of a kernel per compute unit, worst case of its instantiations for this K (0: it does not fit; K above
// TSAMD_SPECIALIZED_K: all 0)
struct Occupancy {
  int first[2] = {0, 0};  // first pass, by TSAMD_FIRST_VEC - 1
  int resident = 0, schedule = 0, holblock = 0, hybrid = 0, hybhol = 0;
};

struct PlanInputs {
  uint32_t n = 0, k = 0, world = 1, rank = 0, max_inner = 0;  // from the configuration
  double nodekappa = 0.5;
  uint32_t flags = 0;
  int cus = 0;                  // compute units of the device (0: unknown)
  uint32_t device_share = 1;    // contexts whose resident kernels share this device (tests: several ranks on one GPU)
  Exchange exchange = Exchange::kNone;
  uint32_t pass_grid_cap = 0;   // at most this many pass-kernel workgroups (0: what the exchange allows); the replay after a failed launch sets it
  Occupancy occ;
  Knobs knobs;
};

// launch geometry of a resident kernel and what tsamd_schedule_geometry reports of it; grid == 0: the context does not qualify
struct ResidentGeometry {
  uint32_t grid = 0, chunk = 0;
  uint32_t indivs_per_thread = 0, exchange_levels = 0, on_chip_per_thread = 0;
};

struct LaunchPlan {
  int qualified = TSAMD_LAUNCH_PER_PASS;  // the highest launch mode the context qualifies for ...
  int mode = TSAMD_LAUNCH_PER_PASS;       // ... and the one in force (tsamd_set_launch_mode, recovery)
  Family family = kFamSchedule;           // the whole-schedule kernel: ts_hybrid when the shard exceeds ts_schedule's register capacity
  bool batch_validation = false;          // validation-mode schedules run batched (batched_form(family)) in TSAMD_LAUNCH_PER_SCHEDULE
  bool split = false;         // lambda_t leaves the pass via ctl->lt and the epilogue is its own kernel
  bool wide = false;          // K above TSAMD_SPECIALIZED_K: run-time-K fallback kernels (tsamd_wide_kernels.h)
  uint32_t rows_from_lt = 0;  // DevParams::rows_from_lt
  uint32_t grid = 0, block = 256, grid_first = 0, first_vec = 1, chunk = 0, chunk_first = 0;  // plain-pass and first-pass launch geometry
  ResidentGeometry snp;       // ts_resident: the same shard as `schedule`, shrunk only as far as ITS exchange has one level
  ResidentGeometry schedule;  // ts_schedule / ts_hybrid (its own geometry when sharded)
  bool qualifies(int m) const {
    return m == TSAMD_LAUNCH_PER_PASS || (m == TSAMD_LAUNCH_PER_SNP && snp.grid != 0u) || (m == TSAMD_LAUNCH_PER_SCHEDULE && schedule.grid != 0u);
  }
  // in mode m the plain passes of a SNP outside a whole-schedule launch run as ts_resident
  bool resident_passes(int m) const { return m >= TSAMD_LAUNCH_PER_SNP && snp.grid != 0u; }
};

// kernels of the state-machine sequence per SNP (ts_reduce_rows shares its pass' parity); 0: the schedule is one launch
inline uint32_t kernels_per_snp(int mode, uint32_t max_inner) {
  return mode == TSAMD_LAUNCH_PER_SCHEDULE ? 0u : mode == TSAMD_LAUNCH_PER_SNP ? 2u : max_inner;
}

namespace plan_detail {

// Launch geometry of the resident kernels for a shard of `npad` padded individuals on at most `cap` workgroups (all
// resident at once): items of resident_vec(K) individuals, a whole number of 256-thread rounds per workgroup.  False
// when the shard does not fit resident_items(K) items per thread.
// one_level: up to this many workgroups the kernel that will run exchanges in ONE level (ts_schedule: kResOneLevelGrid;
// ts_resident: 16 at K <= 8, never above -- its sweep's registers leave no room for the wider form).
inline bool resident_geometry(uint32_t k, uint32_t npad, uint32_t cap, uint32_t *grid, uint32_t *chunk, bool one_gpu, uint32_t one_level) {
  if (cap == 0u || npad == 0u || (int)k > kResidentMaxK) return false;
  const uint32_t nitems = npad / (uint32_t)resident_vec((int)k);
  auto rounds = [&](uint32_t workgroups) {
    const uint32_t ch = (nitems + workgroups - 1u) / workgroups;
    return (ch + (uint32_t)kResidentBlock - 1u) / (uint32_t)kResidentBlock;
  };
  uint32_t r = rounds(cap);
  // (a sharded launch -- one_gpu false -- holds sharded_items(K) items per thread: one fewer than resident_items(K) at K = 14 and 16)
  if (r > (uint32_t)(one_gpu ? resident_items((int)k) : sharded_items((int)k))) return false;
  // Small shards on one GPU: up to kResOneLevelGrid workgroups exchange in ONE level (1.9 us against 3.0 per pass), which is
  // worth a few more individuals per thread -- each costs about 0.33 K us per update (gamma step + ten sweeps), the nine
  // shorter exchanges save about 10 (profiles/r03_experiments.md)
  if (one_gpu && one_level > 0u && (nitems + r * (uint32_t)kResidentBlock - 1u) / (r * (uint32_t)kResidentBlock) > one_level) {
    const uint32_t r1 = rounds(one_level);
    if (r1 <= (uint32_t)resident_items((int)k) && (r1 - r) * k < 20u) r = r1;  // (measured with a threshold of 16: K = 8, N = 10 000: 39.0 against 43.7 us per update; K = 20, N = 8 000 would lose)
  }
  // ... and the smallest cohorts on ONE workgroup, which exchanges nothing at all (a pass is then a sweep, a fold and an
  // epilogue: about 1 us), when its extra individuals per thread cost less than the exchanges they replace
  if (one_gpu) {
    const uint32_t r0 = rounds(1u);
    if (r0 <= (uint32_t)resident_items((int)k) && (r0 - r) * k < 50u) r = r0;
  }
  *chunk = r * (uint32_t)kResidentBlock;
  *grid = (nitems + *chunk - 1u) / *chunk;
  return true;
}

// Launch geometry of ts_hybrid for a shard above ts_schedule's capacity: all `cap` workgroups, a whole number of 256-thread
// rounds each; the first hy_reg_items(K) + hy_lds_items(K) rounds of a workgroup stay on chip, the rest is streamed.
inline bool hybrid_geometry(uint32_t k, uint32_t npad, uint32_t cap, uint32_t *grid, uint32_t *chunk) {
  if (cap == 0u || npad == 0u || (int)k > kResidentMaxK) return false;
  // (the kernel is bound by memory: ALL `cap` workgroups take an equal share -- a multiple of 16 individuals, i.e. of a column
  // word and of 128 bytes of a weight row -- rather than whole 256-thread rounds on fewer workgroups; a workgroup's last round
  // is then partly filled)
  const uint32_t ch = ((npad + cap - 1u) / cap + 15u) / 16u * 16u;
  const uint32_t r = (ch + (uint32_t)kResidentBlock - 1u) / (uint32_t)kResidentBlock;
  if (r > (uint32_t)(hy_reg_items((int)k) + hy_lds_items((int)k) + kHybridMaxStreamed)) return false;
  *chunk = ch;
  *grid = (npad + ch - 1u) / ch;
  return true;
}

// Launch geometry of the pass kernels.  The pass kernel is a streaming reduction: enough waves per CU to cover
// HBM latency, but few workgroups, because every workgroup of the NEXT launch adds all
// partial rows up again (and, sharded peer-to-peer, every workgroup sends its row to every
// rank: max_grid = kXchgBlocks there).
inline void pass_geometry(const PlanInputs &in, uint32_t npad, uint32_t max_grid, LaunchPlan *pl) {
  const Knobs &kn = in.knobs;
  const uint32_t npairs = npad / 2u;
  if (pl->wide) {  // one individual per thread, at most kWideItems individuals per thread
    uint32_t chunk = (npad + max_grid - 1) / max_grid;
    chunk = (chunk + kWideBlock - 1) / kWideBlock * kWideBlock;
    pl->chunk_first = pl->chunk = chunk;
    pl->grid_first = pl->grid = (npad + chunk - 1) / chunk;
    pl->block = kWideBlock;
    return;
  }
  uint32_t block = kn.block != kKnobUnset ? kn.block : (in.k <= 16 && npairs >= 256u * 1024u) ? 512u : 256u;
  if (block != 256u && block != 512u && block != 1024u) block = 256u;
  if (block == 1024u && in.k > 8) block = 512u;  // register budget of the pipelined loop
  auto geometry = [&](uint32_t nitems, uint32_t blk, uint32_t target, uint32_t &chunk, uint32_t &grid) {
    target = std::min<uint32_t>(std::max<uint32_t>(target, 1u), max_grid);
    chunk = (nitems + target - 1) / target;
    chunk = (chunk + blk - 1) / blk * blk;
    grid = (nitems + chunk - 1) / chunk;
  };
  pl->block = block;
  pl->first_vec = kn.first_vec == 2 ? 2 : 1;
  // Ranks that SHARE one device (tests, rehearsals: TSAMD_DEVICE_SHARE=<ranks>): a pass kernel of the peer-to-peer sequence
  // spins in its prologue until every rank's rows of the previous pass have arrived, so all ranks' kernels must fit the
  // device together -- a first pass that fills every compute unit (it is register-bound: one workgroup per unit from K = 12
  // on) would keep its peers' previous passes off the device until its bounded wait gives up (4 ranks x 250 000 individuals,
  // K = 20: "timed out waiting for a peer (epoch 2)").  Each rank gets its share of the workgroups.  One rank per device: 1.
  const uint32_t share = std::max<uint32_t>(1u, in.device_share);
  geometry(npairs, block, kn.grid != kKnobUnset ? kn.grid : share > 1u ? std::max<uint32_t>(8u, 256u / share) : 256u, pl->chunk, pl->grid);
  // first pass: exactly as many workgroups as are resident at once (one round; the kernel is
  // register-bound, so that is 2 per compute unit at K = 8 and 1 from K = 12 on)
  uint32_t first_target = 512;
  const int nb = in.occ.first[pl->first_vec - 1u];
  if (nb > 0 && in.cus > 0) first_target = (uint32_t)in.cus * (uint32_t)std::min(nb, 4);
  if (share > 1u) first_target = std::max<uint32_t>(8u, std::min<uint32_t>(first_target, 256u) / share);
  geometry(npad / pl->first_vec, 256, kn.grid_first != kKnobUnset ? kn.grid_first : first_target, pl->chunk_first, pl->grid_first);
}

// what tsamd_schedule_geometry reports of a resident launch; one_level as for resident_geometry
inline void describe(const PlanInputs &in, uint32_t one_level, bool hybrid, ResidentGeometry *g) {
  g->indivs_per_thread = (g->chunk + (uint32_t)kResidentBlock - 1u) / (uint32_t)kResidentBlock * (uint32_t)resident_vec((int)in.k);
  g->exchange_levels = (g->grid == 1u && in.world == 1u) ? 0u : (in.world == 1u && g->grid <= one_level) ? 1u : 2u;
  g->on_chip_per_thread = hybrid ? std::min<uint32_t>(g->indivs_per_thread, (uint32_t)(hy_reg_items((int)in.k) + hy_lds_items((int)in.k))) : g->indivs_per_thread;
}

}  // namespace plan_detail

// The decision.  `mode` of the result is the highest mode the context qualifies for.
inline LaunchPlan plan_launch(const PlanInputs &in) {
  using namespace plan_detail;
  const Knobs &kn = in.knobs;
  LaunchPlan pl;
  const bool p2p = in.exchange == Exchange::kP2p;
  const uint32_t npad = padded_width(in.n, in.rank, in.world);
  pl.wide = in.k > TSAMD_SPECIALIZED_K;
  pl.split = in.world > 1u || (in.flags & TSAMD_FLAG_SPLIT_EPILOGUE) || in.exchange != Exchange::kNone;
  pl.rows_from_lt = (pl.split && !p2p) ? 1u : 0u;  // (peer-to-peer: the rows arrive in the exchange buffer)
  // (peer-to-peer: every workgroup of the next launch polls all flags and re-adds all rows of all ranks)
  const uint32_t xchg_grid = p2p ? std::max<uint32_t>(16u, std::min<uint32_t>(kXchgBlocks, 512u / in.world)) : (uint32_t)kMaxGrid;
  pass_geometry(in, npad, in.pass_grid_cap ? in.pass_grid_cap : xchg_grid, &pl);

  // ---- the resident kernels: every qualification condition, once ---------------------------------------------------
  // K <= 32, a pass cap the kernels' counters hold, and then
  //   ts_resident (one GPU): the shard's weights fit the register file (resident_items(K) items per thread of a 256-thread
  //     workgroup) and every workgroup can be resident at once -- which the kernels verify for themselves at the start of
  //     every launch;
  //   ts_schedule: the same with the reference's default learning-rate exponent (the kernel carries no pow());
  //   ts_hybrid: a shard above that capacity -- the same one-launch structure with part of the weights in LDS and the rest
  //     streamed instead of ten launches per update.
  const bool snp_ok = !pl.wide && in.max_inner >= 2u && in.max_inner <= 200u && kn.resident != 0u;
  const bool schedule_ok = snp_ok && in.nodekappa == 0.5 && kn.persistent != 0u;
  const bool hybrid_ok = schedule_ok && kn.hybrid != 0u && in.occ.hybrid >= 1;
  const uint32_t full = (uint32_t)(kResGroups * kResMembers);
  // (ts_resident<K> instantiates its exchange with one level up to 16 workgroups at K <= 8 and never above)
  const uint32_t snp_one_level = in.k <= 8u ? 16u : 0u;
  bool hybrid = false;
  if (in.exchange == Exchange::kNone && !pl.split) {
    // One GPU.
    int cus = in.cus;
    // (test hook: fewer workgroups than the device holds, so that small shards exercise the many-items-per-thread paths --
    // ts_hybrid's LDS and streamed items for every K -- at a size the oracle finishes in a moment)
    if ((in.flags & TSAMD_FLAG_TEST_HOOKS) && kn.test_max_workgroups > 0u) cus = std::min<int>(cus, (int)kn.test_max_workgroups);
    // (tuning knob, round 6's geometry sweep: at most this many workgroups for the resident kernels -- fewer members per exchange
    // group against more individuals per thread; profiles/r06_experiments.md.  Every rank of a sharded run must see the same value)
    if (kn.sched_workgroups >= (uint32_t)kResGroups) cus = std::min<int>(cus, (int)kn.sched_workgroups);
    const uint32_t cap = std::min<uint32_t>(full, (uint32_t)std::max(cus, 0));
    // (TSAMD_GRID / TSAMD_BLOCK shape the launch-per-pass kernels: a context TSAMD_GRID is set for runs those)
    const bool shaped = kn.grid != kKnobUnset && kn.grid != 0u;
    ResidentGeometry sched, snp;
    if (!pl.wide && cap > 0u && !shaped) {
      if (resident_geometry(in.k, npad, cap, &sched.grid, &sched.chunk, true, (uint32_t)kResOneLevelGrid)) {
        if (snp_ok && in.occ.resident >= 1) {
          resident_geometry(in.k, npad, cap, &snp.grid, &snp.chunk, true, snp_one_level);
          pl.snp = snp;
          if (schedule_ok && in.occ.schedule >= 1) pl.schedule = sched;
        }
      } else if (hybrid_ok && hybrid_geometry(in.k, npad, cap, &sched.grid, &sched.chunk)) {
        pl.schedule = sched;
        hybrid = true;
      }
    }
  } else if (p2p && schedule_ok && in.world <= 8u && in.occ.schedule >= 1 && in.cus > 0) {
    // ts_schedule on a shard: one launch per rank and schedule, weights resident, level 2 of the in-launch exchange across
    // the ranks (Xchg::res_sums).  Every rank must reach the same verdict, so it depends only on the configuration: up to 8
    // ranks, the reference's default learning-rate exponent, every rank's shard fits the register file of at most
    // min(256, CUs / device_share) workgroups and fills at least 8 of them (all 8 groups of every rank then post a sum).
    // (ranks sharing a device: the dispatcher deals a launch's workgroups round robin over the 8 XCDs, every rank's launch starting at the
    // same one, so a rank may take floor(compute units per XCD / ranks) per XCD -- 3 ranks: 80 workgroups each, not 256 / 3 = 85, which put 33
    // workgroups on five XCDs of 32 compute units and lost the launch to the co-residency check: every 3-rank ts_hybrid test of round 5 in fact ran
    // its replay.  One rank per device: all compute units.)
    const uint32_t per_xcd = (uint32_t)in.cus / (uint32_t)kResGroups;
    uint32_t cap = std::min<uint32_t>(full, in.device_share > 1u ? (uint32_t)kResGroups * (per_xcd / in.device_share) : (uint32_t)in.cus);
    if (kn.sched_workgroups >= (uint32_t)kResGroups) cap = std::min<uint32_t>(cap, kn.sched_workgroups);  // (tuning knob, see above)
    // first ts_schedule on every rank; if a rank's shard exceeds its register capacity, ts_hybrid on every rank (up to 4 ranks:
    // the instantiations tsamd_hyb.hip carries)
    for (int attempt = 0; attempt < 2 && cap >= (uint32_t)kResGroups; ++attempt) {
      hybrid = attempt == 1;
      if (hybrid && (in.world > 4u || !hybrid_ok)) break;
      bool ok = true, too_big = false;
      ResidentGeometry mine;
      for (uint32_t r = 0; r < in.world && ok; ++r) {
        uint32_t b = 0, cnt = 0, grid = 0, chunk = 0;
        shard_range(in.n, r, in.world, &b, &cnt);
        const uint32_t npad_r = (cnt + 511u) / 512u * 512u;
        const bool fits = hybrid ? hybrid_geometry(in.k, npad_r, cap, &grid, &chunk) : resident_geometry(in.k, npad_r, cap, &grid, &chunk, false, 0u);
        too_big = too_big || (!fits && cnt != 0u);
        ok = fits && grid >= (uint32_t)kResGroups;
        if (r == in.rank) {
          mine.grid = grid;
          mine.chunk = chunk;
        }
      }
      if (ok) {
        pl.schedule = mine;
        break;
      }
      // ts_hybrid is for shards ABOVE the register capacity.  A shard too SMALL to fill 8 workgroups (up to ~1 800 individuals:
      // not every group of every rank would post a sum) stays with one launch per pass and the peer-to-peer rows -- an
      // untuned hybrid geometry of 16 individuals per workgroup is not what such a run should get (advisor, round 4)
      if (!too_big) break;
    }
  }
  // (a sharded context -- RCCL, or no exchange chosen yet -- runs one launch per pass)
  if (pl.snp.grid) describe(in, snp_one_level, false, &pl.snp);
  if (pl.schedule.grid) {
    pl.family = hybrid ? kFamHybrid : kFamSchedule;
    describe(in, (uint32_t)kResOneLevelGrid, hybrid, &pl.schedule);
    // validation-mode schedules run batched (one GPU, or on every rank alike: level 2 of the wide exchange in Xchg::res_wide):
    // ts_holblock while the context runs ts_schedule, ts_hybhol while it runs ts_hybrid
    pl.batch_validation = (hybrid ? in.occ.hybhol : in.occ.holblock) >= 1;
  }
  pl.qualified = pl.schedule.grid ? TSAMD_LAUNCH_PER_SCHEDULE : pl.snp.grid ? TSAMD_LAUNCH_PER_SNP : TSAMD_LAUNCH_PER_PASS;
  pl.mode = pl.qualified;
  return pl;
}

}  // namespace tsamd
