// Capacity constants of the kernels that the HOST's launch decision needs as well (tsamd_plan.h): what a thread, a
// workgroup and a launch of each kernel family hold.  No HIP include: a host compiler reads this file on its own.  The
// kernel headers include it instead of defining the values.
#pragma once
#include <stdint.h>

namespace tsamd {

// ---- launch-per-pass kernels (tsamd_device.h, tsamd_kernels.h) --------------------------------------------------------
constexpr int kMaxGrid = 2048;    // upper bound on pass-kernel workgroups
// (peer-to-peer exchange buffer, struct Xchg in tsamd_device.h: pass kernels then run with at most 512 / world
// workgroups, never more than kXchgBlocks)
constexpr int kMaxRanks = 16;
constexpr int kXchgBlocks = 256;

// ---- wide-K fallback (tsamd_wide_kernels.h) ---------------------------------------------------------------------------
constexpr int kWideBlock = 512;
constexpr int kWideItems = 8;   // max individuals per thread (the launch geometry guarantees it)

// ---- the register-resident kernels (tsamd_resident_kernels.h): geometry per K --------------------------------------------
constexpr int kResidentMaxK = 32;
constexpr int kResidentBlock = 256;
#ifdef TSAMD_RES_VEC  // (experiments, UNIT=all tools/variant.sh: 2 = pairs of individuals per item at K <= 8, round 2's geometry)
constexpr int resident_vec(int k) { return k <= 8 ? TSAMD_RES_VEC : 1; }
#else
constexpr int resident_vec(int) { return 1; }
#endif
// (K = 22: 4, not floor(112 / 22) = 5 -- with 110 doubles of weights every ts_schedule<22> instantiation spilled 36 ... 76 bytes
// to scratch: profiles/r06_kernel_resources.txt, round 6)
constexpr int resident_items(int k) { return k <= 8 ? 16 / resident_vec(k) : k <= 16 ? 128 / k : k == 22 ? 4 : k <= 24 ? 112 / k : 3; }
// individuals a workgroup can hold
constexpr int resident_capacity(int k) { return resident_items(k) * resident_vec(k) * kResidentBlock; }
// ... and what a thread of a SHARDED launch holds (ts_schedule<K, ., WR > 0>, ts_holblock<K, WR > 0>: the ranks' launches share one
// geometry rule, resident_geometry in csrc/tsamd_plan.h): K = 16 one item less -- its 128 doubles of weights fill the AGPR half of the
// register file, and the sharded exchange's few extra registers went to scratch (20 ... 52 bytes); K = 14 (9 x 14 = 126 doubles) likewise
constexpr int sharded_items(int k) { return k == 16 ? 7 : k == 14 ? 8 : resident_items(k); }
constexpr int sched_items(int k, int wr) { return wr > 0 ? sharded_items(k) : resident_items(k); }

// ---- their in-launch exchange (described in tsamd_resident_kernels.h) ---------------------------------------------------
constexpr int kResGroups = 8;    // (Xchg::res_sums is laid out for these two)
constexpr int kResMembers = 32;  // workgroups per group (grid <= 256)
#ifndef TSAMD_ONE_LEVEL  // (experiments: 0 = always two levels.  Measured at K = 8: up to 16 rows 34.5 us per update against
#define TSAMD_ONE_LEVEL 32  // 43.8 with two levels; 17 ... 32 rows -- since the row sums run on the vector ALU -- 33.8 against
#endif                      // 37.1 at N = 16 000; 64 loses at every size: profiles/r03_experiments.md)
constexpr int kResOneLevelGrid = TSAMD_ONE_LEVEL;  // up to this many workgroups (one GPU) the exchange has ONE level: everybody reads every row

// ---- ts_hybrid (tsamd_hybrid_kernels.h) -------------------------------------------------------------------------------
// items whose weights live in LDS: what 160 KB hold beside the K x 2 arrays, at most 16 (their codes share one register)
constexpr int hy_lds_items(int k) {
  const int n = (160 * 1024 - 1024 - 200 * k) / (k * 8 * 256);
  return n > 16 ? 16 : n;
}
// items in registers: ts_schedule's, one fewer above K = 20 (the streamed items' pipeline needs the registers); round 6, from the
// build's resource table (profiles/r06_kernel_resources.txt): K = 9 13 instead of 14 and K = 29 ... 32 one instead of two -- the
// streamed instantiations of those K used 20 ... 236 bytes of scratch
// (K = 22: floor(112 / 22) - 1 = 4, as before ts_schedule<22> went from 5 items to 4 in round 6)
constexpr int hy_reg_items(int k) { return k == 9 ? 13 : k <= 20 ? resident_items(k) : k <= 24 ? 112 / k - 1 : k <= 28 ? 2 : 1; }
// individuals a workgroup holds without streaming any weights
constexpr int hybrid_resident_capacity(int k) { return (hy_reg_items(k) + hy_lds_items(k)) * kResidentBlock; }
// streamed items per thread at most (a bound on the loop, not a register budget: 4M individuals per GPU at least)
constexpr int kHybridMaxStreamed = 64;

// ---- ts_holblock (tsamd_holblock_kernels.h) ---------------------------------------------------------------------------
// locations whose accumulators AND exp(Elogbeta) a thread holds at once (4 K BA <= 64 doubles: with the pairs re-read from
// LDS per item and four locations' accumulators -- round 4's first form -- a sub-batch sweep took twice the instructions) ...
constexpr int hol_sub(int k) { return k <= 4 ? 4 : k <= 8 ? 2 : 1; }
// ... and locations per exchange: a multiple of that, at most 16, rows of at most 256 values (BX K <= 128)
constexpr int hol_batch(int k) {
  const int ba = hol_sub(k);
  int n = 128 / (k * ba);
  if (n > 16 / ba) n = 16 / ba;
  if (n < 1) n = 1;
  return n * ba;
}
constexpr uint32_t kHolChunk = 1u << 14;

}  // namespace tsamd
