// What the column sweeps of the analysis calls (tsamd_train_loglik, tsamd_snp_scan, tsamd_fold_in) share of their host-only
// geometry, as plain C++ without any ROCm header: how many location segments fill the device when the tiles of individuals
// alone do not, and how a chunk of listed locations is cut into segments.  No kernel calls anything here.
// (tests/analysis_plan_check.cpp replays the geometries recorded before this header existed.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TSAMD_SW_HD __host__ __device__
#else
#define TSAMD_SW_HD
#endif

namespace tsamd {

// segments of a full chunk on a grid of ntiles x segments workgroups: 1 when the tiles alone fill the cus compute units
// (taken inside [1, 1024]), otherwise two workgroups per unit; at most max_segments
TSAMD_SW_HD inline uint64_t sweep_fill_segments(uint32_t ntiles, uint32_t cus, uint32_t max_segments) {
  if (cus < 1u) cus = 1u;
  if (cus > 1024u) cus = 1024u;
  const uint64_t nseg = ntiles >= cus ? 1u : (2ull * cus + ntiles - 1u) / ntiles;
  return nseg > max_segments ? max_segments : nseg;
}

// segments of a chunk of len locations, at most nseg_max: at least 8 locations each, so that a workgroup's theta load is
// shared, and none of them empty
struct SweepSegs {
  uint32_t nseg, seg_len;
};
TSAMD_SW_HD inline SweepSegs sweep_segments(uint32_t nseg_max, uint32_t len) {
  uint32_t nseg = (len + 7u) / 8u;
  if (nseg > nseg_max) nseg = nseg_max;
  if (nseg < 1u) nseg = 1u;
  SweepSegs s;
  s.seg_len = (len + nseg - 1u) / nseg;
  s.nseg = s.seg_len ? (len + s.seg_len - 1u) / s.seg_len : 1u;
  return s;
}

}  // namespace tsamd
