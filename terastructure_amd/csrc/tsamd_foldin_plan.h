// tsamd_fold_in: the per-entry contribution, the change of an update and the tile / segment geometry, as plain C++ that the
// host, the kernels (tsamd_foldin_kernels.h) and a stand-alone check without any ROCm header (tests/fold_in_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tsamd_sweep_plan.h"

#if defined(__HIPCC__)
#define TSAMD_FI_HD __host__ __device__
#else
#define TSAMD_FI_HD
#endif

namespace tsamd {

constexpr uint32_t kFoldinBlock = 256;                    // threads per workgroup
constexpr uint32_t kFoldinBatch = 32;                     // locations whose exp(Elogbeta) a workgroup keeps in LDS at a time, K <= 32 ...
constexpr uint32_t kFoldinWideBatch = 16;                 // ... and at a run-time K up to 128 (2 x 16 x 128 doubles = 32 KB)
constexpr uint32_t kFoldinSpecializedK = 32;              // ts_foldin_sweep<K> exists for K = 1 .. 32
constexpr uint32_t kFoldinMaxK = 128;                     // the largest k a context accepts
constexpr uint32_t kFoldinMaxSegments = 128;              // location segments, at most (few tiles: the projection shape)
constexpr uint32_t kFoldinMinSegLen = 64;                 // locations per segment, at least: a workgroup's load of w is shared
constexpr uint64_t kFoldinScratchBound = 256ull << 20;    // bytes of partials ([nseg][K][npad] doubles), at most -- see foldin_scratch_bound

// individuals per thread: w and acc of a thread, 2 IPT K doubles (at most 64: 128 VGPRs), stay in its registers for every
// location it visits.  IPT divides 16: a thread's individuals share one 32-bit word of a 2-bit column.  Above
// kFoldinSpecializedK (0 stands for the run-time-K kernel): one, w and acc in [K][npad] arrays.
TSAMD_FI_HD constexpr uint32_t foldin_ipt(uint32_t K) {
  return K == 0u || K > 16u ? 1u : K <= 2u ? 16u : K <= 4u ? 8u : K <= 8u ? 4u : 2u;
}

// one segment of partials is as large as gamma itself and cannot be cut: the bound is kFoldinScratchBound or that, whichever
// is larger (above 256 MB only past 33.5M weights per GPU, n x k)
TSAMD_FI_HD inline uint64_t foldin_scratch_bound(uint32_t npad, uint32_t K) {
  const uint64_t one = (uint64_t)npad * K * sizeof(double);
  return one > kFoldinScratchBound ? one : kFoldinScratchBound;
}

// PLINK 2-bit code -> weights of the two allele copies as code_weights has them (tsamd_device.h): y and 2 - y for
// 00 -> 0, 10 -> 1, 11 -> 2; (0, 0) for 01 (missing, held out, padding), which therefore contributes nothing
TSAMD_FI_HD inline void foldin_code_weights(uint32_t c, double &mom, double &dad) {
  const uint32_t hi = c >> 1, lo = c & 1u, miss = lo & (hi ^ 1u), y = hi * (1u + lo);
  mom = (double)y;
  dad = (double)(2u - y - 2u * miss);
}

// 1 / x for the positive normal sums S0, S1: on the device the third-order step of fast_rcp (tsamd_device.h: error below
// 2^-73 plus the final rounding, four instructions where an IEEE division takes a dozen), on the host a division
TSAMD_FI_HD inline double foldin_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double r = __builtin_amdgcn_rcp(x);
  const double e = fma(-x, r, 1.0);
  return fma(r, fma(e, e, e), r);
#else
  return 1.0 / x;
#endif
}

// the two coefficients of one (individual, location) entry: acc_k += c0 eb[k][0] + c1 eb[k][1]
TSAMD_FI_HD inline void foldin_coeffs(double s0, double s1, uint32_t code, double &c0, double &c1) {
  double mom, dad;
  foldin_code_weights(code, mom, dad);
  c0 = mom * foldin_rcp(s0);
  c1 = dad * foldin_rcp(s1);
}

// one entry with a run-time K, as the kernels compute it (the sums in ascending k, multiply-adds): w [K], eb [K][2]
TSAMD_FI_HD inline void foldin_entry(const double *w, const double *eb, uint32_t K, uint32_t code, double *acc) {
  double s0 = 0.0, s1 = 0.0;
  for (uint32_t k = 0; k < K; ++k) {
    s0 = fma(w[k], eb[2u * k], s0);
    s1 = fma(w[k], eb[2u * k + 1u], s1);
  }
  double c0, c1;
  foldin_coeffs(s0, s1, code, c0, c1);
  for (uint32_t k = 0; k < K; ++k) acc[k] = fma(c0, eb[2u * k], fma(c1, eb[2u * k + 1u], acc[k]));
}

// the update of one population and the change of an update: mean_k |gamma' - gamma| / mean_k gamma' (the two 1 / K cancel)
TSAMD_FI_HD inline double foldin_gamma(double alpha, double w, double acc) { return fma(w, acc, alpha); }
TSAMD_FI_HD inline double foldin_change(double sum_abs_diff, double sum_new) { return sum_abs_diff / sum_new; }

// One update = one sweep on a grid of ntiles x nseg workgroups: workgroup (tile, seg) takes the tile's tile_n individuals
// through the listed positions [seg * seg_len, min(n_locs, (seg + 1) * seg_len)) and writes one partial per (seg, k,
// individual); then one step per individual, which adds the segments in ascending order.
struct FoldinGeom {
  uint32_t ipt, tile_n, ntiles, batch;
  uint32_t nseg, seg_len;
};

// npad: the shard's padded width (a multiple of 512); cus: compute units to fill; test_segments: TSAMD_TEST_FOLDIN_SEGMENTS
// (0: none; otherwise at most that many segments, whatever cus says)
TSAMD_FI_HD inline FoldinGeom foldin_geometry(uint32_t npad, uint32_t K, uint32_t n_locs, uint32_t cus, uint32_t test_segments) {
  FoldinGeom g;
  g.ipt = foldin_ipt(K);
  g.tile_n = kFoldinBlock * g.ipt;
  g.ntiles = (npad + g.tile_n - 1u) / g.tile_n;
  g.batch = K > kFoldinSpecializedK ? kFoldinWideBatch : kFoldinBatch;
  uint64_t nseg = sweep_fill_segments(g.ntiles, cus, kFoldinMaxSegments);
  if (test_segments > 0u) nseg = test_segments < kFoldinMaxSegments ? test_segments : kFoldinMaxSegments;
  // the partials [nseg][K][npad] stay under the bound
  const uint64_t one = (uint64_t)npad * K * sizeof(double);
  const uint64_t fit = foldin_scratch_bound(npad, K) / one;
  if (nseg > fit) nseg = fit;
  // segments of whole batches, at least kFoldinMinSegLen locations each (test_segments: any length) and none of them empty
  const uint32_t min_len = test_segments > 0u ? 1u : kFoldinMinSegLen;
  const uint64_t most = ((uint64_t)n_locs + min_len - 1u) / min_len;
  if (nseg > most) nseg = most;
  if (nseg < 1u) nseg = 1u;
  uint64_t len = ((uint64_t)n_locs + nseg - 1u) / nseg;
  if (test_segments == 0u) len = (len + g.batch - 1u) / g.batch * g.batch;
  if (len < 1u) len = 1u;
  g.seg_len = (uint32_t)len;
  g.nseg = (uint32_t)(((uint64_t)n_locs + len - 1u) / len);
  if (g.nseg < 1u) g.nseg = 1u;
  return g;
}

TSAMD_FI_HD inline uint64_t foldin_scratch_bytes(const FoldinGeom &g, uint32_t npad, uint32_t K) {
  return (uint64_t)g.nseg * K * npad * sizeof(double);
}

#if defined(__HIPCC__)
// what one update's launches need (tsamd_foldin.hip)
struct FoldinArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *eb;      // [l][K][2]
  const uint32_t *locs;  // the listed locations; NULL: position j is location j
  double *gam;           // [K][npad]
  double *w;             // [K][npad]  exp(Elogtheta) up to a factor per individual, as DevParams::w
  double *part;          // [nseg][K][npad]
  uint32_t *iters;       // [npad] updates applied
  double *change;        // [npad] change of the last update
  uint32_t *frozen;      // [npad] 1: converged (or padding: never updated)
  uint32_t *active;      // [1 + ntiles]: individuals still active, then per tile whether any is
  uint32_t npad, n_local, K, n_locs, nseg, seg_len, ntiles, tile_n;
  double alpha, tol;
};
// before the first update: iters = 0, change = 0, frozen = (n >= n_local), active = {n_local, tiles with a real individual}
void foldin_launch_init(const FoldinArgs &a, hipStream_t stream);
// one update: the sweep on a grid of (ntiles, nseg), then the step, which leaves the new count and tile flags in a.active
void foldin_launch_update(const FoldinArgs &a, hipStream_t stream);
#endif

}  // namespace tsamd
