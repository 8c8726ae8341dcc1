// tsamd_train_loglik: the per-entry term and the tile / segment / chunk geometry, as plain C++ that the host, the kernels
// (tsamd_loglik_kernels.h) and a stand-alone check without any ROCm header (tests/train_loglik_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tsamd_sweep_plan.h"

#if defined(__HIPCC__)
#define TSAMD_LL_HD __host__ __device__
#else
#define TSAMD_LL_HD
#endif

namespace tsamd {

constexpr uint32_t kLoglikBlock = 256;              // threads per workgroup
constexpr uint32_t kLoglikBatch = 32;               // locations whose Ebeta a workgroup keeps in LDS at a time
constexpr uint32_t kLoglikMaxSegments = 64;         // location segments per chunk (small shards)
constexpr uint32_t kLoglikMaxChunk = 1u << 16;      // locations per chunk, at most
constexpr uint64_t kLoglikScratchBound = 256ull << 20;  // bytes of partial-sum buffers, at most (shards up to 11M individuals)
constexpr uint32_t kLoglikPartBytes = 12;           // a partial: a double sum and a 32-bit count

// individuals per thread: IPT * K doubles of normalised theta (at most 64, 128 VGPRs) stay in the thread's registers for all
// the locations it visits.  0 stands for the run-time-K path (K above TSAMD_SPECIALIZED_K): theta comes from a scratch array.
TSAMD_LL_HD constexpr uint32_t loglik_ipt(uint32_t K) { return K == 0u || K > 32u ? 1u : K <= 4u ? 16u : K <= 8u ? 8u : K <= 16u ? 4u : 2u; }

// C(2,y) q^y (1-q)^(2-y) for y = 0, 1, 2 without pow: y picks the two factors
TSAMD_LL_HD inline double loglik_product(double q, uint32_t y) {
  const double r = 1.0 - q;
  const double a = y == 2u ? q : r;
  const double b = y == 0u ? r : q;
  const double p = a * b;
  return y == 1u ? p + p : p;
}

// the term of snp_likelihood (src/snpsamplinge.hh:336-360): one log per entry
TSAMD_LL_HD inline double loglik_term(double q, uint32_t y) {
  const double p = loglik_product(q, y);
  return log(p < 1e-30 ? 1e-30 : p);
}

// PLINK 2-bit code -> genotype as code_weights does (tsamd_device.h): 00 -> 0, 10 -> 1, 11 -> 2; 01 has no term
TSAMD_LL_HD inline uint32_t loglik_code_y(uint32_t c) { return (c >> 1) * (1u + (c & 1u)); }
TSAMD_LL_HD inline bool loglik_code_ok(uint32_t c) { return ((c & 1u) & ((c >> 1) ^ 1u)) == 0u; }

// One call = chunks of at most `chunk` listed locations; a chunk = a grid of ntiles x nseg workgroups: workgroup
// (tile, seg) takes the tile's tile_n individuals through the chunk's locations [seg * seg_len, (seg + 1) * seg_len).
struct LoglikGeom {
  uint32_t ipt, tile_n, ntiles;
  uint32_t nseg_max;  // segments of a full chunk: 1 when the tiles alone fill the device
  uint32_t chunk;     // locations per chunk
};

// npad: the shard's padded width (a multiple of 512); cus: compute units to fill; test_chunk: TSAMD_TEST_LOGLIK_CHUNK (0: none)
TSAMD_LL_HD inline LoglikGeom loglik_geometry(uint32_t npad, uint32_t K, uint32_t cus, uint32_t test_chunk) {
  LoglikGeom g;
  g.ipt = loglik_ipt(K);
  g.tile_n = kLoglikBlock * g.ipt;
  g.ntiles = (npad + g.tile_n - 1u) / g.tile_n;
  uint64_t nseg = sweep_fill_segments(g.ntiles, cus, kLoglikMaxSegments);
  // the per-individual partials ([nseg][npad]) take at most half of the bound ...
  const uint64_t row = (uint64_t)npad * kLoglikPartBytes;
  const uint64_t fit = (kLoglikScratchBound / 2u) / row;
  if (nseg > fit) nseg = fit < 1u ? 1u : fit;
  g.nseg_max = (uint32_t)nseg;
  // ... and the per-location ones ([chunk][ntiles]) what is left
  const uint64_t used = nseg * row;
  const uint64_t left = used < kLoglikScratchBound ? kLoglikScratchBound - used : 0u;
  uint64_t chunk = left / ((uint64_t)g.ntiles * kLoglikPartBytes);
  if (chunk > kLoglikMaxChunk) chunk = kLoglikMaxChunk;
  if (test_chunk > 0u && chunk > test_chunk) chunk = test_chunk;
  if (chunk < 1u) chunk = 1u;
  g.chunk = (uint32_t)chunk;
  return g;
}

// segments of a chunk of len locations (sweep_segments, tsamd_sweep_plan.h)
using LoglikSegs = SweepSegs;
TSAMD_LL_HD inline LoglikSegs loglik_segments(const LoglikGeom &g, uint32_t len) { return sweep_segments(g.nseg_max, len); }

// bytes of the partial-sum buffers of a geometry
TSAMD_LL_HD inline uint64_t loglik_scratch_bytes(const LoglikGeom &g, uint32_t npad) {
  return ((uint64_t)g.chunk * g.ntiles + (uint64_t)g.nseg_max * npad) * kLoglikPartBytes;
}

#if defined(__HIPCC__)
// what one chunk's launches need (tsamd_loglik.hip)
struct LoglikArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *gam;     // [K][npad]
  const double *thn;     // run-time-K path: normalised theta [K][npad]
  const double *lam;     // [l][K][2]
  const uint32_t *locs;  // the chunk's locations
  uint32_t npad, K, len, seg_len, ntiles;
  double *part_loc_sum;    // [len][ntiles]
  uint32_t *part_loc_cnt;  // [len][ntiles]
  double *part_ind_sum;    // [nseg][npad]
  uint32_t *part_ind_cnt;  // [nseg][npad]
};
// the sweep of one chunk on a grid of (ntiles, nseg), then the two index-order additions: per location over the tiles into
// out_sum / out_cnt [len], per individual over the segments onto acc_sum / acc_cnt [npad]
void loglik_launch_chunk(const LoglikArgs &a, uint32_t nseg, double *out_sum, uint32_t *out_cnt, double *acc_sum, uint32_t *acc_cnt,
                         hipStream_t stream);
// run-time-K path: thn = gam / sum_k gam, once per call
void loglik_launch_theta(const double *gam, uint32_t npad, uint32_t K, double *thn, hipStream_t stream);
#endif

}  // namespace tsamd
