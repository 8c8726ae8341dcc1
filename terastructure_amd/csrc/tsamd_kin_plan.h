// tsamd_kinship: the per-entry terms and the tile-pair / segment / chunk geometry, as plain C++ that the host, the kernels
// (tsamd_kin_kernels.h) and a stand-alone check without any ROCm header (tests/kinship_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tsamd_loglik_plan.h"  // loglik_code_y / loglik_code_ok: the 2-bit codes

#if defined(__HIPCC__)
#define TSAMD_KIN_HD __host__ __device__
#else
#define TSAMD_KIN_HD
#endif

namespace tsamd {

constexpr uint32_t kKinMaxM = 32768;                  // TSAMD_KIN_MAX_M
constexpr uint32_t kKinTile = 64;                     // T: side of the tile of listed individuals a workgroup owns (see tsamd_kin_kernels.h)
constexpr uint32_t kKinBlock = 256;                   // threads per workgroup (4 waves) of every kernel of the family
constexpr uint32_t kKinStep = 4;                      // locations per k-step of v_mfma_f64_16x16x4_f64
constexpr uint32_t kKinStageSteps = 4;                // k-steps (16 locations) a workgroup stages in LDS at a time
constexpr uint32_t kKinMinSegSteps = 4;               // a segment covers at least that many k-steps (or the whole chunk)
constexpr uint32_t kKinResidBatch = 32;               // locations whose Ebeta a ts_kin_resid workgroup keeps in LDS
constexpr uint32_t kKinMaxSegments = 64;              // location segments per chunk, at most
constexpr uint32_t kKinMaxChunk = 1u << 16;           // locations per chunk, at most (a multiple of kKinStep)
constexpr uint64_t kKinScratchBound = 256ull << 20;   // bytes of the r / s scratch, and of the partial tiles, at most (each)
constexpr uint64_t kKinTileBytes = 2ull * kKinTile * kKinTile * sizeof(double);  // a partial: the tile of both products

// r = y - 2q and s = sqrt(q (1 - q)) of one stored entry; both 0 where the code is 01 (missing, held out, padding).
// (q (1 - q) <= 0 -- q outside (0, 1) by rounding -- gives s = 0, never a NaN.)
TSAMD_KIN_HD inline void kin_terms(double q, uint32_t code, double *r, double *s) {
  const bool ok = loglik_code_ok(code);
  const double v = q * (1.0 - q);
  *r = ok ? (double)loglik_code_y(code) - (q + q) : 0.0;
  *s = ok && v > 0.0 ? sqrt(v) : 0.0;
}

// m listed individuals padded to whole tiles; the padding rows of r and s are zero
TSAMD_KIN_HD constexpr uint32_t kin_mpad(uint32_t m) { return (m + kKinTile - 1u) / kKinTile * kKinTile; }
TSAMD_KIN_HD constexpr uint32_t kin_ntiles(uint32_t m) { return (m + kKinTile - 1u) / kKinTile; }
// tile pairs (ti <= tj), row by row: (0,0) (0,1) .. (0,nt-1) (1,1) ..
TSAMD_KIN_HD constexpr uint32_t kin_npairs(uint32_t nt) { return nt * (nt + 1u) / 2u; }
TSAMD_KIN_HD constexpr uint32_t kin_row_first(uint32_t ti, uint32_t nt) { return ti * nt - ti * (ti - 1u) / 2u; }  // (ti = 0: 0 - 0)
struct KinPair {
  uint32_t ti, tj;
};
TSAMD_KIN_HD inline KinPair kin_pair(uint32_t p, uint32_t nt) {
  const double b = 2.0 * nt + 1.0;
  double d = b * b - 8.0 * p;
  int64_t ti = (int64_t)((b - sqrt(d < 0.0 ? 0.0 : d)) * 0.5);
  if (ti < 0) ti = 0;
  if (ti >= (int64_t)nt) ti = (int64_t)nt - 1;
  while (ti > 0 && kin_row_first((uint32_t)ti, nt) > p) --ti;              // (the square root is an estimate: settle it exactly)
  while (ti + 1 < (int64_t)nt && kin_row_first((uint32_t)ti + 1u, nt) <= p) ++ti;
  KinPair r;
  r.ti = (uint32_t)ti;
  r.tj = r.ti + (p - kin_row_first(r.ti, nt));
  return r;
}

// One call = chunks of at most `chunk` listed locations.  A chunk: ts_kin_resid fills r and s [chunk4][mpad] (chunk4 = the chunk
// rounded up to whole k-steps, the tail rows zero); then, `pairs_per_launch` tile pairs at a time, ts_kin_syrk on a grid of
// (pairs, nseg) writes the segments' tiles and ts_kin_finish adds them onto the accumulators.
struct KinGeom {
  uint32_t mpad, ntiles, npairs;
  uint32_t nseg_max;          // segments of a full chunk: 1 when the tile pairs alone fill the device
  uint32_t pairs_per_launch;  // nseg_max * pairs_per_launch partial tiles fit the bound
  uint32_t chunk;             // locations per chunk
};

TSAMD_KIN_HD constexpr uint32_t kin_round_step(uint32_t len) { return (len + kKinStep - 1u) / kKinStep * kKinStep; }

// cus: compute units to fill; test_chunk / test_segments: TSAMD_TEST_KIN_CHUNK / TSAMD_TEST_KIN_SEGMENTS (0: none)
TSAMD_KIN_HD inline KinGeom kin_geometry(uint32_t m, uint32_t cus, uint32_t test_chunk, uint32_t test_segments) {
  KinGeom g;
  g.mpad = kin_mpad(m);
  g.ntiles = kin_ntiles(m);
  g.npairs = kin_npairs(g.ntiles);
  if (cus < 1u) cus = 1u;
  if (cus > 1024u) cus = 1024u;
  uint32_t nseg = g.npairs >= 2u * cus ? 1u : (2u * cus + g.npairs - 1u) / g.npairs;
  if (test_segments > 0u) nseg = test_segments;
  if (nseg > kKinMaxSegments) nseg = kKinMaxSegments;
  g.nseg_max = nseg;
  const uint64_t fit = kKinScratchBound / kKinTileBytes / nseg;  // (>= 64: kKinMaxSegments tiles are far below the bound)
  g.pairs_per_launch = g.npairs < fit ? g.npairs : (uint32_t)fit;
  uint64_t chunk = kKinScratchBound / (2ull * sizeof(double) * g.mpad) / kKinStep * kKinStep;  // (>= 512 at mpad = 32768)
  if (chunk > kKinMaxChunk) chunk = kKinMaxChunk;
  if (test_chunk > 0u && chunk > test_chunk) chunk = test_chunk;
  g.chunk = (uint32_t)chunk;
  return g;
}

// segments of a chunk of len locations, in k-steps: segment g covers steps [g seg_steps, min(steps, (g + 1) seg_steps))
struct KinSegs {
  uint32_t steps, nseg, seg_steps;
};
TSAMD_KIN_HD inline KinSegs kin_segments(const KinGeom &g, uint32_t len) {
  KinSegs s;
  s.steps = kin_round_step(len) / kKinStep;
  uint32_t nseg = s.steps / kKinMinSegSteps;
  if (nseg > g.nseg_max) nseg = g.nseg_max;
  if (nseg < 1u) nseg = 1u;
  s.seg_steps = (s.steps + nseg - 1u) / nseg;
  s.nseg = s.seg_steps ? (s.steps + s.seg_steps - 1u) / s.seg_steps : 1u;
  return s;
}

// bytes of the r / s scratch, of the partial tiles and of the two accumulators of a geometry
TSAMD_KIN_HD inline uint64_t kin_rs_bytes(const KinGeom &g) { return 2ull * kin_round_step(g.chunk) * g.mpad * sizeof(double); }
TSAMD_KIN_HD inline uint64_t kin_part_bytes(const KinGeom &g) { return (uint64_t)g.nseg_max * g.pairs_per_launch * kKinTileBytes; }
TSAMD_KIN_HD inline uint64_t kin_acc_bytes(const KinGeom &g) { return 2ull * g.mpad * g.mpad * sizeof(double); }

#if defined(__HIPCC__)
// what one chunk's launches need (tsamd_kin.hip)
struct KinArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *gam;     // [K][npad]
  const double *lam;     // [l][K][2]
  const uint32_t *ids;   // [mpad] LOCAL individuals of the rows; 0xffffffff: a padding row
  const uint32_t *locs;  // the chunk's locations
  uint32_t npad, K, len, len4, mpad, ntiles;
  double *r, *s;         // [len4][mpad]
  double *part;          // [nseg][pairs_per_launch][2][T * T]
  double *num, *den;     // [mpad][mpad]: the call's accumulators (upper tile pairs)
};
// r and s of the chunk
void kin_launch_resid(const KinArgs &a, hipStream_t stream);
// pairs [pair0, pair0 + npairs): the segments' tiles, then their addition in ascending order onto num / den
void kin_launch_pairs(const KinArgs &a, uint32_t pair0, uint32_t npairs, const KinSegs &sg, hipStream_t stream);
// after the last chunk: x[b][a] = x[a][b] for a < b, both accumulators
void kin_launch_mirror(double *num, double *den, uint32_t mpad, hipStream_t stream);
// kin = num / (4 den), 0 where den == 0, written over num
void kin_launch_form(double *num, const double *den, uint32_t mpad, hipStream_t stream);
#endif

}  // namespace tsamd
