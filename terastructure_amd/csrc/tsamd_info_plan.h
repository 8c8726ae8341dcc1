// tsamd_theta_info / tsamd_theta_se: the per-entry terms, the packed index, the block / chunk / segment geometry and the whole of
// tsamd_theta_se, as plain C++ that the host, the kernels (tsamd_info_kernels.h) and a stand-alone check without any ROCm header
// (tests/theta_info_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "tsamd_kin_plan.h"     // kin_row_first: the packed order; kin_segments: a chunk's segments in k-steps
#include "tsamd_loglik_plan.h"  // loglik_code_y / loglik_code_ok: the 2-bit codes
#include "tsamd_sweep_plan.h"   // sweep_fill_segments

#if defined(__HIPCC__)
#define TSAMD_INFO_HD __host__ __device__
#else
#define TSAMD_INFO_HD
#endif

namespace tsamd {

constexpr uint32_t kInfoMaxK = 128;                   // TSAMD_MAX_K
constexpr uint32_t kInfoTile = 64;                    // T: individuals x packed columns of the tile a workgroup owns
constexpr uint32_t kInfoBlock = 256;                  // threads per workgroup (4 waves) of every kernel of the family
constexpr uint32_t kInfoStep = 4;                     // locations per k-step of v_mfma_f64_16x16x4_f64
constexpr uint32_t kInfoStageSteps = 4;               // k-steps (16 locations) a workgroup stages in LDS at a time
constexpr uint32_t kInfoCoefIndivs = 256;             // individuals (one per thread) of a ts_info_coef workgroup ...
constexpr uint32_t kInfoCoefBatch = 16;               // ... and its locations: their Ebeta and their columns' bytes in LDS
constexpr uint32_t kInfoMaxSegments = 64;             // location segments per chunk, at most
constexpr uint32_t kInfoMaxChunk = 4096;              // locations per chunk, at most
constexpr uint32_t kInfoMaxBlockIndivs = 8192;        // individuals per block, at most
constexpr uint64_t kInfoScratchBound = 256ull << 20;  // bytes of c_obs / c_exp, of BB, of the partial tiles, of a block's accumulators, at most (each)
constexpr uint64_t kInfoTileBytes = 2ull * kInfoTile * kInfoTile * sizeof(double);  // a partial: the tile of both products

// The two curvature terms of one stored entry: c_obs = y / q^2 + (2 - y) / (1 - q)^2 (observed information) and
// c_exp = 2 / (q (1 - q)) (expected information).  Both 0 where the code is 01 (missing, held out, padding) and where q is not
// inside (0, 1) (by rounding) or so close to 0 that a term overflows: never an inf or a NaN.  A quotient whose numerator is 0
// (y = 0 over q^2, 2 - y = 0 over (1 - q)^2) is not formed, so a q^2 that underflows to 0 costs an entry with y = 0 nothing.
TSAMD_INFO_HD inline void info_terms(double q, uint32_t code, double *c_obs, double *c_exp) {
  const double p = 1.0 - q;
  const double y = (double)loglik_code_y(code);
  const double t0 = y > 0.0 ? y / (q * q) : 0.0, t1 = y < 2.0 ? (2.0 - y) / (p * p) : 0.0;
  const double co = t0 + t1, ce = 2.0 / (q * p);
  const bool ok = loglik_code_ok(code) && q > 0.0 && p > 0.0 && co <= 1.7976931348623157e308 && ce <= 1.7976931348623157e308;
  *c_obs = ok ? co : 0.0;
  *c_exp = ok ? ce : 0.0;
}

// Packed symmetric K x K: entry (a <= b) at a K - a (a - 1) / 2 + (b - a), row by row -- kin_row_first's order
TSAMD_INFO_HD constexpr uint32_t info_packed(uint32_t k) { return k * (k + 1u) / 2u; }
TSAMD_INFO_HD constexpr uint32_t info_index(uint32_t a, uint32_t b, uint32_t k) { return kin_row_first(a, k) + (b - a); }
TSAMD_INFO_HD constexpr uint32_t info_index_sym(uint32_t a, uint32_t b, uint32_t k) { return a <= b ? info_index(a, b, k) : info_index(b, a, k); }
struct InfoAB {
  uint32_t a, b;
};
TSAMD_INFO_HD inline InfoAB info_unindex(uint32_t p, uint32_t k) {
  const KinPair r = kin_pair(p, k);
  InfoAB ab;
  ab.a = r.ti, ab.b = r.tj;
  return ab;
}

TSAMD_INFO_HD constexpr uint32_t info_round_tile(uint32_t x) { return (x + kInfoTile - 1u) / kInfoTile * kInfoTile; }
TSAMD_INFO_HD constexpr uint32_t info_round_step(uint32_t x) { return (x + kInfoStep - 1u) / kInfoStep * kInfoStep; }
// P padded to whole column tiles; the padded columns of BB are zero
TSAMD_INFO_HD constexpr uint32_t info_ppad(uint32_t k) { return info_round_tile(info_packed(k)); }

// One call = blocks of at most `block` listed individuals; a block = chunks of at most `chunk` listed locations.  A chunk:
// ts_info_coef fills c_obs and c_exp [chunk4][bpad] (chunk4 = the chunk rounded up to whole k-steps, bpad = the block rounded up
// to whole tiles; tail rows and padding columns zero), ts_info_outer fills BB [chunk4][ppad]; then, `tiles_per_launch` tiles at a
// time, ts_info_gemm on a grid of (tiles, nseg) writes the segments' tiles and ts_info_finish adds them onto the block's
// accumulators [itiles][ptiles][2][T * T].  After the last chunk ts_info_rows writes the block's rows [block][P] twice.
struct InfoGeom {
  uint32_t k, p, ppad, ptiles;
  uint32_t block, bpad, itiles;  // individuals per block (a multiple of 4; of 64 without the test hook), padded, its tiles
  uint32_t chunk;                // locations per chunk
  uint32_t tiles;                // tiles of a full block: itiles * ptiles
  uint32_t nseg_max;             // segments of a full chunk: 1 when the tiles alone fill the device
  uint32_t tiles_per_launch;     // nseg_max * tiles_per_launch partial tiles fit the bound
};

// m: listed individuals; cus: compute units to fill; test_chunk / test_block: TSAMD_TEST_INFO_CHUNK / TSAMD_TEST_INFO_BLOCK (0: none)
TSAMD_INFO_HD inline InfoGeom info_geometry(uint32_t m, uint32_t k, uint32_t n_locs, uint32_t cus, uint32_t test_chunk, uint32_t test_block) {
  InfoGeom g;
  g.k = k;
  g.p = info_packed(k);
  g.ppad = info_ppad(k);
  g.ptiles = g.ppad / kInfoTile;
  // the block: its accumulators (two products) fit the bound -- 1984 individuals at K = 128
  uint64_t block = kInfoScratchBound / (2ull * sizeof(double) * g.ppad) / kInfoTile * kInfoTile;
  if (block > kInfoMaxBlockIndivs) block = kInfoMaxBlockIndivs;
  if (block > info_round_tile(m)) block = info_round_tile(m);
  if (test_block > 0u && block > info_round_step(test_block)) block = info_round_step(test_block);
  g.block = (uint32_t)block;
  g.bpad = info_round_tile(g.block);
  g.itiles = g.bpad / kInfoTile;
  // the chunk: c_obs and c_exp of the block, and BB, fit the bound (each) -- at least 2048 and 4064 locations
  uint64_t chunk = kInfoScratchBound / (2ull * sizeof(double) * g.bpad) / kInfoStep * kInfoStep;
  const uint64_t bb_fit = kInfoScratchBound / (sizeof(double) * g.ppad) / kInfoStep * kInfoStep;
  if (chunk > bb_fit) chunk = bb_fit;
  if (chunk > kInfoMaxChunk) chunk = kInfoMaxChunk;
  if (test_chunk > 0u && chunk > test_chunk) chunk = test_chunk;
  if (chunk > n_locs) chunk = n_locs;
  if (chunk < 1u) chunk = 1u;
  g.chunk = (uint32_t)chunk;
  g.tiles = g.itiles * g.ptiles;
  g.nseg_max = (uint32_t)sweep_fill_segments(g.tiles, cus, kInfoMaxSegments);
  const uint64_t fit = kInfoScratchBound / kInfoTileBytes / g.nseg_max;  // (>= 64)
  g.tiles_per_launch = g.tiles < fit ? g.tiles : (uint32_t)fit;
  return g;
}

// segments of a chunk of len locations, in k-steps (kin_segments: at least kKinMinSegSteps k-steps each, none empty).  They do
// not depend on the block, so a row's summation order is the same in every block of a call.
TSAMD_INFO_HD inline KinSegs info_segments(const InfoGeom &g, uint32_t len) {
  static_assert(kKinStep == kInfoStep, "the k-step of the same instruction");
  KinGeom kg{};
  kg.nseg_max = g.nseg_max;
  return kin_segments(kg, len);
}

// bytes of c_obs + c_exp, of BB, of the partial tiles, of a block's accumulators and of its two sets of rows
TSAMD_INFO_HD inline uint64_t info_coef_bytes(const InfoGeom &g) { return 2ull * info_round_step(g.chunk) * g.bpad * sizeof(double); }
TSAMD_INFO_HD inline uint64_t info_bb_bytes(const InfoGeom &g) { return (uint64_t)info_round_step(g.chunk) * g.ppad * sizeof(double); }
TSAMD_INFO_HD inline uint64_t info_part_bytes(const InfoGeom &g) { return (uint64_t)g.nseg_max * g.tiles_per_launch * kInfoTileBytes; }
TSAMD_INFO_HD inline uint64_t info_acc_bytes(const InfoGeom &g) { return (uint64_t)g.tiles * kInfoTileBytes; }
TSAMD_INFO_HD inline uint64_t info_rows_bytes(const InfoGeom &g) { return 2ull * g.block * g.p * sizeof(double); }

// ---- tsamd_theta_se: pure host function (no context, no device) ------------------------------------------------------------

constexpr double kInfoPivotTol = 1e-12;  // a pivot must exceed this times its own original diagonal entry

// One individual: info [P] packed -> se [k], cov [P] packed (may be NULL); returns the status (0: identified, 1: not, se and cov
// NaN).  M = Z^T H Z with Z the basis that drops the last component (M_ab = H_ab - H_aK - H_Kb + H_KK, a, b < K - 1), Cholesky
// of M without pivoting, cov = Z M^-1 Z^T, se_k = sqrt(cov_kk).  work: at least 2 (k - 1)^2 doubles.
inline uint8_t theta_se_row(const double *info, uint32_t k, double *se, double *cov, double *work) {
  const uint32_t P = info_packed(k);
  if (k == 1u) {
    se[0] = 0.0;
    if (cov) cov[0] = 0.0;
    return 0u;
  }
  const uint32_t r = k - 1u;
  double *L = work, *W = work + (size_t)r * r;  // L: the Cholesky factor (lower); W: its inverse (lower), then M^-1 (full)
  const double hkk = info[info_index(r, r, k)];
  for (uint32_t a = 0; a < r; ++a)
    for (uint32_t b = 0; b <= a; ++b) L[(size_t)a * r + b] = info[info_index(b, a, k)] - info[info_index(a, r, k)] - info[info_index(b, r, k)] + hkk;
  bool ok = true;
  for (uint32_t j = 0; j < r && ok; ++j) {
    const double orig = L[(size_t)j * r + j];
    double d = orig;
    for (uint32_t t = 0; t < j; ++t) d -= L[(size_t)j * r + t] * L[(size_t)j * r + t];
    if (!(d > kInfoPivotTol * orig) || !(d > 0.0) || !isfinite(d)) {  // (also an orig of 0 or a NaN)
      ok = false;
      break;
    }
    const double ljj = sqrt(d);
    L[(size_t)j * r + j] = ljj;
    for (uint32_t i = j + 1u; i < r; ++i) {
      double s = L[(size_t)i * r + j];
      for (uint32_t t = 0; t < j; ++t) s -= L[(size_t)i * r + t] * L[(size_t)j * r + t];
      L[(size_t)i * r + j] = s / ljj;
    }
  }
  if (!ok) {
    for (uint32_t a = 0; a < k; ++a) se[a] = NAN;
    if (cov)
      for (uint32_t p = 0; p < P; ++p) cov[p] = NAN;
    return 1u;
  }
  // W = L^-1 (lower), column by column
  for (uint32_t c = 0; c < r; ++c)
    for (uint32_t i = 0; i < r; ++i) {
      if (i < c) {
        W[(size_t)i * r + c] = 0.0;
        continue;
      }
      double s = i == c ? 1.0 : 0.0;
      for (uint32_t t = c; t < i; ++t) s -= L[(size_t)i * r + t] * W[(size_t)t * r + c];
      W[(size_t)i * r + c] = s / L[(size_t)i * r + i];
    }
  // M^-1 = W^T W into L (full, symmetric)
  for (uint32_t a = 0; a < r; ++a)
    for (uint32_t b = a; b < r; ++b) {
      double s = 0.0;
      for (uint32_t t = b; t < r; ++t) s += W[(size_t)t * r + a] * W[(size_t)t * r + b];
      L[(size_t)a * r + b] = s;
      L[(size_t)b * r + a] = s;
    }
  // cov = Z M^-1 Z^T: the last row / column is minus the sum of the others
  double total = 0.0;
  for (uint32_t a = 0; a < r; ++a) {
    double rs = 0.0;
    for (uint32_t b = 0; b < r; ++b) rs += L[(size_t)a * r + b];
    total += rs;
    se[a] = sqrt(L[(size_t)a * r + a]);
    if (cov) {
      for (uint32_t b = a; b < r; ++b) cov[info_index(a, b, k)] = L[(size_t)a * r + b];
      cov[info_index(a, r, k)] = -rs;
    }
  }
  se[r] = sqrt(total);
  if (cov) cov[info_index(r, r, k)] = total;
  return 0u;
}

// every individual; cov and status may be NULL
inline void theta_se(const double *info, uint32_t m, uint32_t k, double *se, double *cov, uint8_t *status) {
  const uint32_t P = info_packed(k);
  std::vector<double> work(2u * (size_t)k * k + 2u);
  for (uint32_t i = 0; i < m; ++i) {
    const uint8_t st = theta_se_row(info + (size_t)i * P, k, se + (size_t)i * k, cov ? cov + (size_t)i * P : nullptr, work.data());
    if (status) status[i] = st;
  }
}

#if defined(__HIPCC__)
// what one chunk's launches need (tsamd_info.hip)
struct InfoArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *gam;     // [K][npad]
  const double *lam;     // [l][K][2]
  const uint32_t *ids;   // [bpad] LOCAL individuals of the block's rows, 0xffffffff: a padding row; NULL: individuals ind0 + row
  const uint32_t *locs;  // the chunk's locations
  uint32_t npad, n_local, K, P, ppad, ptiles;
  uint32_t ind0, blen, bpad;  // the block: blen listed individuals, padded to whole tiles
  uint32_t len, len4;         // the chunk: len listed locations, rounded up to k-steps
  double *cobs, *cexp;   // [len4][bpad]
  double *bb;            // [len4][ppad]
  double *part;          // [nseg][tiles of the launch][2][T * T]
  double *acc;           // [tiles of the block][2][T * T]
};
// c_obs, c_exp and BB of the chunk
void info_launch_coef(const InfoArgs &a, hipStream_t stream);
// tiles [tile0, tile0 + ntiles) of the block (tile t: individuals' tile t / ptiles, column tile t % ptiles): the segments' tiles,
// then their addition in ascending order onto acc
void info_launch_tiles(const InfoArgs &a, uint32_t tile0, uint32_t ntiles, const KinSegs &sg, hipStream_t stream);
// the block's rows from acc: obs and exp [blen][P]
void info_launch_rows(const InfoArgs &a, double *obs, double *exp, hipStream_t stream);
#endif

}  // namespace tsamd
