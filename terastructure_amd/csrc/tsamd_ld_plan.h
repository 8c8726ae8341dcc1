// tsamd_ld / tsamd_ld_statistics / tsamd_ld_prune: the per-entry terms, the band layout, the tile-pair / chunk / block / segment
// geometry and the two pure host functions, as plain C++ that the host, the kernels (tsamd_ld_kernels.h) and a stand-alone check
// without any ROCm header (tests/ld_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tsamd_loglik_plan.h"  // loglik_code_y / loglik_code_ok: the 2-bit codes

#if defined(__HIPCC__)
#define TSAMD_LD_HD __host__ __device__
#else
#define TSAMD_LD_HD
#endif

namespace tsamd {

constexpr uint32_t kLdMaxWindow = 1024;              // TSAMD_LD_MAX_WINDOW
constexpr uint32_t kLdTile = 64;                     // T: side of the tile of listed locations a workgroup owns (see tsamd_ld_kernels.h)
constexpr uint32_t kLdBlock = 256;                   // threads per workgroup (4 waves) of every kernel of the family
constexpr uint32_t kLdStep = 4;                      // individuals per k-step of v_mfma_f64_16x16x4_f64
constexpr uint32_t kLdStageSteps = 4;                // k-steps (16 individuals) a workgroup stages in LDS at a time
constexpr uint32_t kLdMinSegSteps = 4;               // a segment covers at least that many k-steps (or the whole block)
constexpr uint32_t kLdResidIndivs = 256;             // individuals (one per thread) of a ts_ld_resid workgroup ...
constexpr uint32_t kLdResidBatch = 16;               // ... and its locations: their Ebeta in LDS, the tile transposed through LDS
constexpr uint32_t kLdMaxSegments = 64;              // segments of a block of individuals, at most
constexpr uint32_t kLdMaxChunkTiles = 64;            // location tiles a chunk owns, at most (4096 locations)
constexpr uint64_t kLdScratchBound = 256ull << 20;   // bytes of the Z / M scratch, of the partial tiles and of a chunk's accumulators, at most (each)
constexpr uint64_t kLdTileBytes = 2ull * kLdTile * kLdTile * sizeof(double);  // a partial: the tile of both products

// z = (y - 2q) / sqrt(2q (1 - q)) and m = 1 of one stored entry: E z = 0 and Var z = 1 under the model; both 0 where the code is
// 01 (missing, held out, padding) or where 2q (1 - q) <= 0 (q outside (0, 1) by rounding): never a NaN
TSAMD_LD_HD inline void ld_terms(double q, uint32_t code, double *z, double *m) {
  const double h = 2.0 * q * (1.0 - q);
  const bool ok = loglik_code_ok(code) && h > 0.0;
  *z = ok ? ((double)loglik_code_y(code) - (q + q)) / sqrt(h) : 0.0;
  *m = ok ? 1.0 : 0.0;
}

// The band: for list positions i = 0 .. n_locs-1 and a window W, row i has W + 1 columns d = 0 .. W; column d is the pair
// (i, i + d), column 0 the location with itself, every column with i + d >= n_locs is 0.
TSAMD_LD_HD constexpr uint64_t ld_band_index(uint32_t i, uint32_t d, uint32_t window) { return (uint64_t)i * (window + 1u) + d; }

TSAMD_LD_HD constexpr uint32_t ld_ntiles(uint32_t n) { return (n + kLdTile - 1u) / kLdTile; }
// tiles a pair of the band can lie apart: floor((i % T + W) / T) <= ceil(W / T)
TSAMD_LD_HD constexpr uint32_t ld_overlap_tiles(uint32_t window) { return (window + kLdTile - 1u) / kLdTile; }
TSAMD_LD_HD constexpr uint32_t ld_round_step(uint32_t len) { return (len + kLdStep - 1u) / kLdStep * kLdStep; }

// Band tile pairs of a chunk: the chunk owns tile rows ti = 0 .. rows-1 of the nt tiles that hold its locations and its
// overlap (rows <= nt <= rows + ov); row ti has the pairs (ti, tj), ti <= tj <= min(ti + ov, nt - 1); enumerated row by row.
TSAMD_LD_HD constexpr uint32_t ld_row_pairs(uint32_t ti, uint32_t nt, uint32_t ov) { return (nt - 1u - ti < ov ? nt - 1u - ti : ov) + 1u; }
// rows with all ov + 1 pairs come first: ti + ov <= nt - 1
TSAMD_LD_HD constexpr uint32_t ld_full_rows(uint32_t rows, uint32_t nt, uint32_t ov) { return nt > ov ? (rows < nt - ov ? rows : nt - ov) : 0u; }
TSAMD_LD_HD constexpr uint32_t ld_row_first(uint32_t ti, uint32_t rows, uint32_t nt, uint32_t ov) {
  const uint32_t f = ld_full_rows(rows, nt, ov);
  if (ti <= f) return ti * (ov + 1u);
  // rows f .. ti-1 have nt - f, nt - f - 1, .. pairs
  const uint32_t t = ti - f, first = nt - f;
  return f * (ov + 1u) + t * first - t * (t - 1u) / 2u;
}
TSAMD_LD_HD constexpr uint32_t ld_npairs(uint32_t rows, uint32_t nt, uint32_t ov) { return ld_row_first(rows, rows, nt, ov); }
struct LdPair {
  uint32_t ti, tj;
};
TSAMD_LD_HD inline LdPair ld_pair(uint32_t p, uint32_t rows, uint32_t nt, uint32_t ov) {
  const uint32_t f = ld_full_rows(rows, nt, ov);
  LdPair r;
  if (p < f * (ov + 1u)) {
    r.ti = p / (ov + 1u);
    r.tj = r.ti + p % (ov + 1u);
    return r;
  }
  uint32_t ti = f, rest = p - f * (ov + 1u);  // (at most ov short rows follow)
  while (ti + 1u < rows && rest >= nt - ti) rest -= nt - ti, ++ti;
  r.ti = ti;
  r.tj = ti + rest;
  return r;
}

// One call = chunks of chunk_tiles whole location tiles.  A chunk owns its rows of the band and also reads the next ov tiles
// (its overlap): Z and M hold [block, rounded to k-steps][lpad] with lpad = (chunk_tiles + ov) tiles, the location contiguous.
// Per chunk the shard's individuals go block after block: ts_ld_resid fills Z and M, then, `pairs_per_launch` tile pairs at a
// time, ts_ld_syrk on a grid of (pairs, nseg) writes the segments' tiles and ts_ld_finish adds them onto the chunk's
// accumulators [pairs][2][T * T]; after the last block ts_ld_band writes the chunk's rows.
struct LdGeom {
  uint32_t window, ov;
  uint32_t chunk_tiles, chunk;  // tiles / locations a chunk owns
  uint32_t lpad;                // columns of Z and M
  uint32_t block;               // individuals per block (a multiple of kLdStep)
  uint32_t max_pairs;           // tile pairs of a full chunk
  uint32_t nseg_max;            // segments of a full block: 1 when the tile pairs alone fill the device
  uint32_t pairs_per_launch;    // nseg_max * pairs_per_launch partial tiles fit the bound
};

// n_local: the shard's individuals; cus: compute units to fill; test_chunk / test_block: TSAMD_TEST_LD_CHUNK / TSAMD_TEST_LD_BLOCK
// (0: none)
TSAMD_LD_HD inline LdGeom ld_geometry(uint32_t n_local, uint32_t n_locs, uint32_t window, uint32_t cus, uint32_t test_chunk, uint32_t test_block) {
  LdGeom g;
  g.window = window;
  g.ov = ld_overlap_tiles(window);
  uint32_t ct = ld_ntiles(n_locs);
  if (ct > kLdMaxChunkTiles) ct = kLdMaxChunkTiles;
  const uint32_t acc_fit = (uint32_t)(kLdScratchBound / kLdTileBytes) / (g.ov + 1u);  // (>= 240 at the largest window)
  if (ct > acc_fit) ct = acc_fit;
  if (test_chunk > 0u && ct > ld_ntiles(test_chunk)) ct = ld_ntiles(test_chunk);
  if (ct < 1u) ct = 1u;
  g.chunk_tiles = ct;
  g.chunk = ct * kLdTile;
  g.lpad = (ct + g.ov) * kLdTile;
  // whole stages of 16 individuals, so that every block starts where ts_ld_resid reads the columns as aligned dwords; the test
  // hook alone gives blocks that start elsewhere
  constexpr uint32_t kStage = kLdStageSteps * kLdStep;
  uint64_t block = kLdScratchBound / (2ull * sizeof(double) * g.lpad) / kStage * kStage;  // (>= 3264 at 80 tiles)
  if (block > ld_round_step(n_local)) block = ld_round_step(n_local);
  if (test_block > 0u && block > ld_round_step(test_block)) block = ld_round_step(test_block);
  if (block < kLdStep) block = kLdStep;
  g.block = (uint32_t)block;
  g.max_pairs = ct * (g.ov + 1u);
  if (cus < 1u) cus = 1u;
  if (cus > 1024u) cus = 1024u;
  uint32_t nseg = g.max_pairs >= 2u * cus ? 1u : (2u * cus + g.max_pairs - 1u) / g.max_pairs;
  if (nseg > kLdMaxSegments) nseg = kLdMaxSegments;
  g.nseg_max = nseg;
  const uint64_t fit = kLdScratchBound / kLdTileBytes / nseg;  // (>= 64)
  g.pairs_per_launch = g.max_pairs < fit ? g.max_pairs : (uint32_t)fit;
  return g;
}

// segments of a block of len individuals, in k-steps: segment s covers steps [s seg_steps, min(steps, (s + 1) seg_steps))
struct LdSegs {
  uint32_t steps, nseg, seg_steps;
};
TSAMD_LD_HD inline LdSegs ld_segments(const LdGeom &g, uint32_t len) {
  LdSegs s;
  s.steps = ld_round_step(len) / kLdStep;
  uint32_t nseg = s.steps / kLdMinSegSteps;
  if (nseg > g.nseg_max) nseg = g.nseg_max;
  if (nseg < 1u) nseg = 1u;
  s.seg_steps = (s.steps + nseg - 1u) / nseg;
  s.nseg = s.seg_steps ? (s.steps + s.seg_steps - 1u) / s.seg_steps : 1u;
  return s;
}

// what chunk number c (locations [c chunk, ..) of the list) covers: len rows of its own, halo further locations it reads
struct LdChunk {
  uint32_t off, len, halo, rows, nt, npairs;
};
TSAMD_LD_HD inline LdChunk ld_chunk(const LdGeom &g, uint32_t n_locs, uint32_t off) {
  LdChunk c;
  c.off = off;
  c.len = n_locs - off < g.chunk ? n_locs - off : g.chunk;
  const uint32_t left = n_locs - off - c.len;
  c.halo = left < g.ov * kLdTile ? left : g.ov * kLdTile;
  c.rows = ld_ntiles(c.len);
  c.nt = ld_ntiles(c.len + c.halo);
  c.npairs = ld_npairs(c.rows, c.nt, g.ov);
  return c;
}

// bytes of the Z / M scratch, of the partial tiles, of a chunk's accumulators and of its rows of the band
TSAMD_LD_HD inline uint64_t ld_zm_bytes(const LdGeom &g) { return 2ull * g.block * g.lpad * sizeof(double); }
TSAMD_LD_HD inline uint64_t ld_part_bytes(const LdGeom &g) { return (uint64_t)g.nseg_max * g.pairs_per_launch * kLdTileBytes; }
TSAMD_LD_HD inline uint64_t ld_acc_bytes(const LdGeom &g) { return (uint64_t)g.max_pairs * kLdTileBytes; }
TSAMD_LD_HD inline uint64_t ld_band_bytes(const LdGeom &g) { return (uint64_t)g.chunk * (g.window + 1u) * (sizeof(double) + sizeof(uint32_t)); }

// ---- pure host functions (no context, no device) ----------------------------------------------------------------------------

// r = num / cnt (0 where cnt < 2) and p = erfc(|r| sqrt(cnt) / sqrt(2)) of every entry of a band; p may be NULL
inline void ld_statistics(const double *num, const uint32_t *cnt, uint64_t count, double *r, double *p) {
  for (uint64_t i = 0; i < count; ++i) {
    const double c = (double)cnt[i];
    const double v = cnt[i] >= 2u ? num[i] / c : 0.0;
    r[i] = v;
    if (p) p[i] = erfc(fabs(v) * sqrt(c) / sqrt(2.0));
  }
}

// positions in ascending order: i is dropped if and only if some KEPT position j in [i - W, i) has r[j][i - j]^2 > r2_max
inline void ld_prune(const double *r, uint32_t n_locs, uint32_t window, double r2_max, uint8_t *keep) {
  for (uint32_t i = 0; i < n_locs; ++i) {
    bool drop = false;
    for (uint32_t j = i > window ? i - window : 0u; j < i && !drop; ++j) {
      const double v = r[ld_band_index(j, i - j, window)];
      drop = keep[j] != 0u && v * v > r2_max;
    }
    keep[i] = drop ? 0u : 1u;
  }
}

#if defined(__HIPCC__)
// what one chunk's launches need (tsamd_ld.hip)
struct LdArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *gam;     // [K][npad]
  const double *lam;     // [l][K][2]
  const uint32_t *locs;  // the chunk's locations, then its overlap's: ncols of them
  uint32_t npad, n_local, K;
  uint32_t ncols, lpad;  // listed locations in Z / M, and its columns (whole tiles; those past ncols are zero)
  uint32_t ind0, blen, rows4;  // the block: individuals [ind0, ind0 + blen) of the shard, rounded up to k-steps
  double *z, *m;         // [rows4][lpad]
  double *part;          // [nseg][pairs of the launch][2][T * T]
  double *acc;           // [pairs of the chunk][2][T * T]
};
// Z and M of the block
void ld_launch_resid(const LdArgs &a, hipStream_t stream);
// pairs [pair0, pair0 + npairs) of the chunk (rows / nt / ov: ld_pair): the segments' tiles, then their addition in ascending
// order onto acc
void ld_launch_pairs(const LdArgs &a, const LdChunk &c, uint32_t ov, uint32_t pair0, uint32_t npairs, const LdSegs &sg, hipStream_t stream);
// the chunk's rows of the band from acc: num [len][window + 1] doubles, cnt likewise as uint32
void ld_launch_band(const LdArgs &a, const LdChunk &c, uint32_t ov, uint32_t window, double *num, uint32_t *cnt, hipStream_t stream);
#endif

}  // namespace tsamd
