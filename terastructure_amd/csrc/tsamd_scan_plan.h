// tsamd_snp_scan / tsamd_scan_statistics: the per-entry terms, the statistics formulas and the tile / segment / chunk geometry,
// as plain C++ that the host, the kernels (tsamd_scan_kernels.h) and a stand-alone check without any ROCm header
// (tests/snp_scan_check.cpp) share.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tsamd_sweep_plan.h"

#if defined(__HIPCC__)
#define TSAMD_SC_HD __host__ __device__
#else
#define TSAMD_SC_HD
#endif

namespace tsamd {

constexpr uint32_t kScanBlock = 256;                  // threads per workgroup
constexpr uint32_t kScanBatch = 32;                   // locations whose Ebeta a workgroup keeps in LDS at a time
constexpr uint32_t kScanMaxSegments = 64;             // location segments per chunk (small shards)
constexpr uint32_t kScanMaxChunk = 1u << 16;          // locations per chunk, at most
constexpr uint64_t kScanScratchBound = 256ull << 20;  // bytes of the partial-sum buffer, at most (shards up to 11M individuals)

// the values a location carries through the fold, in this order: a partial is scan_values(trait) doubles
enum : int {
  kScanE0 = 0,  // sum (1-q)^2
  kScanE1,      // sum h,  h = 2q(1-q)
  kScanE2,      // sum q^2
  kScanVH,      // sum h(1-h)
  kScanO0,      // entries with y = 0, 1, 2 (exact integers in a double)
  kScanO1,
  kScanO2,
  kScanFitValues,  // = 7: what a call without a trait carries
  kScanT = kScanFitValues,  // sum t
  kScanTR,                  // sum t r,  r = y - 2q
  kScanTTH,                 // sum t^2 h
  kScanTH,                  // sum t h
  kScanR,                   // sum r
  kScanH,                   // sum h
  kScanNT,                  // phenotyped entries (an exact integer in a double)
  kScanTraitValues          // = 14
};
constexpr uint32_t kScanFitSums = 4, kScanFitCounts = 3, kScanTraitSums = 6, kScanStats = 6;

TSAMD_SC_HD constexpr uint32_t scan_values(bool trait) { return trait ? (uint32_t)kScanTraitValues : (uint32_t)kScanFitValues; }

// individuals per thread: IPT * K doubles of normalised theta (at most 64, 128 VGPRs) stay in the thread's registers for all
// the locations it visits, the thread's trait values beside them.  0 stands for the run-time-K path (K above
// TSAMD_SPECIALIZED_K): theta comes from a scratch array.  Starts from loglik_ipt; the trait form carries 14 sums, 2 IPT
// doubles of trait and mask and three more products per entry, and stays inside the 256 architected VGPRs with half the
// individuals at K <= 4 (profiles/r06_kernel_resources.txt: no instantiation spills).
TSAMD_SC_HD constexpr uint32_t scan_ipt(uint32_t K, bool trait) {
  return K == 0u || K > 32u ? 1u : K <= 4u ? (trait ? 8u : 16u) : K <= 8u ? 8u : K <= 16u ? 4u : 2u;
}

// PLINK 2-bit code -> genotype as code_weights does (tsamd_device.h): 00 -> 0, 10 -> 1, 11 -> 2; 01 has no term
TSAMD_SC_HD inline uint32_t scan_code_y(uint32_t c) { return (c >> 1) * (1u + (c & 1u)); }
TSAMD_SC_HD inline uint32_t scan_code_ok(uint32_t c) { return ((c & 1u) & ((c >> 1) ^ 1u)) ^ 1u; }

// One entry's terms added onto v[0 .. scan_values(TRAIT)): q the individual-specific allele frequency, c the stored 2-bit code,
// t the trait value with 0 in place of NaN, pm = 1 where the individual is phenotyped and 0 where not.  The stored-entry mask
// and the phenotyped mask enter as factors (0 or 1), so an entry that does not count adds exact zeros; no branch, no
// division, no log.
template <bool TRAIT>
TSAMD_SC_HD inline void scan_add_entry(double q, uint32_t c, double t, double pm, double *v) {
  const uint32_t ok = scan_code_ok(c), hi = c >> 1, lo = c & 1u;
  const uint32_t is2 = hi & lo, is1 = hi & (lo ^ 1u);  // (01 gives neither)
  const double m = (double)ok, d1 = (double)is1, d2 = (double)is2;
  const double omq = 1.0 - q;
  const double h = 2.0 * q * omq;
  v[kScanE0] += m * (omq * omq);
  v[kScanE1] += m * h;
  v[kScanE2] += m * (q * q);
  v[kScanVH] += m * (h * (1.0 - h));
  v[kScanO0] += m - d1 - d2;
  v[kScanO1] += d1;
  v[kScanO2] += d2;
  if (TRAIT) {
    const double y = d1 + 2.0 * d2;
    const double r = y - 2.0 * q;
    const double mt = m * pm, a = m * t;  // (t is 0 where pm is)
    const double th = a * h;
    v[kScanT] += a;
    v[kScanTR] += a * r;
    v[kScanTTH] += t * th;
    v[kScanTH] += th;
    v[kScanR] += mt * r;
    v[kScanH] += mt * h;
    v[kScanNT] += mt;
  }
}

// z and p of one location from its sufficient statistics (added across ranks by the caller): stats[0 .. 6) =
// z_het, p_het, z_freq, p_freq, z_trait, p_trait; z = 0 and p = 1 where a denominator is not positive, where fewer than two
// individuals carry a trait value, or where trait_sums is NULL
inline double scan_p_value(double z) { return erfc(fabs(z) / sqrt(2.0)); }
inline void scan_statistics_row(const double *fit_sums, const uint32_t *fit_counts, const double *trait_sums, uint32_t trait_count,
                                double *stats) {
  const double e1 = fit_sums[1], e2 = fit_sums[2], vh = fit_sums[3];
  const double o1 = (double)fit_counts[1], o2 = (double)fit_counts[2];
  const double z_het = vh > 0.0 ? (o1 - e1) / sqrt(vh) : 0.0;  // O1 is a sum of independent Bernoulli(h)
  const double z_freq = e1 > 0.0 ? ((o1 + 2.0 * o2) - (e1 + 2.0 * e2)) / sqrt(e1) : 0.0;  // Var y = h
  double z_trait = 0.0;
  if (trait_sums && trait_count >= 2u) {
    const double c = trait_sums[0] / (double)trait_count;  // the trait's mean among the contributing individuals
    const double u = trait_sums[1] - c * trait_sums[4];
    const double v = trait_sums[2] - 2.0 * c * trait_sums[3] + c * c * trait_sums[5];
    if (v > 0.0) z_trait = u / sqrt(v);
  }
  stats[0] = z_het, stats[1] = scan_p_value(z_het);
  stats[2] = z_freq, stats[3] = scan_p_value(z_freq);
  stats[4] = z_trait, stats[5] = scan_p_value(z_trait);
}

// One call = chunks of at most `chunk` listed locations; a chunk = a grid of ntiles x nseg workgroups: workgroup
// (tile, seg) takes the tile's tile_n individuals through the chunk's locations [seg * seg_len, (seg + 1) * seg_len).
// There are no per-individual outputs: the segments only split the list, the one buffer is part [chunk][ntiles][values].
struct ScanGeom {
  uint32_t ipt, tile_n, ntiles, values;
  uint32_t nseg_max;  // segments of a full chunk: 1 when the tiles alone fill the device
  uint32_t chunk;     // locations per chunk
};

// npad: the shard's padded width (a multiple of 512); cus: compute units to fill; test_chunk: TSAMD_TEST_SCAN_CHUNK (0: none)
TSAMD_SC_HD inline ScanGeom scan_geometry(uint32_t npad, uint32_t K, bool trait, uint32_t cus, uint32_t test_chunk) {
  ScanGeom g;
  g.ipt = scan_ipt(K, trait);
  g.tile_n = kScanBlock * g.ipt;
  g.ntiles = (npad + g.tile_n - 1u) / g.tile_n;
  g.values = scan_values(trait);
  g.nseg_max = (uint32_t)sweep_fill_segments(g.ntiles, cus, kScanMaxSegments);
  uint64_t chunk = kScanScratchBound / ((uint64_t)g.ntiles * g.values * sizeof(double));
  if (chunk > kScanMaxChunk) chunk = kScanMaxChunk;
  if (test_chunk > 0u && chunk > test_chunk) chunk = test_chunk;
  if (chunk < 1u) chunk = 1u;
  g.chunk = (uint32_t)chunk;
  return g;
}

// segments of a chunk of len locations (sweep_segments, tsamd_sweep_plan.h)
using ScanSegs = SweepSegs;
TSAMD_SC_HD inline ScanSegs scan_segments(const ScanGeom &g, uint32_t len) { return sweep_segments(g.nseg_max, len); }

// bytes of the partial-sum buffer of a geometry
TSAMD_SC_HD inline uint64_t scan_scratch_bytes(const ScanGeom &g) {
  return (uint64_t)g.chunk * g.ntiles * g.values * sizeof(double);
}

#if defined(__HIPCC__)
// what one chunk's launches need (tsamd_scan.hip)
struct ScanArgs {
  const uint8_t *bed;
  uint64_t colstride;
  const double *gam;     // [K][npad]
  const double *thn;     // run-time-K path: normalised theta [K][npad]
  const double *lam;     // [l][K][2]
  const double *trait;   // [npad], NaN = not phenotyped (padding included); NULL without a trait
  const uint32_t *locs;  // the chunk's locations
  uint32_t npad, K, len, seg_len, ntiles;
  double *part;          // [len][ntiles][values]
};
// the sweep of one chunk on a grid of (ntiles, nseg), then the index-order addition of a location's tiles into out_sums
// [len][10] (the fit sums, then the trait sums) and out_counts [len][4] (y = 0, 1, 2, then the phenotyped entries)
void scan_launch_chunk(const ScanArgs &a, uint32_t nseg, double *out_sums, uint32_t *out_counts, hipStream_t stream);
#endif

}  // namespace tsamd
