// Stand-alone check of csrc/tsamd_ld_plan.h (no ROCm header, no GPU): the per-entry terms of tsamd_ld against long double, the
// band tile-pair enumeration (every pair (i, i + d) of the band in exactly one tile pair of exactly one chunk), chunk overlap,
// blocks and segments (every individual by exactly one k-step of one segment), the stated bounds on the scratch buffers, and
// ld_statistics / ld_prune on hand-made bands.  Built and run by tests/test_ld_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "tsamd_ld_plan.h"

using namespace tsamd;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++failures;                                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
    }                                            \
  } while (0)

static void check_terms() {
  std::vector<double> qs = {1e-300, 1e-200, 1e-17, 1e-9, 0.25, 0.5, 0.75, 1.0 - 1e-9, 1.0 - 1e-16};
  for (int i = 1; i < 1000; ++i) qs.push_back(i / 1000.0);
  for (int e = -290; e < 0; e += 7) qs.push_back(std::pow(10.0, e)), qs.push_back(1.0 - std::pow(10.0, e / 20.0 - 1.0));
  const long double want_y[4] = {0, 0, 1, 2};  // codes 00, 01 (no term), 10, 11
  for (double q : qs)
    for (uint32_t code = 0; code < 4; ++code) {
      double z = -7, m = -7;
      ld_terms(q, code, &z, &m);
      if (code == 1u) {
        CHECK(z == 0.0 && m == 0.0, "q = %.17g: code 01 gives (%g, %g)", q, z, m);
        continue;
      }
      const long double lq = q, lnum = want_y[code] - 2.0L * lq, lz = lnum / sqrtl(2.0L * lq * (1.0L - lq));
      // in units of u = 2^-53: the difference rounds once (2q is exact; where it cancels, y = 1 near q = 0.5, it is exact by
      // Sterbenz): 1 u.  1 - q and the product (2q)(1 - q) round once each, the root halves those 2 u and rounds itself: 2 u.  The
      // quotient rounds once more: 4 u = 4.44e-16 to first order.
      CHECK(fabsl((long double)z - lz) <= 4.5e-16L * fabsl(lz), "q = %.17g code = %u: z = %.17g, exact %.17Lg", q, code, z, lz);
      CHECK(m == 1.0 && std::isfinite(z), "q = %.17g code = %u: (%g, %g)", q, code, z, m);
    }
  // q outside (0, 1) by rounding: no term, never a NaN
  for (double q : {0.0, 1.0, 1.0 + 2.3e-16, -1e-18})
    for (uint32_t code = 0; code < 4; ++code) {
      double z, m;
      ld_terms(q, code, &z, &m);
      CHECK(z == 0.0 && m == 0.0, "q = %.17g code = %u: (%g, %g)", q, code, z, m);
    }
}

// every pair (i, i + d), d <= W, i + d < n_locs, lies in the rows of exactly one chunk and there in exactly one enumerated tile
// pair; no tile pair is enumerated twice or lies outside the band; the chunks' rows cover the list once
static void check_band(uint32_t n_locs, uint32_t window, uint32_t test_chunk) {
  const LdGeom g = ld_geometry(1000, n_locs, window, 256, test_chunk, 0);
  CHECK(g.ov == (window + 63u) / 64u && g.chunk == g.chunk_tiles * kLdTile && g.lpad == (g.chunk_tiles + g.ov) * kLdTile, "L = %u W = %u: geometry", n_locs, window);
  uint32_t bad = 0, rows_seen = 0;
  for (uint32_t off = 0; off < n_locs; off += g.chunk) {
    const LdChunk c = ld_chunk(g, n_locs, off);
    bad += !(c.len >= 1u && c.len <= g.chunk && c.off == off && c.rows == ld_ntiles(c.len) && c.nt >= c.rows && c.nt <= c.rows + g.ov);
    bad += !((uint64_t)c.nt * kLdTile <= g.lpad && c.npairs <= g.max_pairs && c.npairs >= c.rows);
    // overlap: what a chunk reads beyond its rows is what its last row's window needs, as far as the list goes
    const uint32_t need = n_locs - off - c.len < window ? n_locs - off - c.len : window;
    bad += !(c.halo >= need && c.halo <= g.ov * kLdTile && off + c.len + c.halo <= n_locs);
    if (off + c.len < n_locs) bad += c.len != g.chunk;  // only the last chunk is short
    rows_seen += c.len;
    std::map<uint64_t, uint32_t> index;  // (ti, tj) -> p
    LdPair prev{0, 0};
    for (uint32_t p = 0; p < c.npairs; ++p) {
      const LdPair pr = ld_pair(p, c.rows, c.nt, g.ov);
      if (!(pr.ti < c.rows && pr.ti <= pr.tj && pr.tj < c.nt && pr.tj <= pr.ti + g.ov)) {
        ++bad;
        continue;
      }
      bad += index.count((uint64_t)pr.ti << 32 | pr.tj) != 0u;
      index[(uint64_t)pr.ti << 32 | pr.tj] = p;
      bad += p != ld_row_first(pr.ti, c.rows, c.nt, g.ov) + (pr.tj - pr.ti);
      bad += pr.tj - pr.ti >= ld_row_pairs(pr.ti, c.nt, g.ov);
      if (p > 0u) bad += !(pr.ti == prev.ti ? pr.tj == prev.tj + 1u : pr.ti == prev.ti + 1u && pr.tj == pr.ti);  // row by row
      prev = pr;
    }
    uint64_t rows_pairs = 0;
    for (uint32_t ti = 0; ti < c.rows; ++ti) rows_pairs += ld_row_pairs(ti, c.nt, g.ov);
    bad += rows_pairs != c.npairs;
    for (uint32_t i = 0; i < c.len; ++i)
      for (uint32_t d = 0; d <= window && off + i + d < n_locs; ++d) {
        const uint32_t j = i + d;
        bad += !(j < c.len + c.halo);
        bad += index.count((uint64_t)(i / kLdTile) << 32 | j / kLdTile) != 1u;
      }
  }
  bad += rows_seen != n_locs;
  CHECK(bad == 0, "L = %u W = %u chunk = %u: %u pairs, tiles or chunks wrong", n_locs, window, test_chunk, bad);
}

static void check_geometry(uint32_t n_local, uint32_t n_locs, uint32_t window) {
  for (uint32_t cus : {1u, 4u, 64u, 256u, 304u})
    for (uint32_t test_chunk : {0u, 1u, 64u, 128u, 4097u})
      for (uint32_t test_block : {0u, 1u, 64u, 260u, 100000u}) {
        const LdGeom g = ld_geometry(n_local, n_locs, window, cus, test_chunk, test_block);
        CHECK(g.chunk_tiles >= 1u && g.chunk_tiles <= kLdMaxChunkTiles && g.chunk_tiles <= ld_ntiles(n_locs), "chunk tiles %u", g.chunk_tiles);
        if (test_chunk) CHECK(g.chunk_tiles <= ld_ntiles(test_chunk), "TSAMD_TEST_LD_CHUNK = %u not honoured: %u tiles", test_chunk, g.chunk_tiles);
        CHECK(g.block >= kLdStep && g.block % kLdStep == 0u && g.block <= ld_round_step(n_local), "n = %u: block %u", n_local, g.block);
        if (test_block) CHECK(g.block <= ld_round_step(test_block), "TSAMD_TEST_LD_BLOCK = %u not honoured: %u", test_block, g.block);
        // without the hook every block starts on a whole stage of 16 individuals: the columns are read as aligned dwords
        if (!test_block && g.block < n_local) CHECK(g.block % (kLdStageSteps * kLdStep) == 0u, "n = %u: block %u starts the next one off a dword", n_local, g.block);
        CHECK(g.nseg_max >= 1u && g.nseg_max <= kLdMaxSegments, "cus = %u: %u segments", cus, g.nseg_max);
        if (g.max_pairs >= 2u * cus) CHECK(g.nseg_max == 1u, "segments though the tile pairs fill the device");
        if (g.nseg_max < kLdMaxSegments) CHECK((uint64_t)g.nseg_max * g.max_pairs >= 2u * cus, "cus = %u: the grid does not fill the device", cus);
        CHECK(g.pairs_per_launch >= 1u && g.pairs_per_launch <= g.max_pairs, "%u pairs per launch", g.pairs_per_launch);
        // the bounds: Z / M, the partial tiles and a chunk's accumulators under 256 MB each; the chunk's band rows with them
        CHECK(ld_zm_bytes(g) <= kLdScratchBound, "n = %u L = %u W = %u: %llu bytes of Z / M", n_local, n_locs, window, (unsigned long long)ld_zm_bytes(g));
        CHECK(ld_part_bytes(g) <= kLdScratchBound, "%llu bytes of partials", (unsigned long long)ld_part_bytes(g));
        CHECK(ld_acc_bytes(g) <= kLdScratchBound, "W = %u: %llu bytes of accumulators", window, (unsigned long long)ld_acc_bytes(g));
        CHECK(ld_band_bytes(g) <= 64ull << 20, "W = %u: %llu bytes of band rows", window, (unsigned long long)ld_band_bytes(g));
        // blocks and their segments, as tsamd_ld walks them: every individual by exactly one k-step of one segment of one block
        std::vector<uint8_t> seen(n_local, 0);
        uint32_t bad = 0;
        for (uint32_t i0 = 0; i0 < n_local; i0 += g.block) {
          const uint32_t len = n_local - i0 < g.block ? n_local - i0 : g.block;
          const LdSegs sg = ld_segments(g, len);
          bad += !(sg.steps * kLdStep == ld_round_step(len) && sg.steps * kLdStep <= g.block);
          bad += !(sg.nseg >= 1u && sg.nseg <= g.nseg_max);
          if (sg.nseg > 1u) bad += sg.seg_steps < kLdMinSegSteps;
          for (uint32_t seg = 0; seg < sg.nseg; ++seg) {
            const uint32_t b = seg * sg.seg_steps, e = b + sg.seg_steps < sg.steps ? b + sg.seg_steps : sg.steps;
            bad += !(b < e);  // no empty segment
            for (uint32_t st = b; st < e; ++st)
              for (uint32_t i = 0; i < kLdStep; ++i)
                if (st * kLdStep + i < len) ++seen[i0 + st * kLdStep + i];
          }
        }
        for (uint32_t i = 0; i < n_local; ++i) bad += seen[i] != 1;
        CHECK(bad == 0, "n = %u cus = %u block = %u: %u individuals or segments wrong", n_local, cus, test_block, bad);
      }
}

static void check_statistics_and_prune() {
  // ld_statistics: cnt < 2 gives r = 0, p = 1; otherwise num / cnt and erfc(|r| sqrt(cnt) / sqrt 2)
  const double num[6] = {5.0, 0.7, -30.0, 0.0, 3.0, -0.25};
  const uint32_t cnt[6] = {0, 1, 100, 50, 2, 4};
  double r[6], p[6], r2[6];
  ld_statistics(num, cnt, 6, r, p);
  ld_statistics(num, cnt, 6, r2, nullptr);
  for (int i = 0; i < 6; ++i) CHECK(r[i] == r2[i], "p == NULL changes r");
  CHECK(r[0] == 0.0 && p[0] == 1.0 && r[1] == 0.0 && p[1] == 1.0, "cnt < 2: r = %g %g, p = %g %g", r[0], r[1], p[0], p[1]);
  CHECK(r[2] == -0.3 && fabs(p[2] - erfc(3.0 / sqrt(2.0))) <= 1e-15 * p[2], "r = %g p = %g", r[2], p[2]);
  CHECK(r[3] == 0.0 && p[3] == 1.0 && r[4] == 1.5 && r[5] == -0.0625, "r = %g %g %g", r[3], r[4], r[5]);
  CHECK(fabs(p[5] - erfc(0.0625 * 2.0 / sqrt(2.0))) <= 1e-15, "p = %g", p[5]);

  // ld_prune.  A chain a - b - c (positions 1, 2, 3; window 2): b is dropped for a, so c, linked to b only, is spared.
  {
    const uint32_t n = 5, w = 2;
    std::vector<double> band((size_t)n * (w + 1u), 0.0);
    for (uint32_t i = 0; i < n; ++i) band[ld_band_index(i, 0, w)] = 1.0;  // (the diagonal is never looked at)
    band[ld_band_index(1, 1, w)] = 0.9;   // a - b
    band[ld_band_index(2, 1, w)] = -0.9;  // b - c
    std::vector<uint8_t> keep(n, 7);
    ld_prune(band.data(), n, w, 0.5, keep.data());
    CHECK(keep[0] == 1 && keep[1] == 1 && keep[2] == 0 && keep[3] == 1 && keep[4] == 1, "chain: %u %u %u %u %u", keep[0], keep[1], keep[2], keep[3], keep[4]);
    band[ld_band_index(1, 2, w)] = 0.8;  // a - c as well: now c goes too
    ld_prune(band.data(), n, w, 0.5, keep.data());
    CHECK(keep[1] == 1 && keep[2] == 0 && keep[3] == 0 && keep[4] == 1, "chain with a - c: %u %u %u", keep[1], keep[2], keep[3]);
    // the threshold is strict: r^2 == r2_max stays
    ld_prune(band.data(), n, w, 0.81, keep.data());
    CHECK(keep[2] == 1 && keep[3] == 1, "r^2 == r2_max: %u %u", keep[2], keep[3]);
    ld_prune(band.data(), n, w, 0.0, keep.data());
    CHECK(keep[0] == 1 && keep[1] == 1 && keep[2] == 0 && keep[3] == 0 && keep[4] == 1, "r2_max = 0");
  }
  // the window's edge: with window 3, positions 0 and 3 are neighbours (column 3), 0 and 4 are not -- a band has no column for them
  {
    const uint32_t n = 6, w = 3;
    std::vector<double> band((size_t)n * (w + 1u), 0.0);
    band[ld_band_index(0, 3, w)] = 1.0;
    band[ld_band_index(1, 3, w)] = 0.2;  // below the threshold
    std::vector<uint8_t> keep(n, 7);
    ld_prune(band.data(), n, w, 0.5, keep.data());
    CHECK(keep[0] == 1 && keep[1] == 1 && keep[2] == 1 && keep[3] == 0 && keep[4] == 1 && keep[5] == 1, "window edge: %u %u", keep[3], keep[4]);
    // n_locs <= window: rows shorter than the band
    std::vector<double> small(2u * (w + 1u), 0.0);
    small[ld_band_index(0, 1, w)] = -1.0;
    small[ld_band_index(0, 2, w)] = 1.0, small[ld_band_index(1, 3, w)] = 1.0;  // (columns past the list: never read)
    ld_prune(small.data(), 2, w, 0.5, keep.data());
    CHECK(keep[0] == 1 && keep[1] == 0, "n_locs <= window: %u %u", keep[0], keep[1]);
  }
}

int main() {
  check_terms();
  for (uint32_t window : {1u, 63u, 64u, 65u, 130u, 1024u})
    for (uint32_t n_locs : {1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 200u, 1024u, 1025u, 4096u, 4097u, 8300u})
      for (uint32_t test_chunk : {0u, 64u, 128u}) check_band(n_locs, window, test_chunk);
  for (uint32_t n_local : {1u, 3u, 4u, 5u, 17u, 600u, 2100u, 70001u})
    for (uint32_t n_locs : {1u, 70u, 4096u, 100000u})
      for (uint32_t window : {1u, 64u, 65u, 1024u}) check_geometry(n_local, n_locs, window);
  // the rate shape: 4096 locations in one chunk of 64 tiles, 4 overlap tiles at W = 256, 3840 individuals per block
  LdGeom g = ld_geometry(1000000, 4096, 256, 256, 0, 0);
  CHECK(g.chunk_tiles == 64 && g.ov == 4 && g.lpad == 4352 && g.block == 3840 && g.max_pairs == 320 && g.nseg_max == 2, "N = 1M: block %u, %u pairs, %u segments",
        g.block, g.max_pairs, g.nseg_max);
  LdChunk c = ld_chunk(g, 4096, 0);
  CHECK(c.len == 4096 && c.halo == 0 && c.nt == 64 && c.npairs == 60 * 5 + 4 + 3 + 2 + 1, "the only chunk: %u pairs", c.npairs);
  // the widest window: 17 pairs per tile row, the accumulators hold 64 rows of them
  g = ld_geometry(1000000, 100000, kLdMaxWindow, 256, 0, 0);
  CHECK(g.ov == 16 && g.chunk_tiles == 64 && g.max_pairs == 1088 && g.nseg_max == 1 && g.block == 3264, "W = 1024: %u tiles, block %u", g.chunk_tiles, g.block);
  check_statistics_and_prune();
  printf("ld: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
