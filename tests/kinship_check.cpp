// Stand-alone check of csrc/tsamd_kin_plan.h (no ROCm header, no GPU): the per-entry terms of tsamd_kinship against long
// double, the tile-pair enumeration (the upper triangle of tiles exactly once), segments and chunks (every listed position
// exactly once) and the stated bounds on the scratch buffers.  Built and run by tests/test_kinship_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tsamd_kin_plan.h"

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
      double r = -7, s = -7;
      kin_terms(q, code, &r, &s);
      if (code == 1u) {
        CHECK(r == 0.0 && s == 0.0, "q = %.17g: code 01 gives (%g, %g)", q, r, s);
        continue;
      }
      const long double lr = want_y[code] - 2.0L * q, ls = sqrtl((long double)q * (1.0L - (long double)q));
      // r: one rounding of the difference (2q is exact).  s: 1 - q, the product and the root round once each (the root halves
      // what the first two carry): 2 ulp.  1 - q is exact above q = 0.5 (Sterbenz) and below loses at most an ulp of 1.
      CHECK(fabsl((long double)r - lr) <= 1.2e-16L * fabsl(lr), "q = %.17g code = %u: r = %.17g, exact %.17Lg", q, code, r, lr);
      CHECK(fabsl((long double)s - ls) <= 2.5e-16L * ls, "q = %.17g code = %u: s = %.17g, exact %.17Lg", q, code, s, ls);
      CHECK(s > 0.0 && std::isfinite(s) && std::isfinite(r), "q = %.17g: (%g, %g)", q, r, s);
    }
  // q outside (0, 1) by rounding: no NaN
  for (double q : {0.0, 1.0, 1.0 + 2.3e-16, -1e-18}) {
    double r, s;
    kin_terms(q, 3u, &r, &s);
    CHECK(s == 0.0 && std::isfinite(r), "q = %.17g: s = %g", q, s);
  }
}

static void check_pairs(uint32_t m) {
  const uint32_t nt = kin_ntiles(m), mpad = kin_mpad(m), np = kin_npairs(nt);
  CHECK(mpad >= m && mpad - m < kKinTile && mpad == nt * kKinTile, "m = %u: mpad = %u, %u tiles", m, mpad, nt);
  std::vector<uint8_t> seen((size_t)nt * nt, 0);
  uint32_t bad = 0;
  KinPair prev{0, 0};
  for (uint32_t p = 0; p < np; ++p) {
    const KinPair pr = kin_pair(p, nt);
    if (!(pr.ti <= pr.tj && pr.tj < nt)) {
      ++bad;
      continue;
    }
    ++seen[(size_t)pr.ti * nt + pr.tj];
    if (p > 0u) bad += !(pr.ti == prev.ti ? pr.tj == prev.tj + 1u : pr.ti == prev.ti + 1u && pr.tj == pr.ti && prev.tj == nt - 1u);  // row by row
    prev = pr;
  }
  for (uint32_t i = 0; i < nt; ++i)
    for (uint32_t j = 0; j < nt; ++j) bad += seen[(size_t)i * nt + j] != (i <= j ? 1 : 0);
  CHECK(bad == 0, "m = %u: %u tile pairs wrong (%u pairs of %u tiles)", m, bad, np, nt);
}

static void check_geometry(uint32_t m, uint32_t n_locs) {
  for (uint32_t cus : {1u, 4u, 64u, 256u, 304u})
    for (uint32_t test_chunk : {0u, 1u, 5u, 4097u})
      for (uint32_t test_segments : {0u, 1u, 3u, 1000u}) {
        KinGeom g = kin_geometry(m, cus, test_chunk, test_segments);
        CHECK(g.mpad == kin_mpad(m) && g.ntiles * kKinTile == g.mpad && g.npairs == kin_npairs(g.ntiles), "m = %u: the tiles", m);
        CHECK(g.chunk >= 1u && g.chunk <= kKinMaxChunk && (test_chunk ? g.chunk <= test_chunk : g.chunk % kKinStep == 0u), "m = %u: chunk %u", m, g.chunk);
        CHECK(g.nseg_max >= 1u && g.nseg_max <= kKinMaxSegments, "m = %u cus = %u: %u segments", m, cus, g.nseg_max);
        if (test_segments) CHECK(g.nseg_max <= test_segments, "test segments not honoured");
        if (!test_segments && g.npairs >= 2u * cus) CHECK(g.nseg_max == 1u, "m = %u cus = %u: segments though the tile pairs fill the device", m, cus);
        if (!test_segments && g.nseg_max < kKinMaxSegments) CHECK((uint64_t)g.nseg_max * g.npairs >= 2u * cus, "m = %u cus = %u: the grid does not fill the device", m, cus);
        CHECK(g.pairs_per_launch >= 1u && g.pairs_per_launch <= g.npairs, "m = %u: %u pairs per launch", m, g.pairs_per_launch);
        // the bounds: r / s scratch and partials under 256 MB each
        CHECK(kin_rs_bytes(g) <= kKinScratchBound, "m = %u: %llu bytes of r / s", m, (unsigned long long)kin_rs_bytes(g));
        CHECK(kin_part_bytes(g) <= kKinScratchBound, "m = %u cus = %u: %llu bytes of partials", m, cus, (unsigned long long)kin_part_bytes(g));
        CHECK(kin_acc_bytes(g) == 16ull * g.mpad * g.mpad, "the accumulators");
        // pair launches: [p0, p0 + pairs_per_launch) cover the pairs once
        uint64_t covered = 0;
        for (uint32_t p0 = 0; p0 < g.npairs; p0 += g.pairs_per_launch) covered += g.npairs - p0 < g.pairs_per_launch ? g.npairs - p0 : g.pairs_per_launch;
        CHECK(covered == g.npairs, "m = %u: pair launches cover %llu of %u", m, (unsigned long long)covered, g.npairs);
        // chunks and their segments, as tsamd_kinship walks them: every listed position by exactly one k-step of one segment
        if (g.chunk > n_locs) g.chunk = n_locs;
        std::vector<uint8_t> seen(n_locs, 0);
        uint32_t bad = 0;
        for (uint32_t off = 0; off < n_locs; off += g.chunk) {
          const uint32_t len = n_locs - off < g.chunk ? n_locs - off : g.chunk;
          const KinSegs sg = kin_segments(g, len);
          bad += !(sg.steps * kKinStep == kin_round_step(len) && sg.steps * kKinStep >= len && sg.steps * kKinStep - len < kKinStep);
          bad += !(sg.nseg >= 1u && sg.nseg <= g.nseg_max && kin_round_step(len) <= kin_round_step(g.chunk));
          if (sg.nseg > 1u) bad += sg.seg_steps < kKinMinSegSteps;
          for (uint32_t seg = 0; seg < sg.nseg; ++seg) {
            const uint32_t b = seg * sg.seg_steps, e = b + sg.seg_steps < sg.steps ? b + sg.seg_steps : sg.steps;
            bad += !(b < e);  // no empty segment
            for (uint32_t st = b; st < e; ++st)
              for (uint32_t i = 0; i < kKinStep; ++i)
                if (st * kKinStep + i < len) ++seen[off + st * kKinStep + i];
          }
        }
        for (uint32_t i = 0; i < n_locs; ++i) bad += seen[i] != 1;
        CHECK(bad == 0, "m = %u n_locs = %u cus = %u chunk = %u segments = %u: %u positions or segments wrong", m, n_locs, cus, test_chunk, test_segments, bad);
      }
}

int main() {
  check_terms();
  for (uint32_t m : {1u, 63u, 64u, 65u, 200u, 32768u}) check_pairs(m);
  for (uint32_t m : {1u, 63u, 64u, 65u, 200u, 4096u, 32768u})
    for (uint32_t n_locs : {1u, 3u, 4u, 5u, 17u, 33u, 130u, 4099u, 70001u}) check_geometry(m, n_locs);
  // the rate shape: 2080 tile pairs fill 256 compute units on their own; 256 MB of r / s are 4096 locations at a time
  KinGeom g = kin_geometry(4096, 256, 0, 0);
  CHECK(g.ntiles == 64 && g.npairs == 2080 && g.nseg_max == 1 && g.chunk == 4096 && g.pairs_per_launch == 2080, "m = 4096: %u pairs, %u segments, chunk %u",
        g.npairs, g.nseg_max, g.chunk);
  // a family-sized list: 10 pairs, the segments carry the grid
  g = kin_geometry(200, 256, 0, 0);
  CHECK(g.ntiles == 4 && g.npairs == 10 && g.nseg_max == 52, "m = 200: %u pairs, %u segments", g.npairs, g.nseg_max);
  // the largest list: 131 328 pairs in launches of 4096, chunks of 512 locations
  g = kin_geometry(kKinMaxM, 256, 0, 0);
  CHECK(g.npairs == 131328 && g.pairs_per_launch == 4096 && g.chunk == 512 && g.nseg_max == 1, "m = 32768: %u pairs, %u per launch, chunk %u", g.npairs,
        g.pairs_per_launch, g.chunk);
  printf("kinship: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
