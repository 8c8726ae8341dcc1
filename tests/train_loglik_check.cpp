// Stand-alone check of csrc/tsamd_loglik_plan.h (no ROCm header, no GPU): the per-entry term of tsamd_train_loglik against
// long double, and the tile / segment / chunk geometry -- every (tile, segment, chunk) covers its individuals and locations
// exactly once and the partial-sum buffers stay under the stated bound.  Built and run by tests/test_train_loglik_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tsamd_loglik_plan.h"

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

static long double exact_term(long double q, uint32_t y) {
  const long double r = 1.0L - q;
  long double p = y == 0 ? r * r : y == 1 ? 2.0L * q * r : q * q;
  if (p < 1e-30L) p = 1e-30L;
  return logl(p);
}

static void check_term() {
  std::vector<double> qs;
  for (int i = 0; i <= 1000; ++i) qs.push_back(i / 1000.0);
  for (int e = -20; e <= -1; ++e) qs.push_back(std::pow(10.0, e)), qs.push_back(1.0 - std::pow(10.0, e));
  // both sides of the clamp: q^2 = 1e-30 at q = 1e-15, 2 q (1 - q) = 1e-30 at q = 5e-31, (1 - q)^2 = 1e-30 at 1 - q = 1e-15
  for (double f : {0.5, 0.9, 0.999999, 1.0, 1.000001, 1.1, 2.0}) {
    qs.push_back(1e-15 * f);
    qs.push_back(5e-31 * f);
    qs.push_back(1.0 - 1e-15 * f);
  }
  const double floor30 = std::log(1e-30);
  for (double q : qs)
    for (uint32_t y = 0; y < 3; ++y) {
      const double got = loglik_term(q, y);
      const long double want = exact_term((long double)q, y);
      // the product carries at most 3 roundings (1 - q, a * b; the doubling is exact): 3 * 2^-53 relative, which moves the log
      // by as much absolutely; the log itself adds an ulp of a result whose magnitude is at most 69.1
      const long double tol = 4.0L * 1.2e-16L + 2.0L * fabsl(want) * 1.2e-16L;
      CHECK(fabsl((long double)got - want) <= tol, "term(q = %.17g, y = %u) = %.17g, exact %.17Lg", q, y, got, want);
      CHECK(got <= 0.0 && got >= floor30, "term(q = %.17g, y = %u) = %.17g out of [log 1e-30, 0]", q, y, got);
      const long double r = 1.0L - (long double)q;
      const long double p = y == 0 ? r * r : y == 1 ? 2.0L * q * r : (long double)q * q;
      if (p < 0.99e-30L) CHECK(got == floor30, "term(q = %.17g, y = %u) = %.17g is not the clamp", q, y, got);
      if (p > 1.01e-30L) CHECK(got > floor30, "term(q = %.17g, y = %u) clamped above the floor", q, y);
    }
  // codes: 00 -> 0, 10 -> 1, 11 -> 2 (the bit pairs as stored: code = 2 * high bit + low bit), 01 has no term
  CHECK(loglik_code_ok(0) && loglik_code_y(0) == 0, "code 00");
  CHECK(!loglik_code_ok(1), "code 01");
  CHECK(loglik_code_ok(2) && loglik_code_y(2) == 1, "code 10");
  CHECK(loglik_code_ok(3) && loglik_code_y(3) == 2, "code 11");
}

static void check_geometry(uint32_t n, uint32_t n_locs) {
  const uint32_t npad = (n + 511u) / 512u * 512u;
  for (uint32_t K : {1u, 4u, 5u, 8u, 9u, 16u, 17u, 32u, 33u, 128u})
    for (uint32_t cus : {1u, 2u, 256u, 304u})
      for (uint32_t test_chunk : {0u, 1u, 5u}) {
        const LoglikGeom g = loglik_geometry(npad, K, cus, test_chunk);
        CHECK(g.ipt * K <= 64u || K > 32u, "K = %u: %u individuals per thread", K, g.ipt);
        CHECK(g.ipt == 1u || 16u % g.ipt == 0u, "K = %u: a thread's individuals do not share one 32-bit word", K);
        CHECK(g.tile_n == 256u * g.ipt && (uint64_t)g.ntiles * g.tile_n >= npad && (uint64_t)(g.ntiles - 1u) * g.tile_n < npad,
              "n = %u K = %u: %u tiles of %u", n, K, g.ntiles, g.tile_n);
        CHECK(g.chunk >= 1u && g.nseg_max >= 1u && g.nseg_max <= kLoglikMaxSegments, "n = %u K = %u", n, K);
        CHECK(loglik_scratch_bytes(g, npad) <= kLoglikScratchBound, "n = %u K = %u cus = %u: %llu bytes of partials", n, K, cus,
              (unsigned long long)loglik_scratch_bytes(g, npad));
        if (test_chunk) CHECK(g.chunk <= test_chunk, "test chunk not honoured");
        if (g.ntiles >= cus) CHECK(g.nseg_max == 1u, "n = %u K = %u cus = %u: segments though the tiles fill the device", n, K, cus);
        // every listed position is visited once per tile: by exactly one (chunk, segment)
        std::vector<uint8_t> seen(n_locs, 0);
        for (uint32_t off = 0; off < n_locs; off += g.chunk) {
          const uint32_t len = n_locs - off < g.chunk ? n_locs - off : g.chunk;
          const LoglikSegs s = loglik_segments(g, len);
          CHECK(s.nseg >= 1u && s.nseg <= g.nseg_max, "n = %u K = %u len = %u: %u segments", n, K, len, s.nseg);
          for (uint32_t seg = 0; seg < s.nseg; ++seg) {
            const uint32_t b = seg * s.seg_len, e = b + s.seg_len < len ? b + s.seg_len : len;
            CHECK(b < e, "n = %u K = %u len = %u: empty segment %u", n, K, len, seg);
            for (uint32_t i = b; i < e; ++i) ++seen[off + i];
          }
        }
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n_locs; ++i) bad += seen[i] != 1;
        CHECK(bad == 0, "n = %u K = %u cus = %u chunk = %u: %u positions not covered exactly once", n, K, cus, g.chunk, bad);
        // ... and every individual of the padded width belongs to one thread of one tile
        CHECK(npad % g.ipt == 0u, "a thread straddles the padded width");
      }
}

int main() {
  check_term();
  check_geometry(1, 1);
  check_geometry(513, 7);
  check_geometry(4096, 70000);
  // the benchmark shape: 512 tiles of 2048 fill the device, one segment, chunks of tens of thousands of locations
  const LoglikGeom g = loglik_geometry(1u << 20, 8, 256, 0);
  CHECK(g.ipt == 8 && g.ntiles == 512 && g.nseg_max == 1 && g.chunk >= 32768u, "N = 1M, K = 8: %u tiles, %u segments, chunk %u", g.ntiles,
        g.nseg_max, g.chunk);
  printf("train loglik: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
