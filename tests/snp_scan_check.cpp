// Stand-alone check of csrc/tsamd_scan_plan.h (no ROCm header, no GPU): the per-entry terms of tsamd_snp_scan against long
// double, the statistics formulas of tsamd_scan_statistics against long double, and the tile / segment / chunk geometry --
// every listed position is covered by exactly one (chunk, segment) and the partial-sum buffer stays under the stated bound.
// Built and run by tests/test_snp_scan_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "tsamd_scan_plan.h"

using namespace tsamd;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
    }                                             \
  } while (0)

static const long double kEps = 1.2e-16L;  // 2^-53 rounded up

static bool near(double got, long double want, long double scale, int roundings) {
  return fabsl((long double)got - want) <= roundings * kEps * scale;
}

static void check_terms() {
  std::vector<double> qs;
  for (int i = 0; i <= 1000; ++i) qs.push_back(i / 1000.0);
  for (int e = -20; e <= -1; ++e) qs.push_back(std::pow(10.0, e)), qs.push_back(1.0 - std::pow(10.0, e));
  const double ts[] = {0.0, 1.0, -1.0, 0.37, -2.5, 1e3, -1e-3, 123456.789};
  for (double q : qs)
    for (uint32_t c = 0; c < 4; ++c)
      for (double t : ts)
        for (int phen = 0; phen < 2; ++phen) {
          const double tz = phen ? t : 0.0, pm = phen ? 1.0 : 0.0;  // (the kernel passes 0 in place of a NaN trait value)
          double v[kScanTraitValues], f[kScanFitValues];
          for (double &x : v) x = 0.0;
          for (double &x : f) x = 0.0;
          scan_add_entry<true>(q, c, tz, pm, v);
          scan_add_entry<false>(q, c, tz, pm, f);
          for (int x = 0; x < kScanFitValues; ++x) CHECK(v[x] == f[x], "q = %.17g code %u: value %d differs with and without a trait", q, c, x);
          if (c == 1u) {  // missing, held out, padding: exact zeros everywhere
            for (int x = 0; x < kScanTraitValues; ++x) CHECK(v[x] == 0.0, "q = %.17g code 01: value %d = %.17g", q, x, v[x]);
            continue;
          }
          const uint32_t y = c == 0u ? 0u : c == 2u ? 1u : 2u;
          const long double Q = q, R = 1.0L - Q, H = 2.0L * Q * R, T = tz, RES = (long double)y - 2.0L * Q;
          // every value is a short product of quantities in [0, 2] (times |t|, |t|^2): a few roundings of the largest factor
          CHECK(near(v[kScanE0], R * R, 1.0L, 3), "E0(q = %.17g) = %.17g", q, v[kScanE0]);
          CHECK(near(v[kScanE1], H, 1.0L, 3), "E1(q = %.17g) = %.17g", q, v[kScanE1]);
          CHECK(near(v[kScanE2], Q * Q, 1.0L, 2), "E2(q = %.17g) = %.17g", q, v[kScanE2]);
          CHECK(near(v[kScanVH], H * (1.0L - H), 1.0L, 6), "VH(q = %.17g) = %.17g", q, v[kScanVH]);
          CHECK(v[kScanE0] >= 0.0 && v[kScanE1] >= 0.0 && v[kScanE2] >= 0.0 && v[kScanVH] >= 0.0, "q = %.17g: a negative fit term", q);
          CHECK(v[kScanO0] == (y == 0u) && v[kScanO1] == (y == 1u) && v[kScanO2] == (y == 2u), "q = %.17g code %u: classes %g %g %g", q, c,
                v[kScanO0], v[kScanO1], v[kScanO2]);
          const long double at = fabsl(T), P = pm;
          CHECK(v[kScanT] == tz, "sum t: %.17g for t = %.17g", v[kScanT], tz);
          CHECK(near(v[kScanTR], T * RES, 2.0L * at, 3), "t r (q = %.17g, y = %u, t = %g) = %.17g", q, y, tz, v[kScanTR]);
          CHECK(near(v[kScanTTH], T * T * H, at * at, 5), "t^2 h (q = %.17g, t = %g) = %.17g", q, tz, v[kScanTTH]);
          CHECK(near(v[kScanTH], T * H, at, 4), "t h (q = %.17g, t = %g) = %.17g", q, tz, v[kScanTH]);
          CHECK(near(v[kScanR], P * RES, 2.0L, 2), "r (q = %.17g, y = %u) = %.17g", q, y, v[kScanR]);
          CHECK(near(v[kScanH], P * H, 1.0L, 3), "h (q = %.17g) = %.17g", q, v[kScanH]);
          CHECK(v[kScanNT] == pm, "phenotyped count %.17g", v[kScanNT]);
          CHECK(v[kScanTTH] >= 0.0, "t^2 h negative");
        }
  // codes: 00 -> 0, 10 -> 1, 11 -> 2 (code = 2 * high bit + low bit), 01 has no term
  CHECK(scan_code_ok(0) == 1u && scan_code_y(0) == 0u, "code 00");
  CHECK(scan_code_ok(1) == 0u, "code 01");
  CHECK(scan_code_ok(2) == 1u && scan_code_y(2) == 1u, "code 10");
  CHECK(scan_code_ok(3) == 1u && scan_code_y(3) == 2u, "code 11");
  // the sums of many entries: counts stay exact integers
  double v[kScanTraitValues] = {0};
  for (uint32_t i = 0; i < 100000u; ++i) scan_add_entry<true>((i % 997u) / 997.0, i & 3u, 0.5, (double)(i % 3u != 0u), v);
  CHECK(v[kScanO0] == 25000.0 && v[kScanO1] == 25000.0 && v[kScanO2] == 25000.0, "class counts %g %g %g", v[kScanO0], v[kScanO1], v[kScanO2]);
  CHECK(v[kScanNT] == std::floor(v[kScanNT]) && v[kScanNT] > 0.0 && v[kScanNT] < 75000.0, "phenotyped count %g", v[kScanNT]);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // xorshift64*: [0, 1)
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

static void check_statistics() {
  const long double sqrt2 = sqrtl(2.0L);
  for (int rep = 0; rep < 20000; ++rep) {
    const double n = 10.0 + std::floor(uniform() * 5000.0);
    double fit[4] = {n * uniform(), n * 0.5 * uniform() + 1e-3, n * uniform(), n * 0.25 * uniform() + 1e-3};
    uint32_t cnt[3] = {(uint32_t)(n * uniform()), (uint32_t)(n * uniform() * 0.5), (uint32_t)(n * uniform() * 0.3)};
    const double c = 4.0 * uniform() - 2.0;
    uint32_t nt = 2u + (uint32_t)(uniform() * n);
    // sums of a trait with mean c among nt individuals, h about 0.3: V = sum (t - c)^2 h is well away from 0
    double tr[6] = {c * nt, (uniform() - 0.5) * std::sqrt((double)nt), (1.0 + c * c) * 0.3 * nt, c * 0.3 * nt, (uniform() - 0.5) * std::sqrt((double)nt),
                    0.3 * nt};
    double st[6];
    scan_statistics_row(fit, cnt, tr, nt, st);
    const long double o1 = cnt[1], o2 = cnt[2];
    const long double zh = (o1 - fit[1]) / sqrtl((long double)fit[3]);
    const long double zf = ((o1 + 2.0L * o2) - ((long double)fit[1] + 2.0L * fit[2])) / sqrtl((long double)fit[1]);
    const long double C = (long double)tr[0] / nt, U = tr[1] - C * tr[4], V = tr[2] - 2.0L * C * tr[3] + C * C * tr[5];
    const long double zt = U / sqrtl(V);
    // a quotient of a difference: the difference carries an ulp of its larger operand, the root and the division one each
    const long double th = 4.0L * kEps * (fabsl(zh) + (o1 + fit[1]) / sqrtl((long double)fit[3]));
    const long double tf = 6.0L * kEps * (fabsl(zf) + (o1 + 2.0L * o2 + fit[1] + 2.0L * fit[2]) / sqrtl((long double)fit[1]));
    const long double vmag = fabsl((long double)tr[2]) + 2.0L * fabsl(C * tr[3]) + C * C * tr[5];
    const long double tt = 8.0L * kEps * ((fabsl((long double)tr[1]) + fabsl(C * tr[4])) / sqrtl(V) + fabsl(zt) * (1.0L + vmag / V));
    CHECK(fabsl(st[0] - zh) <= th, "z_het %.17g, exact %.17Lg", st[0], zh);
    CHECK(fabsl(st[2] - zf) <= tf, "z_freq %.17g, exact %.17Lg", st[2], zf);
    CHECK(fabsl(st[4] - zt) <= tt, "z_trait %.17g, exact %.17Lg", st[4], zt);
    for (int x = 0; x < 3; ++x) {
      const long double p = erfcl(fabsl((long double)st[2 * x]) / sqrt2);  // (of the z the function returned: erfc alone)
      CHECK(fabsl(st[2 * x + 1] - p) <= 16.0L * kEps * p * (1.0L + st[2 * x] * st[2 * x]) + 1e-300L, "p(%.17g) = %.17g, exact %.17Lg", st[2 * x],
            st[2 * x + 1], p);
      CHECK(st[2 * x + 1] >= 0.0 && st[2 * x + 1] <= 1.0, "p out of [0, 1]");
    }
  }
  // the degenerate rows: z = 0, p = 1
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double fit[4] = {10.0, 5.0, 3.0, 2.0}, tr[6] = {4.0, 1.0, 9.0, 2.0, 0.5, 3.0}, st[6];
  uint32_t cnt[3] = {7, 6, 2};
  auto null_at = [&](int x) { return st[2 * x] == 0.0 && st[2 * x + 1] == 1.0; };
  scan_statistics_row(fit, cnt, tr, 8u, st);
  CHECK(!null_at(0) && !null_at(1) && !null_at(2), "a regular row came out null");
  scan_statistics_row(fit, cnt, nullptr, 8u, st);
  CHECK(!null_at(0) && !null_at(1) && null_at(2), "no trait sums");
  for (uint32_t n : {0u, 1u}) {
    scan_statistics_row(fit, cnt, tr, n, st);
    CHECK(null_at(2), "count %u", n);
  }
  for (double bad : {0.0, -1.0, nan}) {
    double f2[4] = {10.0, 5.0, 3.0, bad};
    scan_statistics_row(f2, cnt, tr, 8u, st);
    CHECK(null_at(0) && !null_at(1), "VH = %g", bad);
    double f3[4] = {10.0, bad, 3.0, 2.0};
    scan_statistics_row(f3, cnt, tr, 8u, st);
    CHECK(null_at(1), "E1 = %g", bad);
  }
  double t0[6] = {4.0, 1.0, 0.5, 2.0, 0.5, 3.0};  // V = 0.5 - 2 * 0.5 * 2 + 0.25 * 3 < 0
  scan_statistics_row(fit, cnt, t0, 8u, st);
  CHECK(null_at(2), "V < 0");
  double t1[6] = {0.0, 1.0, 0.0, 0.0, 0.5, 3.0};  // V = 0
  scan_statistics_row(fit, cnt, t1, 8u, st);
  CHECK(null_at(2), "V = 0");
}

static void check_geometry(uint32_t npad, uint32_t n_locs) {
  for (uint32_t K : {1u, 2u, 4u, 5u, 8u, 9u, 16u, 17u, 20u, 32u, 33u, 64u, 128u})
    for (int trait = 0; trait < 2; ++trait)
      for (uint32_t cus : {1u, 2u, 4u, 256u, 304u})
        for (uint32_t test_chunk : {0u, 1u, 5u}) {
          const ScanGeom g = scan_geometry(npad, K, trait != 0, cus, test_chunk);
          CHECK(g.ipt * K <= 64u || K > 32u, "K = %u: %u individuals per thread", K, g.ipt);
          CHECK(g.ipt == 1u || 16u % g.ipt == 0u, "K = %u: a thread's individuals do not share one 32-bit word", K);
          CHECK(g.ipt == scan_ipt(K <= 32u ? K : 0u, trait != 0), "K = %u: the run-time-K kernel takes one individual per thread", K);
          CHECK(g.tile_n == 256u * g.ipt && (uint64_t)g.ntiles * g.tile_n >= npad && (uint64_t)(g.ntiles - 1u) * g.tile_n < npad,
                "npad = %u K = %u: %u tiles of %u", npad, K, g.ntiles, g.tile_n);
          CHECK(g.values == (trait ? 14u : 7u), "values %u", g.values);
          CHECK(g.chunk >= 1u && g.chunk <= kScanMaxChunk && g.nseg_max >= 1u && g.nseg_max <= kScanMaxSegments, "npad = %u K = %u", npad, K);
          CHECK(scan_scratch_bytes(g) <= kScanScratchBound, "npad = %u K = %u: %llu bytes of partials", npad, K,
                (unsigned long long)scan_scratch_bytes(g));
          if (test_chunk) CHECK(g.chunk <= test_chunk, "test chunk not honoured");
          if (g.ntiles >= cus) CHECK(g.nseg_max == 1u, "npad = %u K = %u cus = %u: segments though the tiles fill the device", npad, K, cus);
          CHECK(npad % g.ipt == 0u, "a thread straddles the padded width");
          // every listed position is visited once per tile: by exactly one (chunk, segment)
          std::vector<uint8_t> seen(n_locs, 0);
          for (uint32_t off = 0; off < n_locs; off += g.chunk) {
            const uint32_t len = n_locs - off < g.chunk ? n_locs - off : g.chunk;
            const ScanSegs s = scan_segments(g, len);
            CHECK(s.nseg >= 1u && s.nseg <= g.nseg_max, "npad = %u K = %u len = %u: %u segments", npad, K, len, s.nseg);
            for (uint32_t seg = 0; seg < s.nseg; ++seg) {
              const uint32_t b = seg * s.seg_len, e = b + s.seg_len < len ? b + s.seg_len : len;
              CHECK(b < e, "npad = %u K = %u len = %u: empty segment %u", npad, K, len, seg);
              for (uint32_t i = b; i < e; ++i) ++seen[off + i];
            }
          }
          uint32_t bad = 0;
          for (uint32_t i = 0; i < n_locs; ++i) bad += seen[i] != 1;
          CHECK(bad == 0, "npad = %u K = %u cus = %u chunk = %u: %u positions not covered exactly once", npad, K, cus, g.chunk, bad);
        }
}

int main() {
  check_terms();
  check_statistics();
  check_geometry(512, 1);
  check_geometry(1024, 7);
  check_geometry(4608, 70000);
  check_geometry(1u << 20, 2048);
  check_geometry(11u << 20, 300);  // 11M individuals: the largest shard the bound is stated for
  // the benchmark shape: 512 tiles of 2048 fill the device, one segment
  const ScanGeom g = scan_geometry(1u << 20, 8, true, 256, 0);
  CHECK(g.ipt == 8 && g.ntiles == 512 && g.nseg_max == 1 && g.chunk >= 2048u, "N = 1M, K = 8: %u tiles, %u segments, chunk %u", g.ntiles, g.nseg_max,
        g.chunk);
  printf("snp scan: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
