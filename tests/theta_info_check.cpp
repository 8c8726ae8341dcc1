// Stand-alone check of csrc/tsamd_info_plan.h (no ROCm header, no GPU): the packed index and its inverse for K = 1..128, the
// two per-entry terms of tsamd_theta_info against long double (code 01 and q at or beyond 0 and 1 included), the block / chunk /
// segment geometry (every listed individual in exactly one block, every listed location in exactly one k-step of one segment of
// one chunk, the scratch within its bounds, the test hooks honoured), and theta_se on a K = 2 case with a closed form, against a
// projected pseudo-inverse at K = 3, and on the rows that are not identified.  Built and run by tests/test_theta_info_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tsamd_info_plan.h"

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

static void check_index() {
  for (uint32_t k = 1; k <= 128u; ++k) {
    const uint32_t P = info_packed(k);
    CHECK(P == k * (k + 1u) / 2u && info_ppad(k) % kInfoTile == 0u && info_ppad(k) >= P && info_ppad(k) < P + kInfoTile, "K = %u: P = %u ppad = %u", k, P,
          info_ppad(k));
    uint32_t next = 0, bad = 0;
    for (uint32_t a = 0; a < k; ++a)
      for (uint32_t b = a; b < k; ++b) {
        const uint32_t p = info_index(a, b, k);
        bad += p != next++;                                        // row by row, no gap
        bad += p != a * k - (a ? a * (a - 1u) / 2u : 0u) + (b - a);  // the header's formula
        const InfoAB ab = info_unindex(p, k);
        bad += ab.a != a || ab.b != b;
        bad += info_index_sym(b, a, k) != p;
      }
    CHECK(next == P && bad == 0u, "K = %u: %u index error(s)", k, bad);
  }
  CHECK(info_packed(128) == 8256u && info_ppad(128) == 8256u && info_ppad(8) == 64u && info_ppad(11) == 128u, "P at K = 128, 8, 11");
}

static void check_terms() {
  std::vector<double> qs = {1e-300, 1e-150, 1e-17, 1e-9, 1e-6, 0.25, 0.5, 0.75, 1.0 - 1e-6, 1.0 - 1e-9, 1.0 - 1.2e-16};
  for (int i = 1; i < 1000; ++i) qs.push_back(i / 1000.0);
  const long double want_y[4] = {0, 0, 1, 2};  // codes 00, 01 (no term), 10, 11
  for (double q : qs)
    for (uint32_t code = 0; code < 4; ++code) {
      double co = -7, ce = -7;
      info_terms(q, code, &co, &ce);
      if (code == 1u) {
        CHECK(co == 0.0 && ce == 0.0, "q = %.17g: code 01 gives (%g, %g)", q, co, ce);
        continue;
      }
      // against long double on the fp64 1 - q the kernel forms (its rounding is d1, accounted for where q's own error is).  In
      // units of u = 2^-53: a square and a quotient round once each, the sum once more: 3 u per term; product, quotient: 2 u.
      const long double lq = q, lp = 1.0 - q, y = want_y[code];
      const long double lo = y / (lq * lq) + (2.0L - y) / (lp * lp), le = 2.0L / (lq * lp);
      if (std::isfinite((double)lo) && std::isfinite((double)le)) {
        CHECK(fabsl((long double)co - lo) <= 3.5e-16L * lo, "q = %.17g code = %u: c_obs = %.17g, exact %.17Lg", q, code, co, lo);
        CHECK(fabsl((long double)ce - le) <= 2.5e-16L * le, "q = %.17g code = %u: c_exp = %.17g, exact %.17Lg", q, code, ce, le);
      }
      // (where a term overflows -- q = 1e-300 with y > 0 -- the entry contributes nothing rather than an inf)
      CHECK(co >= 0.0 && ce >= 0.0 && std::isfinite(co) && std::isfinite(ce) && (q < 1e-100 || ce > 0.0), "q = %.17g code = %u: (%g, %g)", q, code, co, ce);
    }
  // q at or beyond 0 and 1 (by rounding): no term, never an inf or a NaN
  for (double q : {0.0, 1.0, 1.0 + 2.3e-16, -1e-18, -0.0, 2.0})
    for (uint32_t code = 0; code < 4; ++code) {
      double co = -7, ce = -7;
      info_terms(q, code, &co, &ce);
      CHECK(co == 0.0 && ce == 0.0, "q = %.17g code = %u: (%g, %g)", q, code, co, ce);
    }
  // the values: y = 1 at q = 0.5 gives 4 + 4 and 8; y = 0 at q = 0.25 gives 2 / 0.5625 and 2 / 0.1875
  double co, ce;
  info_terms(0.5, 2u, &co, &ce);
  CHECK(co == 8.0 && ce == 8.0, "q = 0.5, y = 1: (%g, %g)", co, ce);
  info_terms(0.25, 0u, &co, &ce);
  CHECK(co == 2.0 / 0.5625 && ce == 2.0 / 0.1875, "q = 0.25, y = 0: (%g, %g)", co, ce);
  info_terms(0.25, 3u, &co, &ce);
  CHECK(co == 32.0, "q = 0.25, y = 2: %g", co);
}

// the loop tsamd_theta_info runs, counted: blocks of individuals, chunks of locations, segments of k-steps, tiles per launch
static void check_geometry(uint32_t m, uint32_t k, uint32_t n_locs, uint32_t cus, uint32_t test_chunk, uint32_t test_block) {
  const InfoGeom g = info_geometry(m, k, n_locs, cus, test_chunk, test_block);
  uint32_t bad = 0;
  bad += !(g.k == k && g.p == info_packed(k) && g.ppad == info_ppad(k) && g.ptiles * kInfoTile == g.ppad);
  bad += !(g.block >= 4u && g.block % 4u == 0u && g.bpad == info_round_tile(g.block) && g.itiles * kInfoTile == g.bpad && g.block <= kInfoMaxBlockIndivs);
  if (test_block == 0u) bad += g.block % kInfoTile != 0u;  // whole tiles: every block starts where the columns are read as aligned dwords
  if (test_block > 0u) bad += g.block > info_round_step(test_block);
  bad += !(g.chunk >= 1u && g.chunk <= kInfoMaxChunk && g.chunk <= n_locs);
  if (test_chunk > 0u) bad += g.chunk > test_chunk;
  bad += !(g.tiles == g.itiles * g.ptiles && g.nseg_max >= 1u && g.nseg_max <= kInfoMaxSegments);
  bad += !(g.tiles_per_launch >= 1u && g.tiles_per_launch <= g.tiles);
  // the stated bounds on the scratch
  bad += info_coef_bytes(g) > kInfoScratchBound;
  bad += info_bb_bytes(g) > kInfoScratchBound;
  bad += info_part_bytes(g) > kInfoScratchBound;
  bad += info_acc_bytes(g) > kInfoScratchBound;
  bad += info_rows_bytes(g) > kInfoScratchBound;
  CHECK(bad == 0u, "m = %u K = %u L = %u cus = %u hooks (%u, %u): %u geometry error(s) (block %u chunk %u tiles %u nseg %u per launch %u)", m, k, n_locs, cus,
        test_chunk, test_block, bad, g.block, g.chunk, g.tiles, g.nseg_max, g.tiles_per_launch);
  // individuals: every one in exactly one block, blocks start on multiples of 4, a block's tiles all launched once
  uint64_t seen = 0;
  bad = 0;
  for (uint32_t i0 = 0; i0 < m; i0 += g.block) {
    const uint32_t blen = g.block < m - i0 ? g.block : m - i0, bpad = info_round_tile(blen), tiles = bpad / kInfoTile * g.ptiles;
    bad += i0 % 4u != 0u || bpad > g.bpad || tiles > g.tiles;
    uint32_t launched = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += g.tiles_per_launch) launched += g.tiles_per_launch < tiles - t0 ? g.tiles_per_launch : tiles - t0;
    bad += launched != tiles;
    seen += blen;
  }
  CHECK(bad == 0u && seen == m, "m = %u K = %u: blocks cover %llu individuals, %u error(s)", m, k, (unsigned long long)seen, bad);
  // locations: every one in exactly one k-step of one segment of one chunk
  uint64_t covered = 0;
  bad = 0;
  for (uint32_t off = 0; off < n_locs; off += g.chunk) {
    const uint32_t len = g.chunk < n_locs - off ? g.chunk : n_locs - off, len4 = info_round_step(len);
    const KinSegs s = info_segments(g, len);
    bad += !(s.steps * kInfoStep == len4 && s.nseg >= 1u && s.nseg <= g.nseg_max && (uint64_t)s.nseg * s.seg_steps >= s.steps);
    bad += !((uint64_t)(s.nseg - 1u) * s.seg_steps < s.steps);  // none of them empty
    bad += (uint64_t)len4 * g.bpad * 2u * sizeof(double) > info_coef_bytes(g) || (uint64_t)len4 * g.ppad * sizeof(double) > info_bb_bytes(g);
    uint32_t steps = 0;
    for (uint32_t sgi = 0; sgi < s.nseg; ++sgi) {
      const uint32_t b = sgi * s.seg_steps, e = s.steps < b + s.seg_steps ? s.steps : b + s.seg_steps;
      steps += e - b;
    }
    bad += steps != s.steps;
    covered += len;
  }
  CHECK(bad == 0u && covered == n_locs, "m = %u K = %u L = %u: chunks cover %llu locations, %u error(s)", m, k, n_locs, (unsigned long long)covered, bad);
}

static void check_se() {
  // K = 2, closed form: se_0 = se_1 = 1 / sqrt(H_00 - 2 H_01 + H_11), cov = [[v, -v], [-v, v]]
  {
    const double H[3] = {7.0, 2.0, 5.0};  // H_00, H_01, H_11
    double se[2], cov[3];
    uint8_t st = 9;
    theta_se(H, 1, 2, se, cov, &st);
    const double v = 1.0 / (7.0 - 4.0 + 5.0);
    CHECK(st == 0u && fabs(se[0] - sqrt(v)) <= 1e-16 && se[0] == se[1], "K = 2: se = (%.17g, %.17g), want %.17g", se[0], se[1], sqrt(v));
    CHECK(fabs(cov[0] - v) <= 1e-16 && fabs(cov[1] + v) <= 1e-16 && fabs(cov[2] - v) <= 1e-16, "K = 2: cov = (%g, %g, %g)", cov[0], cov[1], cov[2]);
    theta_se(H, 1, 2, se, nullptr, nullptr);  // cov and status may be NULL
    CHECK(fabs(se[0] - sqrt(v)) <= 1e-16, "K = 2 without cov");
  }
  // K = 1: nothing to estimate
  {
    const double H[1] = {3.0};
    double se[1] = {5.0}, cov[1] = {5.0};
    uint8_t st = 9;
    theta_se(H, 1, 1, se, cov, &st);
    CHECK(st == 0u && se[0] == 0.0 && cov[0] == 0.0, "K = 1: (%g, %g, %u)", se[0], cov[0], st);
  }
  // K = 3 from two rows of outer products b b^T with weights: cov rows sum to zero, cov (Z^T H Z) cov-block = identity
  {
    const uint32_t k = 3;
    const double bs[5][3] = {{0.1, 0.5, 0.9}, {0.8, 0.3, 0.2}, {0.4, 0.4, 0.7}, {0.05, 0.95, 0.5}, {0.6, 0.1, 0.3}};
    const double w[5] = {3.0, 8.0, 5.0, 11.0, 4.0};
    double H[6] = {0};
    for (int j = 0; j < 5; ++j)
      for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = a; b < k; ++b) H[info_index(a, b, k)] += w[j] * bs[j][a] * bs[j][b];
    double se[3], cov[6];
    uint8_t st = 9;
    theta_se(H, 1, k, se, cov, &st);
    CHECK(st == 0u, "K = 3: status %u", st);
    auto h = [&](uint32_t a, uint32_t b) { return H[info_index_sym(a, b, k)]; };
    auto c = [&](uint32_t a, uint32_t b) { return cov[info_index_sym(a, b, k)]; };
    for (uint32_t a = 0; a < k; ++a) {
      CHECK(fabs(c(a, 0) + c(a, 1) + c(a, 2)) <= 1e-15 * fabs(c(a, a)), "K = 3: row %u of cov sums to %g", a, c(a, 0) + c(a, 1) + c(a, 2));
      CHECK(se[a] == sqrt(c(a, a)) && se[a] > 0.0, "K = 3: se[%u] = %g", a, se[a]);
    }
    for (uint32_t a = 0; a < 2; ++a)
      for (uint32_t b = 0; b < 2; ++b) {
        double s = 0.0;  // (M cov-block)_ab
        for (uint32_t t = 0; t < 2; ++t) s += (h(a, t) - h(a, 2) - h(2, t) + h(2, 2)) * c(t, b);
        CHECK(fabs(s - (a == b ? 1.0 : 0.0)) <= 1e-13, "K = 3: (M cov)[%u][%u] = %.17g", a, b, s);
      }
  }
  // not identified: an all-zero row; one locus at K = 3 (fewer stored loci than K - 1); duplicated populations; a NaN
  {
    const uint32_t k = 3;
    double H[4][6] = {{0}};
    const double b1[3] = {0.2, 0.7, 0.4};
    for (uint32_t a = 0; a < k; ++a)
      for (uint32_t b = a; b < k; ++b) H[1][info_index(a, b, k)] = 9.0 * b1[a] * b1[b];
    const double bd[4][3] = {{0.3, 0.3, 0.8}, {0.6, 0.6, 0.1}, {0.2, 0.2, 0.5}, {0.9, 0.9, 0.4}};  // populations 0 and 1 alike
    for (int j = 0; j < 4; ++j)
      for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = a; b < k; ++b) H[2][info_index(a, b, k)] += (2.0 + j) * bd[j][a] * bd[j][b];
    for (uint32_t p = 0; p < 6; ++p) H[3][p] = NAN;
    double se[4][3], cov[4][6];
    uint8_t st[4] = {9, 9, 9, 9};
    theta_se(&H[0][0], 4, k, &se[0][0], &cov[0][0], st);
    for (int i = 0; i < 4; ++i) {
      bool all_nan = true;
      for (uint32_t a = 0; a < k; ++a) all_nan = all_nan && std::isnan(se[i][a]);
      for (uint32_t p = 0; p < 6; ++p) all_nan = all_nan && std::isnan(cov[i][p]);
      CHECK(st[i] == 1u && all_nan, "row %d must not be identified: status %u se = (%g, %g, %g)", i, st[i], se[i][0], se[i][1], se[i][2]);
    }
  }
  // K = 128, a diagonally dominant H: runs inside its work space (the sanitizers watch), identified, rows of cov sum to ~0
  {
    const uint32_t k = 128, P = info_packed(k);
    std::vector<double> H(2u * P), se(2u * k), cov(2u * P);
    for (uint32_t i = 0; i < 2u; ++i)
      for (uint32_t a = 0; a < k; ++a)
        for (uint32_t b = a; b < k; ++b) H[(size_t)i * P + info_index(a, b, k)] = a == b ? 300.0 + a + i : 1.0 + 0.001 * ((a * 7u + b * 13u) % 17u);
    uint8_t st[2] = {9, 9};
    theta_se(H.data(), 2, k, se.data(), cov.data(), st);
    double worst = 0.0;
    for (uint32_t a = 0; a < k; ++a) {
      double s = 0.0;
      for (uint32_t b = 0; b < k; ++b) s += cov[info_index_sym(a, b, k)];
      worst = fmax(worst, fabs(s) / cov[info_index(a, a, k)]);
    }
    CHECK(st[0] == 0u && st[1] == 0u && worst <= 1e-12 && se[0] > 0.0 && se[2u * k - 1u] > 0.0, "K = 128: status (%u, %u), row sums %g", st[0], st[1], worst);
  }
}

int main() {
  check_index();
  check_terms();
  const uint32_t ms[] = {1u, 2u, 63u, 64u, 65u, 130u, 200u, 1000u, 8191u, 8192u, 8193u, 65536u, 100003u, 1u << 20};
  const uint32_t ks[] = {1u, 2u, 3u, 8u, 10u, 11u, 16u, 32u, 33u, 64u, 127u, 128u};
  for (uint32_t m : ms)
    for (uint32_t k : ks)
      for (uint32_t cus : {1u, 4u, 256u, 5000u}) {
        check_geometry(m, k, 70000u, cus, 0u, 0u);
        check_geometry(m, k, 37u, cus, 0u, 0u);
        check_geometry(m, k, 1u, cus, 8u, 64u);
        check_geometry(m, k, 130u, cus, 8u, 64u);
        check_geometry(m, k, 4099u, cus, 1000u, 20u);
        check_geometry(m, k, 3u, cus, 1u, 1u);
      }
  for (uint32_t k = 1; k <= 128u; ++k) check_geometry(12345u, k, 65536u, 256u, 0u, 0u), check_geometry(777u, k, 100u, 4u, 8u, 64u);
  // what the documents state: 8192 individuals at small K, 1984 at K = 128; chunks of 2048 at a full block
  const InfoGeom g8 = info_geometry(8192, 8, 65536, 256, 0, 0), g128 = info_geometry(1u << 20, 128, 65536, 256, 0, 0);
  CHECK(g8.block == 8192u && g8.chunk == 2048u && g8.tiles == 128u && g8.nseg_max == 4u, "K = 8: block %u chunk %u tiles %u nseg %u", g8.block, g8.chunk,
        g8.tiles, g8.nseg_max);
  CHECK(g128.block == 1984u && g128.ptiles == 129u && g128.nseg_max == 1u, "K = 128: block %u ptiles %u nseg %u", g128.block, g128.ptiles, g128.nseg_max);
  check_se();
  printf("theta_info: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
