// Stand-alone check of csrc/tsamd_foldin_plan.h (no ROCm header, no GPU): the per-entry contribution and the change of
// tsamd_fold_in against long double, and the tile / segment geometry -- tiles x segments cover every (individual, listed
// position) exactly once and the partials stay under the stated bound.  Built and run by tests/test_fold_in_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tsamd_foldin_plan.h"

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

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // splitmix64 -> (0, 1)
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
}

static void check_entry() {
  // codes: 00 -> (0, 2), 10 -> (1, 1), 11 -> (2, 0) (code = 2 * high bit + low bit), 01 -> (0, 0)
  const double want_mom[4] = {0, 0, 1, 2}, want_dad[4] = {2, 0, 1, 0};
  for (uint32_t c = 0; c < 4; ++c) {
    double mom, dad;
    foldin_code_weights(c, mom, dad);
    CHECK(mom == want_mom[c] && dad == want_dad[c], "code %u -> (%g, %g)", c, mom, dad);
  }
  for (uint32_t K : {1u, 3u, 8u, 16u, 20u, 32u, 33u, 128u})
    for (int rep = 0; rep < 50; ++rep) {
      std::vector<double> w(K), eb(2 * K), acc(K), acc0(K);
      // w spans the scales exp(Elogtheta) takes (down to 1e-12 of the largest), eb lies in (0, 1)
      for (uint32_t k = 0; k < K; ++k) {
        w[k] = std::pow(10.0, -12.0 * uniform() * (rep % 3 == 0 ? 1.0 : 0.2));
        eb[2 * k] = uniform(), eb[2 * k + 1] = uniform();
        acc0[k] = rep % 2 ? 1000.0 * uniform() : 0.0;
      }
      for (uint32_t code = 0; code < 4; ++code) {
        acc = acc0;
        foldin_entry(w.data(), eb.data(), K, code, acc.data());
        long double s0 = 0, s1 = 0;
        for (uint32_t k = 0; k < K; ++k) s0 += (long double)w[k] * eb[2 * k], s1 += (long double)w[k] * eb[2 * k + 1];
        const long double y = code == 3 ? 2 : code == 2 ? 1 : 0, miss = code == 1;
        long double inv = 0;  // sum_k w_k * contribution_k = 2 for a stored entry: the invariant sum_k gamma' = k alpha + 2 M
        for (uint32_t k = 0; k < K; ++k) {
          const long double add = miss ? 0.0L : y * eb[2 * k] / s0 + (2 - y) * eb[2 * k + 1] / s1;
          const long double want = (long double)acc0[k] + add;
          // all terms are positive: K multiply-adds per sum ((K + 1) 2^-53 relative), the reciprocal, two products and two
          // additions -- (K + 8) 2^-53 of the result covers it
          const long double tol = (K + 8) * 1.2e-16L * fabsl(want);
          CHECK(fabsl((long double)acc[k] - want) <= tol, "K = %u code = %u k = %u: %.17g, exact %.17Lg", K, code, k, acc[k], want);
          if (miss) CHECK(acc[k] == acc0[k], "K = %u: a missing entry moved acc", K);
          inv += (long double)w[k] * ((long double)acc[k] - acc0[k]);
        }
        if (!miss && rep % 2 == 0) CHECK(fabsl(inv - 2.0L) <= (2 * K + 16) * 1.2e-16L * 2.0L, "K = %u code = %u: sum_k w_k d acc_k = %.17Lg", K, code, inv);
      }
    }
  // the update and the change
  for (int rep = 0; rep < 200; ++rep) {
    const uint32_t K = 1 + (uint32_t)(uniform() * 128) % 128;
    const double alpha = 1.0 / K;
    double sa = 0, sn = 0;
    long double lsa = 0, lsn = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const double w = uniform(), acc = 1e4 * uniform(), old = 1e4 * uniform();
      const double nw = foldin_gamma(alpha, w, acc);
      const long double lnw = (long double)alpha + (long double)w * acc;
      CHECK(fabsl((long double)nw - lnw) <= 1.2e-16L * fabsl(lnw), "gamma' = %.17g, exact %.17Lg", nw, lnw);
      sa += std::fabs(nw - old), sn += nw;
      lsa += fabsl(lnw - old), lsn += lnw;
    }
    const double ch = foldin_change(sa, sn);
    const long double want = (lsa / K) / (lsn / K);
    // |gamma' - gamma| carries the rounding of gamma' relative to max(gamma', gamma) <= 1e4 + 1: absolute 1.2e-12 per term
    CHECK(fabsl((long double)ch - want) <= (2 * K + 4) * 1.2e-16L * want + K * 1.2e-12L / lsn, "change = %.17g, exact %.17Lg (K = %u)", ch, want, K);
  }
  CHECK(foldin_change(0.0, 0.25) == 0.0, "an individual that does not move has change 0");
}

static void check_geometry(uint32_t npad, uint32_t n_locs) {
  for (uint32_t K : {1u, 3u, 8u, 16u, 20u, 32u, 33u, 128u})
    for (uint32_t cus : {1u, 2u, 64u, 256u, 304u})
      for (uint32_t test_segments : {0u, 1u, 7u, 1000u}) {
        const FoldinGeom g = foldin_geometry(npad, K, n_locs, cus, test_segments);
        CHECK(K > 32u ? g.ipt == 1u : 2u * g.ipt * K <= 64u, "K = %u: %u individuals per thread", K, g.ipt);
        CHECK(16u % g.ipt == 0u && npad % g.ipt == 0u, "K = %u: a thread's individuals do not share one 32-bit word", K);
        CHECK(g.tile_n == 256u * g.ipt && g.tile_n % 256u == 0u, "K = %u: tile of %u", K, g.tile_n);
        CHECK(g.batch == (K > 32u ? kFoldinWideBatch : kFoldinBatch), "K = %u: batch %u", K, g.batch);
        CHECK(g.nseg >= 1u && g.nseg <= kFoldinMaxSegments && g.seg_len >= 1u, "npad = %u K = %u: %u segments of %u", npad, K, g.nseg, g.seg_len);
        CHECK(foldin_scratch_bytes(g, npad, K) <= foldin_scratch_bound(npad, K), "npad = %u K = %u cus = %u: %llu bytes of partials", npad, K, cus,
              (unsigned long long)foldin_scratch_bytes(g, npad, K));
        CHECK(foldin_scratch_bound(npad, K) == kFoldinScratchBound || foldin_scratch_bound(npad, K) == (uint64_t)npad * K * 8u, "the bound");
        if (test_segments) CHECK(g.nseg <= test_segments, "test segments not honoured");
        if (test_segments == 1u) CHECK(g.nseg == 1u && g.seg_len == n_locs, "one segment");
        if (!test_segments && g.ntiles >= cus) CHECK(g.nseg == 1u, "npad = %u K = %u cus = %u: segments though the tiles fill the device", npad, K, cus);
        if (!test_segments && g.nseg > 1u) CHECK(g.seg_len % g.batch == 0u && g.seg_len >= kFoldinMinSegLen, "segment of %u", g.seg_len);
        // individuals: tile t owns [t tile_n, (t + 1) tile_n), thread by thread ipt consecutive ones -- every individual of the
        // padded width once (checked on the tile boundaries: the inside is contiguous by construction)
        CHECK((uint64_t)g.ntiles * g.tile_n >= npad && (uint64_t)(g.ntiles - 1u) * g.tile_n < npad, "npad = %u K = %u: %u tiles of %u", npad, K, g.ntiles,
              g.tile_n);
        // listed positions: by exactly one segment, none of them empty
        std::vector<uint8_t> seen(n_locs, 0);
        for (uint32_t seg = 0; seg < g.nseg; ++seg) {
          const uint64_t b = (uint64_t)seg * g.seg_len, e = b + g.seg_len < n_locs ? b + g.seg_len : n_locs;
          CHECK(b < e, "npad = %u K = %u n_locs = %u: empty segment %u", npad, K, n_locs, seg);
          for (uint64_t i = b; i < e; ++i) ++seen[i];
        }
        uint32_t bad = 0;
        for (uint32_t i = 0; i < n_locs; ++i) bad += seen[i] != 1;
        CHECK(bad == 0, "npad = %u K = %u cus = %u: %u positions not covered exactly once", npad, K, cus, bad);
      }
}

int main() {
  check_entry();
  for (uint32_t npad : {512u, 1024u, 4608u, 1u << 20})
    for (uint32_t n_locs : {1u, 33u, 4099u, 70000u}) check_geometry(npad, n_locs);
  // the benchmark shape: 1024 tiles of 1024 fill the device, one segment of 64 MB ...
  FoldinGeom g = foldin_geometry(1u << 20, 8, 2048, 256, 0);
  CHECK(g.ipt == 4 && g.ntiles == 1024 && g.nseg == 1, "N = 1M, K = 8: %u tiles, %u segments", g.ntiles, g.nseg);
  // ... and the projection shape: 8 tiles, the segments carry the grid
  g = foldin_geometry(8192, 8, 262144, 256, 0);
  CHECK(g.ntiles == 8 && g.nseg == 64 && g.seg_len == 4096, "N = 8192, K = 8, L = 262144: %u tiles, %u segments of %u", g.ntiles, g.nseg, g.seg_len);
  printf("fold in: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
