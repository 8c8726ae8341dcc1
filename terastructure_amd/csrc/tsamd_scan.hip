// tsamd_snp_scan's kernels (tsamd_scan_kernels.h): every K-specialised instantiation and the run-time-K one, with and without
// a trait, in one translation unit of their own -- csrc/tsamd.hip sees only the launcher declared in tsamd_scan_plan.h.
#include <array>
#include <utility>

#include "tsamd_scan_kernels.h"

namespace tsamd {

namespace {
using ScanKernel = void (*)(const ScanArgs);
template <bool TRAIT, int... Ks>
constexpr void fill(ScanKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks] = ts_scan<Ks, TRAIT>), ...);
}
ScanKernel scan_kernel(uint32_t K, bool trait) {
  static_assert(TSAMD_SPECIALIZED_K == 32, "instantiations K = 1 .. TSAMD_SPECIALIZED_K");
  using Table = std::array<std::array<ScanKernel, TSAMD_SPECIALIZED_K + 1>, 2>;  // [trait][K], [.][0]: run-time K
  static const Table table = [] {
    Table t{};
    fill<false>(t[0].data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    fill<true>(t[1].data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    return t;
  }();
  return table[trait ? 1 : 0][K <= (uint32_t)TSAMD_SPECIALIZED_K ? K : 0u];
}
}  // namespace

void scan_launch_chunk(const ScanArgs &a, uint32_t nseg, double *out_sums, uint32_t *out_counts, hipStream_t stream) {
  const bool trait = a.trait != nullptr;
  hipLaunchKernelGGL(scan_kernel(a.K, trait), dim3(a.ntiles, nseg), dim3(kScanBlock), 0, stream, a);
  hipLaunchKernelGGL(ts_scan_finish, dim3((a.len * (uint32_t)kScanTraitValues + 255u) / 256u), dim3(256), 0, stream, a.part, a.len, a.ntiles,
                     scan_values(trait), out_sums, out_counts);
}

}  // namespace tsamd
