// tsamd_fold_in's kernels (tsamd_foldin_kernels.h): every K-specialised sweep, the run-time-K one and the step in one
// translation unit of their own -- csrc/tsamd.hip sees only the launchers declared in tsamd_foldin_plan.h.
#include <array>
#include <utility>

#include "tsamd_foldin_kernels.h"

namespace tsamd {

namespace {
using FoldinKernel = void (*)(const FoldinArgs);
template <int... Ks>
constexpr void fill(FoldinKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks + 1] = ts_foldin_sweep<Ks + 1>), ...);
}
FoldinKernel foldin_kernel(uint32_t K) {
  static const std::array<FoldinKernel, kFoldinSpecializedK + 1> table = [] {  // [0]: run-time K
    std::array<FoldinKernel, kFoldinSpecializedK + 1> t{};
    t[0] = ts_foldin_sweep_wide;
    fill(t.data(), std::make_integer_sequence<int, (int)kFoldinSpecializedK>{});
    return t;
  }();
  return table[K <= kFoldinSpecializedK ? K : 0u];
}
}  // namespace

void foldin_launch_init(const FoldinArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(ts_foldin_init, dim3((a.npad + 255u) / 256u), dim3(256), 0, stream, a);
}

void foldin_launch_update(const FoldinArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(foldin_kernel(a.K), dim3(a.ntiles, a.nseg), dim3(kFoldinBlock), 0, stream, a);
  (void)hipMemsetAsync(a.active, 0, (size_t)(1u + a.ntiles) * sizeof(uint32_t), stream);  // (a failure shows in hipGetLastError)
  hipLaunchKernelGGL(ts_foldin_step, dim3((a.npad + 255u) / 256u), dim3(256), 0, stream, a);
}

}  // namespace tsamd
