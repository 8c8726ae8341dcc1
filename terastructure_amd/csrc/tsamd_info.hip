// tsamd_theta_info's kernels (tsamd_info_kernels.h): every K-specialised instantiation of ts_info_coef, its run-time-K form and
// the K-independent product kernels in one translation unit of their own -- csrc/tsamd.hip sees only the launchers declared in
// tsamd_info_plan.h.
#include <array>
#include <utility>

#include "tsamd_info_kernels.h"

namespace tsamd {

namespace {
using InfoCoefKernel = void (*)(const InfoArgs);
template <int... Ks>
constexpr void fill(InfoCoefKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks] = ts_info_coef<Ks>), ...);
}
InfoCoefKernel info_coef_kernel(uint32_t K) {
  static_assert(TSAMD_SPECIALIZED_K == 32, "instantiations K = 1 .. TSAMD_SPECIALIZED_K");
  static const std::array<InfoCoefKernel, TSAMD_SPECIALIZED_K + 1> table = [] {  // [0]: run-time K
    std::array<InfoCoefKernel, TSAMD_SPECIALIZED_K + 1> t{};
    fill(t.data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    return t;
  }();
  return table[K <= (uint32_t)TSAMD_SPECIALIZED_K ? K : 0u];
}
}  // namespace

void info_launch_coef(const InfoArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(info_coef_kernel(a.K), dim3((a.bpad + kInfoCoefIndivs - 1u) / kInfoCoefIndivs, (a.len4 + kInfoCoefBatch - 1u) / kInfoCoefBatch),
                     dim3(kInfoBlock), 0, stream, a);
  hipLaunchKernelGGL(ts_info_outer, dim3((a.ppad + kInfoBlock - 1u) / kInfoBlock, a.len4), dim3(kInfoBlock), 0, stream, a);
}

void info_launch_tiles(const InfoArgs &a, uint32_t tile0, uint32_t ntiles, const KinSegs &sg, hipStream_t stream) {
  hipLaunchKernelGGL(ts_info_gemm, dim3(ntiles, sg.nseg), dim3(kInfoBlock), 0, stream, a.cobs, a.cexp, a.bb, a.bpad, a.ppad, a.ptiles, tile0, sg.steps,
                     sg.seg_steps, a.part);
  hipLaunchKernelGGL(ts_info_finish, dim3(ntiles), dim3(kInfoBlock), 0, stream, a.part, sg.nseg, tile0, a.acc);
}

void info_launch_rows(const InfoArgs &a, double *obs, double *exp, hipStream_t stream) {
  hipLaunchKernelGGL(ts_info_rows, dim3((a.P + kInfoBlock - 1u) / kInfoBlock, a.blen), dim3(kInfoBlock), 0, stream, a.acc, a.P, a.ptiles, obs, exp);
}

}  // namespace tsamd
