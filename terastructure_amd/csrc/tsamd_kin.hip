// tsamd_kinship's kernels (tsamd_kin_kernels.h): every K-specialised instantiation of ts_kin_resid, its run-time-K form and the
// K-independent matrix-product kernels in one translation unit of their own -- csrc/tsamd.hip sees only the launchers
// declared in tsamd_kin_plan.h.
#include <array>
#include <utility>

#include "tsamd_kin_kernels.h"

namespace tsamd {

namespace {
using KinResidKernel = void (*)(const KinArgs);
template <int... Ks>
constexpr void fill(KinResidKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks] = ts_kin_resid<Ks>), ...);
}
KinResidKernel kin_resid_kernel(uint32_t K) {
  static_assert(TSAMD_SPECIALIZED_K == 32, "instantiations K = 1 .. TSAMD_SPECIALIZED_K");
  static const std::array<KinResidKernel, TSAMD_SPECIALIZED_K + 1> table = [] {  // [0]: run-time K
    std::array<KinResidKernel, TSAMD_SPECIALIZED_K + 1> t{};
    fill(t.data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    return t;
  }();
  return table[K <= (uint32_t)TSAMD_SPECIALIZED_K ? K : 0u];
}
}  // namespace

void kin_launch_resid(const KinArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(kin_resid_kernel(a.K), dim3((a.mpad + kKinBlock - 1u) / kKinBlock, (a.len4 + kKinResidBatch - 1u) / kKinResidBatch),
                     dim3(kKinBlock), 0, stream, a);
}

void kin_launch_pairs(const KinArgs &a, uint32_t pair0, uint32_t npairs, const KinSegs &sg, hipStream_t stream) {
  hipLaunchKernelGGL(ts_kin_syrk, dim3(npairs, sg.nseg), dim3(kKinBlock), 0, stream, a.r, a.s, a.mpad, a.ntiles, pair0, sg.steps,
                     sg.seg_steps, a.part);
  hipLaunchKernelGGL(ts_kin_finish, dim3(npairs), dim3(kKinBlock), 0, stream, a.part, sg.nseg, a.mpad, a.ntiles, pair0, a.num, a.den);
}

void kin_launch_mirror(double *num, double *den, uint32_t mpad, hipStream_t stream) {
  hipLaunchKernelGGL(ts_kin_mirror, dim3((mpad + kKinBlock - 1u) / kKinBlock, mpad, 2), dim3(kKinBlock), 0, stream, num, den, mpad);
}

void kin_launch_form(double *num, const double *den, uint32_t mpad, hipStream_t stream) {
  const size_t count = (size_t)mpad * mpad;
  hipLaunchKernelGGL(ts_kin_form, dim3((uint32_t)((count + kKinBlock - 1u) / kKinBlock)), dim3(kKinBlock), 0, stream, num, den, count);
}

}  // namespace tsamd
