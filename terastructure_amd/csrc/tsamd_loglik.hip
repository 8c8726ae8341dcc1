// tsamd_train_loglik's kernels (tsamd_loglik_kernels.h): every K-specialised instantiation and the run-time-K one in one
// translation unit of their own -- csrc/tsamd.hip sees only the launchers declared in tsamd_loglik_plan.h.
#include <array>
#include <utility>

#include "tsamd_loglik_kernels.h"

namespace tsamd {

namespace {
using LoglikKernel = void (*)(const LoglikArgs);
template <int... Ks>
constexpr void fill(LoglikKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks] = ts_loglik<Ks>), ...);
}
LoglikKernel loglik_kernel(uint32_t K) {
  static_assert(TSAMD_SPECIALIZED_K == 32, "instantiations K = 1 .. TSAMD_SPECIALIZED_K");
  static const std::array<LoglikKernel, TSAMD_SPECIALIZED_K + 1> table = [] {  // [0]: run-time K
    std::array<LoglikKernel, TSAMD_SPECIALIZED_K + 1> t{};
    fill(t.data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    return t;
  }();
  return table[K <= (uint32_t)TSAMD_SPECIALIZED_K ? K : 0u];
}
}  // namespace

void loglik_launch_chunk(const LoglikArgs &a, uint32_t nseg, double *out_sum, uint32_t *out_cnt, double *acc_sum, uint32_t *acc_cnt,
                         hipStream_t stream) {
  hipLaunchKernelGGL(loglik_kernel(a.K), dim3(a.ntiles, nseg), dim3(kLoglikBlock), 0, stream, a);
  hipLaunchKernelGGL(ts_loglik_finish_loc, dim3((a.len + 255u) / 256u), dim3(256), 0, stream, a.part_loc_sum, a.part_loc_cnt, a.len,
                     a.ntiles, out_sum, out_cnt);
  hipLaunchKernelGGL(ts_loglik_finish_indiv, dim3((a.npad + 255u) / 256u), dim3(256), 0, stream, a.part_ind_sum, a.part_ind_cnt, nseg,
                     a.npad, acc_sum, acc_cnt);
}

void loglik_launch_theta(const double *gam, uint32_t npad, uint32_t K, double *thn, hipStream_t stream) {
  hipLaunchKernelGGL(ts_loglik_theta, dim3((npad + 255u) / 256u), dim3(256), 0, stream, gam, npad, K, thn);
}

}  // namespace tsamd
