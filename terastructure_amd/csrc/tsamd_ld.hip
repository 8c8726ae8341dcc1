// tsamd_ld's kernels (tsamd_ld_kernels.h): every K-specialised instantiation of ts_ld_resid, its run-time-K form and the
// K-independent band-product kernels in one translation unit of their own -- csrc/tsamd.hip sees only the launchers declared in
// tsamd_ld_plan.h.
#include <array>
#include <utility>

#include "tsamd_ld_kernels.h"

namespace tsamd {

namespace {
using LdResidKernel = void (*)(const LdArgs);
template <int... Ks>
constexpr void fill(LdResidKernel *t, std::integer_sequence<int, Ks...>) {
  ((t[Ks] = ts_ld_resid<Ks>), ...);
}
LdResidKernel ld_resid_kernel(uint32_t K) {
  static_assert(TSAMD_SPECIALIZED_K == 32, "instantiations K = 1 .. TSAMD_SPECIALIZED_K");
  static const std::array<LdResidKernel, TSAMD_SPECIALIZED_K + 1> table = [] {  // [0]: run-time K
    std::array<LdResidKernel, TSAMD_SPECIALIZED_K + 1> t{};
    fill(t.data(), std::make_integer_sequence<int, TSAMD_SPECIALIZED_K + 1>{});
    return t;
  }();
  return table[K <= (uint32_t)TSAMD_SPECIALIZED_K ? K : 0u];
}
}  // namespace

void ld_launch_resid(const LdArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(ld_resid_kernel(a.K), dim3((a.rows4 + kLdResidIndivs - 1u) / kLdResidIndivs, a.lpad / kLdResidBatch), dim3(kLdBlock), 0, stream, a);
}

void ld_launch_pairs(const LdArgs &a, const LdChunk &c, uint32_t ov, uint32_t pair0, uint32_t npairs, const LdSegs &sg, hipStream_t stream) {
  hipLaunchKernelGGL(ts_ld_syrk, dim3(npairs, sg.nseg), dim3(kLdBlock), 0, stream, a.z, a.m, a.lpad, c.rows, c.nt, ov, pair0, sg.steps, sg.seg_steps,
                     a.part);
  hipLaunchKernelGGL(ts_ld_finish, dim3(npairs), dim3(kLdBlock), 0, stream, a.part, sg.nseg, pair0, a.acc);
}

void ld_launch_band(const LdArgs &a, const LdChunk &c, uint32_t ov, uint32_t window, double *num, uint32_t *cnt, hipStream_t stream) {
  hipLaunchKernelGGL(ts_ld_band, dim3((window + kLdBlock) / kLdBlock, c.len), dim3(kLdBlock), 0, stream, a.acc, c.rows, c.nt, ov, a.ncols, window, num,
                     cnt);
}

}  // namespace tsamd
