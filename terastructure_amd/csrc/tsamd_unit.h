// What the per-K translation units (tsamd_inst.hip, tsamd_sched.hip, tsamd_hol.hip, tsamd_hyb.hip, tsamd_hhol.hip; compiled
// with -DTSAMD_K=<k>, terastructure_amd/build.py) share, and what each exports to csrc/tsamd.hip: ONE const ops object per K.
// Include after the kernel header of the unit.
#pragma once
#include <hip/hip_runtime.h>

#include "tsamd_kernels.h"

#if !defined(TSAMD_K) && !defined(TSAMD_MAIN_TU)
#error "compile with -DTSAMD_K=<populations>"
#endif
#define TSAMD_CAT2(a, b) a##b
#define TSAMD_CAT(a, b) TSAMD_CAT2(a, b)

namespace tsamd {

// tsamd_inst.hip: the launch-per-pass kernels and ts_resident (LaunchFn: tsamd_kernels.h)
struct PassOps {
  LaunchFn launch;
  int (*first_blocks_per_cu)(int vec);  // resident first-pass workgroups per compute unit (register-bound: 2 at K = 8, 1 from K = 12)
  int (*resident_blocks_per_cu)();      // can a workgroup of ts_resident run on a compute unit (register budget)?
};

// the whole-launch units: n entries at `sched` (pinned host or device memory), starting from and leaving the State of parity par
using ScheduleFn = void (*)(uint32_t grid, uint32_t chunk, hipStream_t stream, const DevParams &p, uint32_t par, const uint32_t *sched,
                            uint32_t n, uint32_t serial);
struct WholeOps {
  ScheduleFn launch;
  int (*blocks_per_cu)();  // does a workgroup of it fit a compute unit (register / LDS budget)?  (worst case of the instantiations)
  int batch;               // ts_holblock / ts_hybhol: locations per exchange (what tsamd_holblock_info reports); 0 elsewhere
};

// The ops object of a unit is host data (the device pass of the compilation must not see it: it points at host functions).
#ifdef __HIP_DEVICE_COMPILE__
#define TSAMD_EXPORT_OPS(type, family, ...)
#else
#define TSAMD_EXPORT_OPS(type, family, ...) extern const type TSAMD_CAT(family##_ops_k, TSAMD_K) = {__VA_ARGS__}
#endif

// workgroups of 256 threads per compute unit, worst case of `kernels` (0: one of them does not fit, or cannot be queried)
template <class... Kernels>
int min_blocks_per_cu(Kernels... kernels) {
  int worst = 1 << 30;
  auto probe = [&](auto kernel) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, 0) != hipSuccess) nb = 0;
    worst = nb < worst ? nb : worst;
  };
  (probe(kernels), ...);
  return worst;
}

}  // namespace tsamd
