// The batched validation-mode kernel ts_holblock<K> (tsamd_holblock_kernels.h), one translation unit per
// K <= kResidentMaxK, compiled with -DTSAMD_K=<k> (terastructure_amd/build.py).
#include "tsamd_holblock_kernels.h"
#include "tsamd_unit.h"

namespace tsamd {

static_assert(TSAMD_K <= kResidentMaxK, "ts_holblock holds the shard's weights in registers");

// n hol-mode entries at `sched` (pinned host memory), pairwise distinct locations, no gamma step pending; same launch
// geometry as ts_schedule (its per-thread partial sums are the same sums)
static void launch(uint32_t grid, uint32_t chunk, hipStream_t stream, const DevParams &p, uint32_t par, const uint32_t *sched, uint32_t n,
                   uint32_t serial) {
  // (a sharded context: the instantiation whose level 2 spans the ranks' group leaders -- WR = 8 up to 2 ranks; 32 above: up to 64
  // rows, polled 16 row pairs at a time)
  if (p.xchg_world == 0u)
    hipLaunchKernelGGL((ts_holblock<TSAMD_K, 0>), dim3(grid), dim3(kResidentBlock), 0, stream, p.ctl, p.w, p.npad, chunk, par, sched, n, p.res, serial, p);
  else if (p.xchg_world <= 2u)
    hipLaunchKernelGGL((ts_holblock<TSAMD_K, 8>), dim3(grid), dim3(kResidentBlock), 0, stream, p.ctl, p.w, p.npad, chunk, par, sched, n, p.res, serial, p);
  else
    hipLaunchKernelGGL((ts_holblock<TSAMD_K, 32>), dim3(grid), dim3(kResidentBlock), 0, stream, p.ctl, p.w, p.npad, chunk, par, sched, n, p.res, serial,
                       p);
}

static int blocks_per_cu() { return min_blocks_per_cu(ts_holblock<TSAMD_K, 0>, ts_holblock<TSAMD_K, 8>, ts_holblock<TSAMD_K, 32>); }

// (batch: locations per exchange / per launch -- what the host cuts a validation-mode schedule into)
TSAMD_EXPORT_OPS(WholeOps, holblock, launch, blocks_per_cu, hol_batch(TSAMD_K));

}  // namespace tsamd
