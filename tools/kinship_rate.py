#!/usr/bin/env python3
"""Rate of tsamd_kinship (csrc/tsamd_kin_kernels.h) beside the library GEMM on the same device and sizes.

    usage: python3 tools/kinship_rate.py [k] [reps] [m,L ...]      (default 8, 3, 4096,65536 8192,65536)

For every (m, L): one engine of m individuals and L locations on synthetic PSD genotypes (2 % missing) with a lambda as
after training; tsamd_kinship(all individuals, all locations, kin only) into a preallocated array, one warm-up call
(allocation of the scratch buffers, code objects, clocks), then `reps` timed calls on the host clock -- the call is
synchronous and ends with the copy of the m x m result to pageable host memory, which is part of what a user waits for and
is printed separately as an estimate (a second call that asks for num and den too, minus the first).  Printed: the call's
median, minimum and maximum, microseconds per location, and the achieved fraction of the 78.6 TFLOP/s fp64 peak on
4 m^2 L flops (two products of 2 m^2 L each; the symmetric half the kernel skips is counted, so the figure compares with a
GEMM's and can exceed 100 %), and beside it the fraction on the flops the kernel EXECUTES: the tile pairs ti <= tj of 64 x
64, a little over half.  For scale, torch fp64 R @ R.T plus S @ S.T with R, S [m][L] random, timed with device events after a warm-up:
the library GEMM is the yardstick, not the code under test."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import terastructure_amd as ts  # noqa: E402

FP64_PEAK_TFLOPS = 78.6  # MI355X fp64 peak, vector and matrix alike (bench.py uses the same figure)

k = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[3:]] or [(4096, 65536), (8192, 65536)]
dp = C.POINTER(C.c_double)


def stats(t):
    t = np.array(t)
    return float(np.median(t)), float(t.min()), float(t.max())


for m, cols in shapes:
    rng = np.random.default_rng(1)
    theta = rng.dirichlet(np.full(k, 0.2), size=m)
    beta = rng.uniform(0.05, 0.95, size=(cols, k))
    flops = 4.0 * m * m * cols
    tiles = (m + 63) // 64
    executed = 4.0 * 64 * 64 * (tiles * (tiles + 1) // 2) * cols  # the upper triangle of 64 x 64 tile pairs, both products
    with ts.Engine(m, cols, k) as eng:
        eng.synth_genotypes(theta, beta, seed=3, missing_rate=0.02)
        c = rng.uniform(0.0, 200.0, size=(cols, 1))
        eng.set_lambda_range(np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2))
        eng.set_gamma(rng.gamma(100.0, 0.01, size=(m, k)))
        out = [np.zeros((m, m)) for _ in range(3)]

        def call(parts):
            t0 = time.perf_counter()
            rc = eng.h.tsamd_kinship(eng.ctx, None, m, None, cols, out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp) if parts else None,
                                     out[2].ctypes.data_as(dp) if parts else None)
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(eng.last_error())
            return dt

        call(False)
        med, lo, hi = stats([call(False) for _ in range(reps)])
        med3, _, _ = stats([call(True) for _ in range(reps)])
        copy = max(0.0, (med3 - med) / 2.0)  # one m x m matrix to pageable host memory
        tf = flops / med / 1e12
        print(f"m={m} L={cols} K={k} reps={reps}: tsamd_kinship(kin) {med * 1e3:.1f} ms median (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
              f"{(hi - lo) / med * 100:.1f} %) -> {med / cols * 1e6:.3f} us per location, {tf:.2f} TFLOP/s on 4 m^2 L = "
              f"{tf / FP64_PEAK_TFLOPS * 100:.1f} % of the {FP64_PEAK_TFLOPS} TFLOP/s fp64 peak ({executed / med / 1e12:.2f} TFLOP/s = "
              f"{executed / med / 1e12 / FP64_PEAK_TFLOPS * 100:.1f} % on the {executed / flops * 100:.1f} % of them it executes); of the call about {copy * 1e3:.1f} ms "
              f"are the copy of one {m} x {m} result to the host ({(med - copy) / cols * 1e6:.3f} us per location without it)", flush=True)
        diag = np.diag(out[0])
        print(f"    mean self-kinship {diag.mean():.4f}, mean |off-diagonal| {np.abs(out[0] - np.diag(diag)).sum() / (m * (m - 1)):.5f}", flush=True)
    del out

    import torch

    dev = torch.device("cuda")
    R = torch.randn(m, cols, dtype=torch.float64, device=dev)
    S = torch.rand(m, cols, dtype=torch.float64, device=dev)

    def gemm():
        return R @ R.T, S @ S.T

    gemm()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gemm()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    gmed, glo, ghi = stats(times)
    gtf = flops / gmed / 1e12
    print(f"m={m} L={cols}: torch fp64 R @ R.T + S @ S.T {gmed * 1e3:.1f} ms median (min {glo * 1e3:.1f}, max {ghi * 1e3:.1f}) -> "
          f"{gmed / cols * 1e6:.3f} us per location, {gtf:.2f} TFLOP/s = {gtf / FP64_PEAK_TFLOPS * 100:.1f} % of the peak; "
          f"tsamd_kinship's call / the two GEMMs = {med / gmed:.2f}", flush=True)
    del R, S
    torch.cuda.empty_cache()
