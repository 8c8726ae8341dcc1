#!/usr/bin/env python3
"""Rate of tsamd_theta_info (csrc/tsamd_info_kernels.h) beside the library GEMM on the same device and shape.

    usage: python3 tools/theta_info_rate.py [reps] [m,k,L ...]      (default 3, 8192,8,65536 8192,16,65536)

For every (m, K, L): one engine of m individuals and L locations on synthetic PSD genotypes (2 % missing) with a lambda as after
training; tsamd_theta_info(the whole shard, all locations, both outputs) into preallocated arrays, one warm-up call (allocation
of the scratch buffers, code objects, clocks), then `reps` timed calls on the host clock -- the call is synchronous and ends
with the copy of the rows to pageable host memory.  Printed: the call's median, minimum and maximum and the achieved fraction
of the 78.6 TFLOP/s fp64 peak, on the flops of the two products themselves (2 x 2 m L P) and on the flops the matrix cores
EXECUTE (64 x 64 tiles: P padded to whole column tiles, m to whole tiles of individuals).  For scale, torch fp64 C.T @ BB with
C [L][m] and BB [L][P] random, twice (observed and expected), timed with device events after a warm-up: the library GEMM on the
product alone, without the sweep that computes C from the 2-bit columns -- the yardstick, not the code under test."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import terastructure_amd as ts  # noqa: E402

FP64_PEAK_TFLOPS = 78.6  # MI355X fp64 peak, vector and matrix alike (bench.py uses the same figure)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[2:]] or [(8192, 8, 65536), (8192, 16, 65536)]


def stats(t):
    t = np.array(t)
    return float(np.median(t)), float(t.min()), float(t.max())


for m, k, cols in shapes:
    rng = np.random.default_rng(1)
    theta = rng.dirichlet(np.full(k, 0.2), size=m)
    beta = rng.uniform(0.05, 0.95, size=(cols, k))
    P = k * (k + 1) // 2
    ppad, mpad = (P + 63) // 64 * 64, (m + 63) // 64 * 64
    flops = 4.0 * m * cols * P
    executed = 4.0 * mpad * cols * ppad
    with ts.Engine(m, cols, k) as eng:
        eng.synth_genotypes(theta, beta, seed=3, missing_rate=0.02)
        c = rng.uniform(0.0, 200.0, size=(cols, 1))
        eng.set_lambda_range(np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2))
        eng.set_gamma(rng.gamma(100.0, 0.01, size=(m, k)))
        obs, exp = np.zeros((m, P)), np.zeros((m, P))
        dp = C.POINTER(C.c_double)

        def call():
            t0 = time.perf_counter()
            rc = eng.h.tsamd_theta_info(eng.ctx, None, m, None, cols, obs.ctypes.data_as(dp), exp.ctypes.data_as(dp))
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(eng.last_error())
            return dt

        call()
        med, lo, hi = stats([call() for _ in range(reps)])
        tf, tfx = flops / med / 1e12, executed / med / 1e12
        print(f"m={m} K={k} L={cols} P={P} reps={reps}: tsamd_theta_info {med * 1e3:.1f} ms median (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
              f"{(hi - lo) / med * 100:.1f} %) = {med / cols * 1e6:.3f} us per location -> {tf:.2f} TFLOP/s on the products' 4 m L P = "
              f"{tf / FP64_PEAK_TFLOPS * 100:.1f} % of the {FP64_PEAK_TFLOPS} TFLOP/s fp64 peak; {tfx:.2f} TFLOP/s = {tfx / FP64_PEAK_TFLOPS * 100:.1f} % on the "
              f"{mpad // 64} x {ppad // 64} tiles it executes ({executed / flops:.2f} x the products)", flush=True)
        se = ts.theta_se(obs, k)
        good = se["status"] == 0
        print(f"    {int(good.sum())} of {m} rows identified, median standard error {np.median(se['se'][good]):.2e}, "
              f"mean exp / obs on the diagonal {np.mean(exp[:, 0] / obs[:, 0]):.4f}", flush=True)

    import torch

    dev = torch.device("cuda")
    Cm = torch.rand(cols, m, dtype=torch.float64, device=dev)
    BB = torch.rand(cols, P, dtype=torch.float64, device=dev)

    def gemm():
        return Cm.T @ BB, Cm.T @ BB

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
    print(f"m={m} L={cols} P={P}: torch fp64 C.T @ BB, twice {gmed * 1e3:.1f} ms median (min {glo * 1e3:.1f}, max {ghi * 1e3:.1f}) -> {gtf:.2f} TFLOP/s on "
          f"4 m L P = {gtf / FP64_PEAK_TFLOPS * 100:.1f} % of the peak; tsamd_theta_info's call / the two products = {med / gmed:.2f}", flush=True)
    del Cm, BB
    torch.cuda.empty_cache()
