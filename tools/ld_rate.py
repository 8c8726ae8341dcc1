#!/usr/bin/env python3
"""Rate of tsamd_ld (csrc/tsamd_ld_kernels.h) beside the library GEMM on the same device and shape.

    usage: python3 tools/ld_rate.py [reps] [n,k,L,W ...]      (default 3, 1000000,8,4096,256 500000,16,4096,256)

For every (N, K, L, W): one engine of N individuals and L locations on synthetic PSD genotypes (2 % missing) with a lambda as
after training; tsamd_ld(all locations, window W, num and cnt) into preallocated bands, one warm-up call (allocation of the
scratch buffers, code objects, clocks), then `reps` timed calls on the host clock -- the call is synchronous and ends with the
copy of the two bands to pageable host memory.  Printed: the call's median, minimum and maximum and the achieved fraction of
the 78.6 TFLOP/s fp64 peak, on the flops of the band itself (two products, 2 N flops per pair, L (W + 1) pairs less the corner
past the list's end) and on the flops the kernels EXECUTE (64 x 64 tile pairs: whole tiles on and beside the band).  For
scale, torch fp64 Z.T @ Z with Z [N][L] random, twice (the second product stands for the masks'), timed with device events
after a warm-up: the full L x L products, of which the band is a part -- the library GEMM is the yardstick, not the code under
test."""
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
shapes = [tuple(int(x) for x in a.split(",")) for a in sys.argv[2:]] or [(1000000, 8, 4096, 256), (500000, 16, 4096, 256)]


def stats(t):
    t = np.array(t)
    return float(np.median(t)), float(t.min()), float(t.max())


for n, k, cols, w in shapes:
    rng = np.random.default_rng(1)
    theta = rng.dirichlet(np.full(k, 0.2), size=n)
    beta = rng.uniform(0.05, 0.95, size=(cols, k))
    band_pairs = cols * (w + 1) - w * (w + 1) // 2
    flops = 4.0 * n * band_pairs
    tiles, ov = (cols + 63) // 64, (w + 63) // 64
    tile_pairs = sum(min(ov, tiles - 1 - t) + 1 for t in range(tiles))
    executed = 4.0 * n * 64 * 64 * tile_pairs
    with ts.Engine(n, cols, k) as eng:
        eng.synth_genotypes(theta, beta, seed=3, missing_rate=0.02)
        c = rng.uniform(0.0, 200.0, size=(cols, 1))
        eng.set_lambda_range(np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2))
        eng.set_gamma(rng.gamma(100.0, 0.01, size=(n, k)))
        del theta
        num, cnt = np.zeros((cols, w + 1)), np.zeros((cols, w + 1), dtype=np.uint32)

        def call():
            t0 = time.perf_counter()
            rc = eng.h.tsamd_ld(eng.ctx, None, cols, w, num.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
            dt = time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(eng.last_error())
            return dt

        call()
        med, lo, hi = stats([call() for _ in range(reps)])
        tf, tfx = flops / med / 1e12, executed / med / 1e12
        print(f"N={n} K={k} L={cols} W={w} reps={reps}: tsamd_ld {med * 1e3:.1f} ms median (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; spread "
              f"{(hi - lo) / med * 100:.1f} %) -> {tf:.2f} TFLOP/s on the band's 4 N x {band_pairs} pairs = {tf / FP64_PEAK_TFLOPS * 100:.1f} % of the "
              f"{FP64_PEAK_TFLOPS} TFLOP/s fp64 peak; {tfx:.2f} TFLOP/s = {tfx / FP64_PEAK_TFLOPS * 100:.1f} % on the {tile_pairs} tile pairs it executes "
              f"({executed / flops:.2f} x the band)", flush=True)
        r, _ = ts.ld_statistics(num, cnt)
        print(f"    mean cnt on the diagonal {cnt[:, 0].mean():.0f}, mean r on it {r[:, 0].mean():.4f}, mean r^2 off it {(r[:, 1:] ** 2).mean():.2e}", flush=True)

    import torch

    dev = torch.device("cuda")
    Z = torch.randn(n, cols, dtype=torch.float64, device=dev)

    def gemm():
        return Z.T @ Z, Z.T @ Z

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
    gflops = 4.0 * n * cols * cols
    gtf = gflops / gmed / 1e12
    print(f"N={n} L={cols}: torch fp64 Z.T @ Z, twice {gmed * 1e3:.1f} ms median (min {glo * 1e3:.1f}, max {ghi * 1e3:.1f}) -> {gtf:.2f} TFLOP/s on "
          f"4 N L^2 = {gtf / FP64_PEAK_TFLOPS * 100:.1f} % of the peak; tsamd_ld's call / the two full products = {med / gmed:.2f} for "
          f"{executed / gflops * 100:.1f} % of their flops", flush=True)
    del Z
    torch.cuda.empty_cache()
