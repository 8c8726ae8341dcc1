#!/usr/bin/env python3
"""Rate of tsamd_train_loglik (the training-data log-likelihood, csrc/tsamd_loglik_kernels.h): one engine on synthetic
genotypes, the call with all locations over as many columns as were synthesised.

    usage: python3 tools/train_loglik_rate.py [n] [k] [columns] [reps]      (default 1 000 000, 8, 2 048, 7)

Prints microseconds per location, genotype bytes per second (N / 4 bytes a location: the one stream the sweep reads from
HBM) and the fraction of the fp64 vector peak on the ALGORITHMIC flop count 2 K + 5 per (individual, location) entry --
q's K multiply-adds, the product, the two additions into the sums; the log is counted as ONE flop, though it executes
dozens, so the fraction understates what the vector units do.  Two warm-up calls (allocation of the partial-sum buffers,
clocks), then `reps` timed calls: median, minimum and maximum are reported -- the spread is part of the result."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import terastructure_amd as ts  # noqa: E402

FP64_VALU_PEAK_TFLOPS = 78.6  # MI355X fp64 vector peak (bench.py uses the same figure)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
k = int(sys.argv[2]) if len(sys.argv) > 2 else 8
cols = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
rng = np.random.default_rng(1)
theta = rng.dirichlet(np.full(k, 0.2), size=n)
with ts.Engine(n, cols, k) as eng:
    eng.synth_genotypes(theta, rng.uniform(0.05, 0.95, size=(cols, k)), seed=3, missing_rate=0.02)
    eng.set_gamma(rng.gamma(100.0, 0.01, size=(n, k)))
    del theta
    for _ in range(2):
        out = eng.train_loglik(per_loc=False, per_indiv=False)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = eng.train_loglik(per_loc=False, per_indiv=False)
        times.append(time.perf_counter() - t0)
    times = np.array(times)
    med, lo, hi = float(np.median(times)), float(times.min()), float(times.max())
    us = med / cols * 1e6
    gbs = cols * (n / 4) / med / 1e9
    tf = (2 * k + 5) * float(n) * cols / med / 1e12
    print(f"N={n} K={k} columns={cols} reps={reps}: tsamd_train_loglik(all locs) {med * 1e3:.2f} ms median "
          f"(min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; spread {(hi - lo) / med * 100:.1f} %) -> {us:.2f} us per location, "
          f"{gbs:.2f} GB/s of genotypes, {tf:.2f} TFLOP/s algorithmic = {tf / FP64_VALU_PEAK_TFLOPS * 100:.1f} % of the "
          f"{FP64_VALU_PEAK_TFLOPS} TFLOP/s fp64 vector peak; mean log-likelihood {out['sum'] / out['count']:.6f} over {out['count']} entries",
          flush=True)
