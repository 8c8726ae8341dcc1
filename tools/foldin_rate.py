#!/usr/bin/env python3
"""Rate of tsamd_fold_in (gamma against a fixed lambda, csrc/tsamd_foldin_kernels.h) beside tsamd_train_loglik on the same
engine: synthetic genotypes, a lambda as after training, the call over all synthesised columns with tol = 0.

    usage: python3 tools/foldin_rate.py [n] [k] [columns] [iters] [reps]      (default 1 000 000, 8, 2 048, 5, 5)

Prints microseconds per location and iteration (the whole call divided by iters x columns: sweep, step and the host's read
of the active count after every step), genotype bytes per second, and the fraction of the fp64 vector peak on the
ALGORITHMIC flop count 8 K + 6 per (individual, location) entry -- 4 K multiply-adds, the two reciprocals and the two
products counted as one flop each, though a reciprocal executes four instructions.  Then the same for tsamd_train_loglik
(totals only; 2 K + 5 flops per entry, its yardstick: the genotype stream is the same).  One warm-up call each
(allocation of the scratch buffers, clocks), then `reps` timed calls: median, minimum and maximum are reported."""
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
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 5
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
rng = np.random.default_rng(1)
theta = rng.dirichlet(np.full(k, 0.2), size=n)
beta = rng.uniform(0.05, 0.95, size=(cols, k))


def timed(fn):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    t = np.array(t)
    return float(np.median(t)), float(t.min()), float(t.max()), out


with ts.Engine(n, cols, k) as eng:
    eng.synth_genotypes(theta, beta, seed=3, missing_rate=0.02)
    c = rng.uniform(0.0, 200.0, size=(cols, 1))
    eng.set_lambda_range(np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2))
    g0 = rng.gamma(100.0, 0.01, size=(n, k))
    del theta

    def fold():
        eng.set_gamma(g0)
        t0 = time.perf_counter()
        out = eng.fold_in(max_iters=iters, tol=0.0)
        out["seconds"] = time.perf_counter() - t0
        return out

    fold()
    secs = np.array([fold()["seconds"] for _ in range(reps)])
    med, lo, hi = float(np.median(secs)), float(secs.min()), float(secs.max())
    us = med / (cols * iters) * 1e6
    gbs = cols * iters * (n / 4) / med / 1e9
    tf = (8 * k + 6) * float(n) * cols * iters / med / 1e12
    print(f"N={n} K={k} columns={cols} iters={iters} reps={reps}: tsamd_fold_in(all locs, tol 0) {med * 1e3:.2f} ms median "
          f"(min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; spread {(hi - lo) / med * 100:.1f} %) -> {us:.3f} us per location and iteration, "
          f"{gbs:.2f} GB/s of genotypes, {tf:.2f} TFLOP/s algorithmic = {tf / FP64_VALU_PEAK_TFLOPS * 100:.1f} % of the "
          f"{FP64_VALU_PEAK_TFLOPS} TFLOP/s fp64 vector peak", flush=True)
    lmed, llo, lhi, out = timed(lambda: eng.train_loglik(per_loc=False, per_indiv=False))
    ltf = (2 * k + 5) * float(n) * cols / lmed / 1e12
    print(f"N={n} K={k} columns={cols}: tsamd_train_loglik(all locs) {lmed * 1e3:.2f} ms median (min {llo * 1e3:.2f}, max {lhi * 1e3:.2f}) -> "
          f"{lmed / cols * 1e6:.3f} us per location, {ltf:.2f} TFLOP/s algorithmic = {ltf / FP64_VALU_PEAK_TFLOPS * 100:.1f} % of the peak; "
          f"fold-in fraction / loglik fraction = {tf / ltf:.2f}", flush=True)
