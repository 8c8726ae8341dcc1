#!/usr/bin/env python3
"""Rate of tsamd_snp_scan (per-SNP fit and association sums, csrc/tsamd_scan_kernels.h) with and without a trait, beside
tsamd_train_loglik on the SAME engine: one engine on synthetic genotypes, every call with all locations over as many columns
as were synthesised.

    usage: python3 tools/scan_rate.py [n] [k] [columns] [reps]      (default 1 000 000, 8, 2 048, 7)

Prints, per call, microseconds per location with the spread, genotype bytes per second (N / 4 bytes a location: the one stream
the sweep reads from HBM) and the fraction of the fp64 vector peak on the ALGORITHMIC flop count per (individual, location)
entry: 2 K + 25 for the scan with a trait, 2 K + 12 without (q's K multiply-adds; h, r, q^2, (1-q)^2, h(1-h) and the masked
additions; with a trait t r, t (t h), t h and theirs), 2 K + 5 for the log-likelihood (its log counted as ONE flop).  Two
warm-up calls each (allocation of the partial-sum buffers, clocks), then `reps` timed calls: median, minimum and maximum are
reported -- the spread is part of the result."""
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
trait = rng.normal(0.0, 1.0, size=n)
trait[rng.random(n) < 0.05] = np.nan
with ts.Engine(n, cols, k) as eng:
    eng.synth_genotypes(theta, rng.uniform(0.05, 0.95, size=(cols, k)), seed=3, missing_rate=0.02)
    eng.set_gamma(rng.gamma(100.0, 0.01, size=(n, k)))
    del theta
    calls = (("tsamd_snp_scan(all locs, trait)", 2 * k + 25, lambda: eng.snp_scan(trait=trait)),
             ("tsamd_snp_scan(all locs)", 2 * k + 12, lambda: eng.snp_scan()),
             ("tsamd_train_loglik(all locs)", 2 * k + 5, lambda: eng.train_loglik(per_loc=False, per_indiv=False)))
    medians = {}
    for name, flops, call in calls:
        for _ in range(2):
            call()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        times = np.array(times)
        med, lo, hi = float(np.median(times)), float(times.min()), float(times.max())
        medians[name] = med
        us = med / cols * 1e6
        gbs = cols * (n / 4) / med / 1e9
        tf = flops * float(n) * cols / med / 1e12
        print(f"N={n} K={k} columns={cols} reps={reps}: {name} {med * 1e3:.2f} ms median (min {lo * 1e3:.2f}, max {hi * 1e3:.2f}; "
              f"spread {(hi - lo) / med * 100:.1f} %) -> {us:.2f} us per location, {gbs:.2f} GB/s of genotypes, {tf:.2f} TFLOP/s algorithmic "
              f"({flops} flops per entry) = {tf / FP64_VALU_PEAK_TFLOPS * 100:.1f} % of the {FP64_VALU_PEAK_TFLOPS} TFLOP/s fp64 vector peak",
              flush=True)
    ll = medians["tsamd_train_loglik(all locs)"]
    print(f"N={n} K={k}: per location, the scan with a trait takes {medians['tsamd_snp_scan(all locs, trait)'] / ll:.2f} x and without one "
          f"{medians['tsamd_snp_scan(all locs)'] / ll:.2f} x the time of tsamd_train_loglik", flush=True)
