"""The four analysis calls from the state they are used in: a planted late-training model (tests/late_state.py with lambda
scaled to an effective sample of 1e6), against the extended-precision references and derived bounds of
tests/analysis_refs.py, from the planted inputs alone.

There gamma components sit at the 1e-8 floor next to ones of order 1e6, Ebeta lies within 1e-6 of 0 and 1, 1 - q cancels
(min q and min 1 - q of order 1e-6 at K = 3 and 8), and sqrt(q (1 - q)) and the fold-in's w span hundreds of orders of
magnitude.  The per-individual log-likelihood is NOT held to 1e-11 |ref| here: one entry with 1 - q = 4e-6 carries
(2K + 4) u / 4e-6 = 5e-10 into a sum of about 40 terms; the bound is derived from each entry's conditioning instead.

Shapes: (1030, 40, 8), (2050, 40, 20), (4200, 36, 3), (700, 40, 33) and (1030, 40, 8) as rank 1 of 3, whose shard begins
at individual 344: no multiple of 16.  The comparisons are those of test_gpu_analysis_every_k.py, on its two geometries (the
device's own: segments of one batch; a two-unit device's: where the shard has two tiles or more -- all but the K = 8 shapes --
one segment with a second batch of 8 or 4 locations), with fold_in for 1 and 5 updates; on top: every output finite, loc_sums <= 0, the floor components of a floor row exactly alpha after one
fold-in update (their w underflows to 0), and the state export byte for byte the same after the three read-only calls.

Measured once on one MI355X (2026-10-20), worst |gpu - ref| / bound over the five shapes and both geometries: train_loglik
2.9e-2 (K = 3), snp_scan 1.4e-3 (rank 1 of 3), kinship 1.9e-1 (K = 3; its bound carries no factor 4, and a plain fp64 numpy
evaluation reaches the same 1.9e-1), fold_in gamma 1.1e-4 of the relative 1e-9 (K = 33), sum_k gamma 1.1e-4 of the relative
1e-11 (K = 33).  The five tests took 0.8 s together.
"""
import numpy as np
import pytest

import analysis_refs as ar
import late_state
from test_gpu_analysis_every_k import pin_reads, run_families, two_geometries
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,l,k,world,rank", ar.LATE_SHAPES)
def test_late_state(ts, n, l, k, world, rank, monkeypatch):
    c, s = ar.plant_late(n, l, k, world, rank)
    b, cnt = c.shard
    engines = two_geometries(ts, monkeypatch, n, l, k, rank, world)
    try:
        for eng in engines:
            assert (eng.shard_begin, eng.shard_count) == c.shard and eng.cfg.alpha == c.alpha
            assert world == 1 or eng.shard_begin % 16 != 0
            late_state.load_engine(eng, s)
            et, ee = pin_reads(eng, c, c.shard)
            before = eng.state_export()
            eng.train_loglik(c.locs)
            eng.snp_scan(c.locs, c.trait[b:b + cnt])
            eng.kinship(c.ids, c.locs)
            after = eng.state_export()
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        worst, full = run_families(engines, c, (1, 5), c.shard)
    finally:
        for eng in engines:
            eng.close()
    print(f"late n={n} l={l} K={k} rank {rank} of {world}: theta {et:.2f} u, Ebeta {ee:.2f} u; worst |gpu - ref| / bound: "
          + ", ".join(f"{f} {v:.3e}" for f, v in worst.items()))
    ll, scan, kin = full["loglik"], full["scan"], full["kin"]
    for a in (ll["loc_sums"], ll["indiv_sums"], ll["sum"], scan["fit_sums"], scan["trait_sums"], *kin, full["foldin"][1], full["foldin"][5]):
        assert np.all(np.isfinite(a))
    assert np.all(ll["loc_sums"] <= 0.0) and np.all(ll["indiv_sums"] <= 0.0)
    rows = c.floor_rows[(c.floor_rows >= b) & (c.floor_rows < b + cnt)]
    assert len(rows) > 0
    for i in rows:
        at_floor = c.gamma[i] == 1e-8
        assert at_floor.any() and np.all(full["foldin"][1][i - b][at_floor] == c.alpha), i
