"""tsamd_ld against the long-double reference of tests/analysis_refs.py (ld_ref) from the PLANTED inputs alone -- genotypes as
PLINK bytes, gamma, lambda, the held-out lists -- within that module's derived first-order bound, at EVERY K, from a
late-training state, across geometries, on a wide band, with a q of exactly 1 and across three shards.  No reference takes a
value read from the engine (tests/test_gpu_ld.py and test_gpu_ld_every_k.py do, at a flat 1e-11 sum |z z|): before any call
the reads are pinned to the planted values (pin_reads).  cnt is exact, the entries past the list's end are exactly 0, every
value is finite; the limit for num is 1.0 x the bound.

  * test_every_k: K = 1 .. 32 (every instantiation of ts_ld_resid<K>) and 33, 64, 128 (the run-time-K form) at n = 602 (three
    workgroups of ts_ld_resid, the last ragged, the last k-step of 4 half empty; individuals 0 and n - 1 held out), l = 150
    (three location tiles, the last of 22), W = 65 (two overlap tiles), on the full list and on an unsorted list of 78 with a
    repeat and both ends, which spans two tiles.
  * test_late_state: analysis_refs.LATE_SHAPES (Ebeta within 1e-6 of 0 and 1, gamma from the 1e-8 floor; at (4200, 36, 3)
    max |z| is 388 and the bound reaches 8.2e-11 sum |z z|, where a flat 1e-11 is no valid tolerance), W = l - 1, rank 1 of 3
    among them; the state export unchanged.  test_late_state_across_geometries: (1030, 150, 8), W = 65, under the test hooks.
  * test_wide_band: l = 600, W = 512 (eight overlap tiles, ten location tiles, the short tile rows of ld_pair) and
    W = TSAMD_LD_MAX_WINDOW, wider than the list.
  * test_q_of_exactly_one_is_no_term: the h <= 0 rule of ld_terms on the device.
  * test_shards_add_up: three ranks, each against its own shard's reference.

Measured once on one MI355X (2026-10-21), worst |gpu - ref| / bound: 2.3e-2 over the 35 every-K tests (K = 1, where every
individual shares q and its rounding does not average out; at most 8.1e-3 from K = 2 on, 2.4e-3 at K = 128); 9.2e-2 over the
five late-state shapes (n = 4200, K = 3; a plain fp64 numpy evaluation reaches the same 9.2e-2; 1.9e-2 at most at the other
four); at (1030, 150, 8) 9.4e-3 on the engine's own geometry, 1.0e-2 with chunks of 64 and blocks of 100, 1.7e-2 on four units;
the wide band 9.8e-3 at W = 512 and 1.0e-2 at W = 1024; 2.4e-2 for the first call of the q = 1 test; 7.8e-3 over the three
shards and one context, their sum 8.8e-3 of the three bounds' sum away from one context's.  The 44 tests took 11 s together
(0.2 s per every-K case, 1.3 s for the wide band, most of it the long-double references).  With ts_ld_resid changed by hand to
read theta of individual n ^ 1, 42 of the 44 failed, at ratios of 1e10 and more (the two K = 1 tests, where theta is 1 for
everybody, cannot see it).
"""
import numpy as np
import pytest

import analysis_refs as ar
import late_state
from helpers import pack_bed
from test_gpu_analysis_every_k import pin_reads
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

LD_HOOKS = ("TSAMD_TEST_LD_CHUNK", "TSAMD_TEST_LD_BLOCK", "TSAMD_TEST_MAX_WORKGROUPS")


def load(eng, c, shard=None):
    """the planted case into an engine as PLINK bytes, gamma, lambda and held-out lists; the reads pinned"""
    b, n = (0, c.n) if shard is None else shard
    eng.upload_bed(pack_bed(c.y))
    eng.set_gamma(c.gamma[b:b + n])
    eng.set_lambda_range(c.lam)
    for loc, ids in c.held.items():
        eng.set_heldout(loc, ids)
    pin_reads(eng, c, shard)


def both_lists(c, window, shard=None):
    """[(list, ref, bound)] of c.locs and of the full list, from one Entries"""
    every = ar.Entries(c.y, c.gamma, c.lam, c.held, None, shard)
    return [(which, *ar.ld_ref(c.y, c.gamma, c.lam, window, c.held, which, shard, entries=every)) for which in (c.locs, None)]


def check_the_repeat(c, got, bound):
    """c.locs' last but one entry repeats its second: a row of its own whose column 0 is that of the first appearance"""
    rep, first = len(c.locs) - 2, 1
    assert c.locs[rep] == c.locs[first]
    assert got["cnt"][rep, 0] == got["cnt"][first, 0]
    assert abs(ar.LD(got["num"][rep, 0]) - ar.LD(got["num"][first, 0])) <= bound["num"][rep, 0] + bound["num"][first, 0]


@pytest.mark.parametrize("k", ar.EVERY_K)
def test_every_k(ts, k):
    c = ar.plant_every_k(k, n=602, l=150)
    w = 65
    assert len(c.locs) == 78 and list(c.locs) != sorted(c.locs) and {0, c.l - 1} <= set(c.locs.tolist()) and 0 in c.held[0] and c.n - 1 in c.held[0]
    worst = 0.0
    with ts.Engine(c.n, c.l, k) as eng:
        load(eng, c)
        for which, ref, bound in both_lists(c, w):
            got = eng.ld(which, w)
            worst = max(worst, ar.compare_ld(got, ref, bound))
            if which is not None:
                check_the_repeat(c, got, bound)
    print(f"K={k}: worst |gpu - ref| / bound: ld {worst:.3e}")


@pytest.mark.parametrize("n,l,k,world,rank", ar.LATE_SHAPES)
def test_late_state(ts, n, l, k, world, rank):
    c, s = ar.plant_late(n, l, k, world, rank)
    w = l - 1
    worst = 0.0
    with ts.Engine(n, l, k, rank=rank, world=world) as eng:
        assert (eng.shard_begin, eng.shard_count) == c.shard
        assert world == 1 or eng.shard_begin == 344
        late_state.load_engine(eng, s)
        pin_reads(eng, c, c.shard)
        before = eng.state_export()
        for which, ref, bound in both_lists(c, w, c.shard):
            got = eng.ld(which, w)
            worst = max(worst, ar.compare_ld(got, ref, bound))
            if which is not None:
                check_the_repeat(c, got, bound)
        after = eng.state_export()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    print(f"late n={n} l={l} K={k} rank {rank} of {world}: worst |gpu - ref| / bound: ld {worst:.3e}")


def test_late_state_across_geometries(ts, monkeypatch):
    """the engine's own geometry, chunks of 64 locations with blocks of 100 individuals (three chunks with two overlap tiles
    each, eleven blocks, the later ones off a dword) and a four-unit device's: each within the bound, cnt the same bytes"""
    n, l, k, w = 1030, 150, 8, 65
    c, s = ar.plant_late(n, l, k)
    for var in LD_HOOKS:
        monkeypatch.delenv(var, raising=False)
    refs = both_lists(c, w, c.shard)
    worst, cnts = {}, {}

    def run(eng, name):
        got = [eng.ld(which, w) for which, _, _ in refs]
        worst[name] = max(ar.compare_ld(g, ref, bound) for g, (_, ref, bound) in zip(got, refs))
        cnts[name] = [g["cnt"].tobytes() for g in got]

    with ts.Engine(n, l, k, flags=ts.FLAG_TEST_HOOKS) as eng:
        late_state.load_engine(eng, s)
        pin_reads(eng, c, c.shard)
        run(eng, "own")
        monkeypatch.setenv("TSAMD_TEST_LD_CHUNK", "64")
        monkeypatch.setenv("TSAMD_TEST_LD_BLOCK", "100")
        run(eng, "chunk 64, block 100")
        monkeypatch.delenv("TSAMD_TEST_LD_CHUNK")
        monkeypatch.delenv("TSAMD_TEST_LD_BLOCK")
    monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
    with ts.Engine(n, l, k, flags=ts.FLAG_TEST_HOOKS) as small:
        late_state.load_engine(small, s)
        pin_reads(small, c, c.shard)
        run(small, "four units")
    print("late n=1030 l=150 K=8, worst |gpu - ref| / bound: " + ", ".join(f"{name} {v:.3e}" for name, v in worst.items()))
    assert cnts["own"] == cnts["chunk 64, block 100"] == cnts["four units"]


def test_wide_band(ts):
    c = ar.plant_every_k(3, n=302, l=600)
    wmax = ts._lib.LD_MAX_WINDOW
    assert wmax > c.l
    # one reference: every pair of the list lies inside the widest window, and a narrower band is its first columns
    ref, bound = ar.ld_ref(c.y, c.gamma, c.lam, wmax, c.held)
    assert np.all(ref["cnt"][:, c.l:] == 0)
    worst = {}
    with ts.Engine(c.n, c.l, c.k) as eng:
        load(eng, c)
        for w in (512, wmax):
            got = eng.ld(None, w)
            assert got["num"].shape == (c.l, w + 1)
            worst[w] = ar.compare_ld(got, {key: v[:, :w + 1] for key, v in ref.items()}, dict(num=bound["num"][:, :w + 1]))
    print("wide band, worst |gpu - ref| / bound: " + ", ".join(f"W={w} {v:.3e}" for w, v in worst.items()))


def test_q_of_exactly_one_is_no_term(ts):
    """K = 1: theta is exactly 1 and q is Ebeta.  lambda = (1e20, 1) gives Ebeta = 1e20 / (1e20 + 1) = 1.0 in fp64, so h = 0:
    ld_terms gives no term, never a NaN.  Every entry of the band with the location in it is an exact 0; every other entry
    keeps its bits (an element of the MFMA's output depends on its own two operand rows only)."""
    n, l, w, loc = 300, 70, 9, 20
    c = ar.plant_every_k(1, n=n, l=l)
    with ts.Engine(n, l, 1) as eng:
        load(eng, c)
        first = eng.ld(None, w)
        worst = ar.compare_ld(first, *ar.ld_ref(c.y, c.gamma, c.lam, w, c.held))
        assert first["cnt"][loc, 0] > 0 and first["num"][loc, 0] > 0.0
        eng.set_lambda(loc, np.array([[1e20, 1.0]]))
        assert eng.get_ebeta()[loc, 0] == 1.0
        second = eng.ld(None, w)
    with_loc = np.zeros((l, w + 1), dtype=bool)
    with_loc[loc, :] = True
    for i in range(max(0, loc - w), loc):
        with_loc[i, loc - i] = True
    assert int(with_loc.sum()) == 2 * w + 1
    assert np.all(second["num"][with_loc] == 0.0) and np.all(second["cnt"][with_loc] == 0)
    assert second["num"][~with_loc].tobytes() == first["num"][~with_loc].tobytes()
    assert second["cnt"][~with_loc].tobytes() == first["cnt"][~with_loc].tobytes()
    assert np.all(np.isfinite(second["num"]))
    r, p = ts.ld_statistics(second["num"], second["cnt"])
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(p)) and np.all(r[with_loc] == 0.0) and np.all(p[with_loc] == 1.0)
    print(f"q = 1: the first call's worst |gpu - ref| / bound: ld {worst:.3e}")


def test_shards_add_up(ts):
    n, l, k, w, world = 1030, 70, 6, 9, 3
    c = ar.plant_every_k(k, n=n, l=l)
    bands, bounds, worst = [], [], 0.0
    for rank in range(world):
        shard = ar.shard_of(n, rank, world)
        with ts.Engine(n, l, k, rank=rank, world=world) as eng:
            assert (eng.shard_begin, eng.shard_count) == shard
            load(eng, c, shard)
            got = eng.ld(None, w)
        ref, bound = ar.ld_ref(c.y, c.gamma, c.lam, w, c.held, None, shard)
        worst = max(worst, ar.compare_ld(got, ref, bound))
        bands.append(got)
        bounds.append(bound["num"])
    with ts.Engine(n, l, k) as one:
        load(one, c)
        whole = one.ld(None, w)
    ref, bound = ar.ld_ref(c.y, c.gamma, c.lam, w, c.held)
    worst = max(worst, ar.compare_ld(whole, ref, bound))
    assert sum(b["cnt"].astype(np.uint64) for b in bands).astype(np.uint32).tobytes() == whole["cnt"].tobytes()
    total = sum(b["num"].astype(ar.LD) for b in bands)
    allowed = sum(bounds)
    # each rank lies within its bound of its shard's exact sum, and those exact sums add up to the whole's
    exact = ar.ratio(total, ref["num"], allowed)
    both = ar.ratio(total, whole["num"], allowed)
    print(f"three shards: worst |gpu - ref| / bound: ld {worst:.3e}; their sum, as multiples of the three bounds' sum: "
          f"{exact:.3e} from the reference, {both:.3e} from one context")
    assert exact <= 1.0 and both <= 1.0
