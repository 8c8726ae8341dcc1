"""tsamd_snp_scan: per-location sufficient statistics of the structure-adjusted fit and association tests, in one sweep of the
listed columns; tsamd_scan_statistics turns them into z and p.

The reference is numpy fp64 from three reads of the engine -- get_theta(), get_ebeta() and download_bed() (which shows
held-out entries as missing, as wanted) -- never from the call under test.  With q = sum_k Ebeta[j][k] Etheta[n][k],
h = 2q(1-q), r = y - 2q, over the entries whose code is not 01:
    fit_sums = sum (1-q)^2, sum h, sum q^2, sum h(1-h);  fit_counts = entries with y = 0, 1, 2;
and over those whose individual carries a trait value t (not NaN):
    trait_sums = sum t, sum t r, sum t^2 h, sum t h, sum r, sum h;  trait_counts = their number.

Tolerance, derived: with M <= 4 099 terms the accumulation error is at most M 2^-53 = 4.6e-13 of sum |term|; q carries at
most about K ulp (1.4e-14 absolute at K = 128).  So the positive sums (E0, E1, E2, VH, sum t^2 h, sum h) are asserted at
1e-11 |ref| + 1e-12, the signed ones (sum t r, sum r, sum t h, sum t) at 1e-11 B with B the sum over the contributing entries
of the term's magnitude bound (2 |t|, 2, |t|, |t|), and the counts exactly.
Measured once on one MI355X (2026-10-19), worst over every comparison of this file: 4.9e-16 of |ref| on the positive sums,
1.4e-16 of B on the signed ones (ts_scan).

Shapes are those of test_gpu_train_loglik.py: one tile with padding, K = 1, N no multiple of 4 / 16 / 512, more than one
tile at every individuals-per-thread figure, and the run-time-K kernel at K = 33 and 128."""
import math

import numpy as np
import pytest

from helpers import pack_bed, unpack_bed
from test_gpu_parity import ts  # noqa: F401
from test_gpu_train_loglik import synth_engine

pytestmark = pytest.mark.gpu

EINVAL = -1
POSITIVE_TRAIT, SIGNED_TRAIT = (2, 5), (0, 1, 3, 4)  # columns of trait_sums
BOUND_OF = {0: lambda t: np.abs(t), 1: lambda t: 2.0 * np.abs(t), 3: lambda t: np.abs(t), 4: lambda t: np.full_like(t, 2.0)}


def make_trait(n, seed, nan_rate=0.05):
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 1.0, size=n)
    t[rng.random(n) < nan_rate] = np.nan
    return t


def reference(eng, locs, trait=None):
    """dict like Engine.snp_scan's, in numpy, with the bounds B of the signed sums under 'trait_bounds'"""
    theta, eb, n = eng.get_theta(), eng.get_ebeta(), eng.shard_count
    locs = [int(x) for x in locs]
    ref = dict(fit_sums=np.zeros((len(locs), 4)), fit_counts=np.zeros((len(locs), 3), dtype=np.uint32))
    if trait is not None:
        ref.update(trait_sums=np.zeros((len(locs), 6)), trait_counts=np.zeros(len(locs), dtype=np.uint32), trait_bounds=np.zeros((len(locs), 6)))
        has = ~np.isnan(trait)
        t = np.where(has, trait, 0.0)
    cache = {}
    for i, loc in enumerate(locs):
        if loc not in cache:
            y = unpack_bed(eng.download_bed(loc)[None, :], n)[0]
            q = theta @ eb[loc]
            ok = y != 3
            h, r = 2.0 * q * (1.0 - q), np.where(ok, y, 0).astype(np.float64) - 2.0 * q
            row = dict(fit_sums=[math.fsum(((1.0 - q) ** 2)[ok]), math.fsum(h[ok]), math.fsum((q * q)[ok]), math.fsum((h * (1.0 - h))[ok])],
                       fit_counts=[int(np.sum(y == v)) for v in (0, 1, 2)])
            if trait is not None:
                m = ok & has
                terms = [t, t * r, t * t * h, t * h, r, h]
                row.update(trait_sums=[math.fsum(x[m]) for x in terms], trait_counts=int(m.sum()),
                           trait_bounds=[math.fsum(BOUND_OF[c](t)[m]) if c in BOUND_OF else 0.0 for c in range(6)])
            cache[loc] = row
        for key, val in cache[loc].items():
            ref[key][i] = val
    return ref


WORST = {}


def assert_matches(got, ref, what=""):
    assert np.array_equal(got["fit_counts"], ref["fit_counts"]), what + "fit_counts"
    g, r = got["fit_sums"], ref["fit_sums"]
    err = float(np.max(np.abs(g - r) / (np.abs(r) + 1e-300)))
    WORST["positive"] = max(WORST.get("positive", 0.0), err)
    print(what, "fit_sums max |gpu - ref| / |ref| =", err)
    assert np.all(np.abs(g - r) <= 1e-11 * np.abs(r) + 1e-12), what + "fit_sums"
    assert ("trait_sums" in got) == ("trait_sums" in ref) and ("trait_counts" in got) == ("trait_counts" in ref)
    if "trait_sums" not in ref:
        return
    assert np.array_equal(got["trait_counts"], ref["trait_counts"]), what + "trait_counts"
    g, r, b = got["trait_sums"], ref["trait_sums"], ref["trait_bounds"]
    for c in POSITIVE_TRAIT:
        err = float(np.max(np.abs(g[:, c] - r[:, c]) / (np.abs(r[:, c]) + 1e-300)))
        WORST["positive"] = max(WORST["positive"], err)
        print(what, "trait_sums[%d] max |gpu - ref| / |ref| =" % c, err)
        assert np.all(np.abs(g[:, c] - r[:, c]) <= 1e-11 * np.abs(r[:, c]) + 1e-12), what + "trait_sums[%d]" % c
    for c in SIGNED_TRAIT:
        err = float(np.max(np.abs(g[:, c] - r[:, c]) / np.maximum(b[:, c], 1e-300)))
        WORST["signed"] = max(WORST.get("signed", 0.0), err)
        print(what, "trait_sums[%d] max |gpu - ref| / B =" % c, err)
        assert np.all(np.abs(g[:, c] - r[:, c]) <= 1e-11 * b[:, c]), what + "trait_sums[%d]" % c
    print(what, "worst so far:", WORST)


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    return set(a) == set(b) and all(a[key][rows_a].tobytes() == b[key][rows_b].tobytes() for key in a)


@pytest.mark.parametrize("n,l,k", [(200, 64, 3), (1000, 40, 1), (1030, 33, 8), (4099, 24, 20), (2050, 16, 32), (700, 12, 33),
                                   (600, 8, 128)])
def test_parity_with_numpy(ts, n, l, k):
    with synth_engine(ts, n, l, k, 40 + k) as eng:
        rng = np.random.default_rng(k)
        locs = rng.permutation(l)[:max(3, l // 2)].astype(np.uint32)
        locs = np.concatenate([locs, locs[1:2], [l - 1]]).astype(np.uint32)  # unsorted, with a repeat (two when l - 1 was drawn)
        assert len(set(locs.tolist())) < len(locs)
        trait = make_trait(n, 90 + k)
        assert 0 < np.isnan(trait).sum() < n // 8
        assert_matches(eng.snp_scan(locs, trait), reference(eng, locs, trait), "list, trait ")
        assert_matches(eng.snp_scan(locs), reference(eng, locs), "list ")
        assert_matches(eng.snp_scan(trait=trait), reference(eng, np.arange(l), trait), "all, trait ")
        got = eng.snp_scan()
        assert set(got) == {"fit_sums", "fit_counts"}
        assert_matches(got, reference(eng, np.arange(l)), "all ")
        # a trait without a single value: the trait rows are exact zeros, the fit rows as ever
        none = eng.snp_scan(trait=np.full(n, np.nan))
        assert not none["trait_sums"].any() and not none["trait_counts"].any()
        assert np.array_equal(none["fit_counts"], got["fit_counts"])
        assert np.all(np.abs(none["fit_sums"] - got["fit_sums"]) <= 1e-11 * got["fit_sums"] + 1e-12)


def raw_call(eng, locs, trait, want):
    """tsamd_snp_scan with any subset of the four outputs; (rc, dict)"""
    from terastructure_amd import _lib
    from terastructure_amd.engine import _dp, _up

    a = None if locs is None else np.ascontiguousarray(locs, dtype=np.uint32)
    n_locs = eng.l if a is None else a.size
    t = None if trait is None else np.ascontiguousarray(trait, dtype=np.float64)
    out = dict(fit_sums=np.zeros((n_locs, _lib.SCAN_FIT_SUMS)), fit_counts=np.zeros((n_locs, _lib.SCAN_FIT_COUNTS), dtype=np.uint32),
               trait_sums=np.zeros((n_locs, _lib.SCAN_TRAIT_SUMS)), trait_counts=np.zeros(n_locs, dtype=np.uint32))
    ptr = {key: (None if key not in want else (_dp(v) if v.dtype == np.float64 else _up(v))) for key, v in out.items()}
    rc = eng.h.tsamd_snp_scan(eng.ctx, None if a is None else _up(a), n_locs, None if t is None else _dp(t), ptr["fit_sums"], ptr["fit_counts"],
                              ptr["trait_sums"], ptr["trait_counts"])
    return rc, {key: out[key] for key in want}


def test_a_locations_rows_do_not_depend_on_the_rest_of_the_call(ts, monkeypatch):
    n, l, k = 2050, 64, 8
    monkeypatch.delenv("TSAMD_TEST_SCAN_CHUNK", raising=False)
    monkeypatch.delenv("TSAMD_TEST_MAX_WORKGROUPS", raising=False)
    trait = make_trait(n, 4)
    with synth_engine(ts, n, l, k, 21, flags=ts.FLAG_TEST_HOOKS) as eng:
        state = eng.state_export()
        for tr in (trait, None):
            full, again = eng.snp_scan(trait=tr), eng.snp_scan(trait=tr)
            assert same_bits(full, again)
            for loc in (0, 13, 37, 63):
                alone = eng.snp_scan(np.array([loc], dtype=np.uint32), tr)
                assert same_bits(alone, full, rows_b=slice(loc, loc + 1)), loc
            listed = np.array([37, 2, 63, 37, 0], dtype=np.uint32)
            part = eng.snp_scan(listed, tr)
            for i, loc in enumerate(listed):
                assert same_bits(part, full, slice(i, i + 1), slice(int(loc), int(loc) + 1)), loc
            monkeypatch.setenv("TSAMD_TEST_SCAN_CHUNK", "5")  # 13 chunks, the last one of 4
            assert same_bits(eng.snp_scan(trait=tr), full)
            monkeypatch.delenv("TSAMD_TEST_SCAN_CHUNK")
            # each optional output alone is the same bits (a trait wants one of its own outputs beside a fit output)
            for key in full:
                rc, one = raw_call(eng, None, tr, [key] if tr is None or key.startswith("trait") else [key, "trait_counts"])
                assert rc == 0 and one[key].tobytes() == full[key].tobytes(), key
        # as on a device of four units: another segment count (the hook is read when the context is created)
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
        with synth_engine(ts, n, l, k, 21, flags=ts.FLAG_TEST_HOOKS, train=False) as small:
            small.state_import(*state)
            assert same_bits(small.snp_scan(trait=trait), eng.snp_scan(trait=trait))
            monkeypatch.setenv("TSAMD_TEST_SCAN_CHUNK", "5")
            assert same_bits(small.snp_scan(), eng.snp_scan())


def test_segments_and_tiles_on_a_small_shard(ts, monkeypatch):
    """three tiles and 600 locations: the real device cuts the list into segments, a two-unit one does not; same bits, and
    everything matches the reference"""
    n, l, k = 4099, 600, 8
    monkeypatch.delenv("TSAMD_TEST_MAX_WORKGROUPS", raising=False)
    monkeypatch.delenv("TSAMD_TEST_SCAN_CHUNK", raising=False)
    trait = make_trait(n, 6)
    with synth_engine(ts, n, l, k, 31, flags=ts.FLAG_TEST_HOOKS) as eng:
        state = eng.state_export()
        ref = reference(eng, np.arange(l), trait)
        wide = eng.snp_scan(trait=trait)
        assert_matches(wide, ref, "device ")
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "2")
        with synth_engine(ts, n, l, k, 31, flags=ts.FLAG_TEST_HOOKS, train=False) as small:
            small.state_import(*state)
            narrow = small.snp_scan(trait=trait)
        assert_matches(narrow, ref, "two units ")
        assert same_bits(narrow, wide)


def test_heldout_entries_leave_every_sum_and_count(ts):
    n, l, k = 1030, 12, 4
    trait = make_trait(n, 8)
    with synth_engine(ts, n, l, k, 7, train=False) as eng:
        rng = np.random.default_rng(3)
        for loc in range(l):
            eng.set_lambda(loc, rng.gamma(2.0, 1.0, size=(k, 2)) + 0.05)
        locs = np.array([2, 9, 5], dtype=np.uint32)
        before = eng.snp_scan(locs, trait)
        assert_matches(before, reference(eng, locs, trait), "before ")
        held = {}
        for loc in locs:
            y = unpack_bed(eng.download_bed(int(loc))[None, :], n)[0]
            held[int(loc)] = np.sort(rng.choice(np.nonzero(y != 3)[0], size=50, replace=False)).astype(np.uint32)
            eng.set_heldout(int(loc), held[int(loc)])
        after = eng.snp_scan(locs, trait)
        assert_matches(after, reference(eng, locs, trait), "after ")
        for i, loc in enumerate(locs):
            assert int(before["fit_counts"][i].sum()) == int(after["fit_counts"][i].sum()) + 50
            assert int(before["trait_counts"][i]) == int(after["trait_counts"][i]) + int((~np.isnan(trait[held[int(loc)]])).sum())
            assert np.all(after["fit_sums"][i] < before["fit_sums"][i])
        untouched = np.array([0, 11], dtype=np.uint32)
        assert_matches(eng.snp_scan(untouched, trait), reference(eng, untouched, trait), "other locations ")


def test_the_call_changes_no_state_in_any_launch_mode(ts):
    n, l, k = 1030, 40, 5
    head, tail = np.array([3, 8, 1], dtype=np.uint32), np.array([4, 4, 17, 0, 9, 33], dtype=np.uint32)
    trait = make_trait(n, 12)
    locs = np.array([5, 1, 1, 39], dtype=np.uint32)
    rows = []
    for mode in (ts.LAUNCH_PER_PASS, ts.LAUNCH_PER_SNP, ts.LAUNCH_PER_SCHEDULE):
        outs = []
        for call in (True, False):
            with synth_engine(ts, n, l, k, 23) as e:
                e.set_launch_mode(mode)
                e.run_schedule(head)  # ends in a training update: its gamma step is pending
                e.synchronize()
                if call:
                    s0, p0, h0, c0 = e.state_export(), e.total_passes(), e.pass_histogram(), e.get_counts()
                    got = e.snp_scan(locs, trait)
                    full = e.snp_scan()
                    s1 = e.state_export()
                    assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes(), mode
                    assert e.total_passes() == p0 and e.pass_histogram().tobytes() == h0.tobytes() and e.get_counts().tobytes() == c0.tobytes()
                    ref = reference(e, locs, trait)
                    assert_matches(got, ref, "mode %d " % mode)
                    assert_matches(full, reference(e, np.arange(l)), "mode %d, all " % mode)
                    rows.append((got, ref["trait_bounds"]))
                e.run_schedule(tail)  # applies the pending step: exactly as without the call
                e.run_schedule(tail[:2], 1)
                e.synchronize()
                outs.append(e.state_export())
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), mode
    # the three modes hold the same model up to the rounding of their own summation orders: the same rows within tolerance
    first, bounds = rows[0]
    for other, _ in rows[1:]:
        assert np.array_equal(other["fit_counts"], first["fit_counts"]) and np.array_equal(other["trait_counts"], first["trait_counts"])
        assert np.all(np.abs(other["fit_sums"] - first["fit_sums"]) <= 1e-11 * np.abs(first["fit_sums"]) + 1e-12)
        d = np.abs(other["trait_sums"] - first["trait_sums"])
        for c in POSITIVE_TRAIT:
            assert np.all(d[:, c] <= 1e-11 * np.abs(first["trait_sums"][:, c]) + 1e-12)
        for c in SIGNED_TRAIT:
            assert np.all(d[:, c] <= 1e-11 * bounds[:, c])


@pytest.mark.parametrize("world", [2, 3])
def test_shards_add_up_to_the_one_shard_answer(ts, world):
    n, l, k = 1030, 10, 6
    rng = np.random.default_rng(8)
    lam = rng.gamma(2.0, 1.0, size=(l, k, 2)) + 0.05
    locs = np.array([7, 0, 3, 3, 9], dtype=np.uint32)
    trait = make_trait(n, 14)
    engines = [synth_engine(ts, n, l, k, 17, train=False)] + [synth_engine(ts, n, l, k, 17, rank=r, world=world, train=False) for r in range(world)]
    try:
        for eng in engines:
            eng.set_lambda_range(lam)
        one = engines[0].snp_scan(locs, trait)
        ref = reference(engines[0], locs, trait)
        assert_matches(one, ref, "one shard ")
        assert sum(e.shard_count for e in engines[1:]) == n
        parts = [e.snp_scan(locs, trait[e.shard_begin:e.shard_begin + e.shard_count]) for e in engines[1:]]
        for e, p in zip(engines[1:], parts):  # every rank answers for its own shard
            assert_matches(p, reference(e, locs, trait[e.shard_begin:e.shard_begin + e.shard_count]), "rank %d " % e.rank)
        added = {key: np.sum([p[key] for p in parts], axis=0).astype(one[key].dtype) for key in one}
        assert_matches(added, ref, "%d shards added " % world)
        assert np.array_equal(added["fit_counts"], one["fit_counts"]) and np.array_equal(added["trait_counts"], one["trait_counts"])
        # ... and the statistics of the added rows are those of the one-shard rows up to that rounding
        za, zo = ts.scan_statistics(**added), ts.scan_statistics(**one)
        assert np.all(np.abs(za[:, 0::2] - zo[:, 0::2]) <= 1e-9)
    finally:
        for eng in engines:
            eng.close()


def test_bad_arguments_are_refused_and_the_state_is_untouched(ts):
    n, l, k = 200, 9, 2
    all4 = ["fit_sums", "fit_counts", "trait_sums", "trait_counts"]
    with synth_engine(ts, n, l, k, 2) as eng:
        s0 = eng.state_export()
        trait = make_trait(n, 1)
        with pytest.raises(ts.TsamdError) as e:
            eng.snp_scan(np.array([1, l], dtype=np.uint32))
        assert e.value.code == EINVAL and "locs[1]" in str(e.value)
        with pytest.raises(ts.TsamdError) as e:
            eng.snp_scan(np.array([], dtype=np.uint32))
        assert e.value.code == EINVAL and "n_locs" in str(e.value)
        rc, _ = raw_call(eng, None, trait, [])
        assert rc == EINVAL and "all NULL" in eng.last_error()
        for want in (["trait_sums"], ["trait_counts"], all4):
            rc, _ = raw_call(eng, None, None, want)
            assert rc == EINVAL and "without a trait" in eng.last_error(), want
        rc, _ = raw_call(eng, None, trait, ["fit_sums", "fit_counts"])
        assert rc == EINVAL and "both NULL" in eng.last_error()
        for bad in (np.inf, -np.inf):
            t = trait.copy()
            t[n - 1] = bad
            with pytest.raises(ts.TsamdError) as e:
                eng.snp_scan(trait=t)
            assert e.value.code == EINVAL and "trait[%d]" % (n - 1) in str(e.value)
        with pytest.raises(ValueError):
            eng.snp_scan(trait=trait[:-1])
        s1 = eng.state_export()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        rc, got = raw_call(eng, None, trait, all4)
        assert rc == 0
        assert_matches(got, reference(eng, np.arange(l), trait))


# -- calibration on true parameters -------------------------------------------------------------------------------------------

def windows(z, null, what):
    """the issue's conditions on the null locations of one z column"""
    v, m, top = float(np.var(z[null])), float(np.mean(z[null])), float(np.max(np.abs(z[null])))
    print(what, "variance %.3f mean %+.3f max |z| %.2f" % (v, m, top))
    assert 0.8 <= v <= 1.25, what
    assert abs(m) <= 0.15, what
    assert top < 6.0, what


def test_calibration_on_true_parameters(ts):
    """genotypes drawn from known theta and beta, the engine set to exactly those: under the model every z is N(0, 1) over the
    null locations; a planted effect and a column stripped of its heterozygotes stand out.  The same windows are asserted on
    the numpy reference from the engine's reads, so a failure of the data can be told from a failure of the kernel."""
    n, l, k = 2000, 1024, 3
    planted, stripped = 300, 700
    rng = np.random.default_rng(2026)
    theta = rng.dirichlet(np.full(k, 0.3), size=n)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    with ts.Engine(n, l, k) as eng:
        eng.synth_genotypes(theta, beta, seed=77, missing_rate=0.1)
        eng.set_gamma(np.maximum(theta, 1e-6) * 1e4)       # theta up to the floor (the setters refuse gamma below 1e-8)
        eng.set_lambda_range(1e3 * np.stack([beta, 1.0 - beta], axis=2))  # Ebeta = beta
        y = unpack_bed(eng.download_bed(planted)[None, :], n)[0]
        trait = rng.normal(0.0, 1.0, size=n) + 0.5 * np.where(y == 3, 0, y)
        trait[rng.random(n) < 0.05] = np.nan
        y = unpack_bed(eng.download_bed(stripped)[None, :], n)[0]
        het = np.nonzero(y == 1)[0]
        y[het] = np.where(rng.random(het.size) < 0.5, 0, 2)  # heterozygotes re-uploaded as homozygotes
        eng.upload_bed(pack_bed(y[None, :]), first_loc=stripped)
        got = eng.snp_scan(trait=trait)
        ref = reference(eng, np.arange(l), trait)
    assert_matches(got, ref, "calibration ")
    null = np.ones(l, dtype=bool)
    null[[planted, stripped]] = False
    for name, rows in (("kernel", got), ("numpy", {key: ref[key] for key in got})):
        z = ts.scan_statistics(**rows)
        assert np.all((z[:, 1::2] >= 0.0) & (z[:, 1::2] <= 1.0))
        for col, what in ((0, "z_het"), (2, "z_freq"), (4, "z_trait")):
            windows(z[:, col], null, name + " " + what)
        print(name, "planted z_trait %.2f, stripped z_het %.2f" % (z[planted, 4], z[stripped, 0]))
        assert z[planted, 4] > 6.0, name
        assert z[stripped, 0] < -10.0, name
