"""tsamd_train_loglik: the training-data log-likelihood per location and per individual, in one sweep of the listed columns.

The reference is numpy fp64 from three reads of the engine -- get_theta(), get_ebeta() and download_bed() (which shows
held-out entries as missing, as wanted) -- never from the call under test:
    term(n, j) = log(max(C(2,y) q^y (1-q)^(2-y), 1e-30)),  q = sum_k Ebeta[j][k] Etheta[n][k],  no term for code 01.

Tolerance, derived: every term is <= 0, so a sum's relative error is at most the accumulation error plus the per-term
error; for M <= 4 099 terms the first is M 2^-53 = 4.6e-13, the second a few ulp.  Asserted everywhere:
|gpu - ref| <= 1e-11 |ref| + 1e-12; counts exactly.

Shapes are the smallest at which a path can go wrong: one tile with padding, K = 1, N no multiple of 4 / 16 / 512, more
than one tile at every individuals-per-thread figure (16 / 8 / 4 / 2 at K <= 4 / 8 / 16 / 32), and the run-time-K kernel
at K = 33 and 128."""
import math

import numpy as np
import pytest

from helpers import init_gamma, pack_bed, unpack_bed
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1


def close(gpu, ref):
    gpu, ref = np.asarray(gpu, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(gpu - ref) <= 1e-11 * np.abs(ref) + 1e-12))


def synth_engine(ts, n, l, k, seed, flags=0, rank=0, world=1, train=True):
    """synthetic genotypes (10 % missing), seeded gamma, and -- on one shard -- a short schedule that ends in a training
    update: its gamma step is pending"""
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.full(k, 0.3), size=n)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    eng = ts.Engine(n, l, k, flags=flags, rank=rank, world=world)
    b, c = eng.shard_begin, eng.shard_count
    eng.synth_genotypes(theta[b:b + c], beta, seed=seed, missing_rate=0.1)
    eng.set_gamma(init_gamma(n, k, seed + 1)[b:b + c])
    if train:
        eng.run_schedule(rng.integers(0, l, size=6).astype(np.uint32))
        eng.run_schedule(np.array([l - 1, 0], dtype=np.uint32), 1)
        eng.run_schedule(np.array([1 % l, l // 2], dtype=np.uint32))
        eng.synchronize()
    return eng


def reference_terms(eng, locs):
    """{loc: (terms [shard_count] with 0 where there is none, ok [shard_count])}"""
    theta, eb, n = eng.get_theta(), eng.get_ebeta(), eng.shard_count
    out = {}
    for loc in sorted(set(int(x) for x in locs)):
        y = unpack_bed(eng.download_bed(loc)[None, :], n)[0]
        q = theta @ eb[loc]
        prod = np.where(y == 0, (1.0 - q) * (1.0 - q), np.where(y == 1, 2.0 * q * (1.0 - q), q * q))
        ok = y != 3
        out[loc] = (np.where(ok, np.log(np.maximum(prod, 1e-30)), 0.0), ok)
    return out


def reference(eng, locs):
    terms = reference_terms(eng, locs)
    n = eng.shard_count
    ref = dict(loc_sums=np.zeros(len(locs)), loc_counts=np.zeros(len(locs), dtype=np.uint64), indiv_sums=np.zeros(n),
               indiv_counts=np.zeros(n, dtype=np.uint64))
    for i, loc in enumerate(locs):
        t, ok = terms[int(loc)]
        ref["loc_sums"][i] = math.fsum(t)
        ref["loc_counts"][i] = ok.sum()
        ref["indiv_sums"] += t
        ref["indiv_counts"] += ok
    ref["sum"] = math.fsum(ref["loc_sums"])
    ref["count"] = int(ref["loc_counts"].sum())
    return ref


def assert_matches(got, ref, what=""):
    for key in ("loc_counts", "indiv_counts"):
        assert np.array_equal(got[key].astype(np.uint64), ref[key]), what + key
    assert got["count"] == ref["count"], what + "count"
    for key in ("loc_sums", "indiv_sums", "sum"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        print(what, key, "max |gpu - ref| / |ref| =", float(np.max(np.abs(g - r) / (np.abs(r) + 1e-300))))
        assert close(g, r), what + key
    assert np.all(got["loc_sums"] <= 0.0) and np.all(got["indiv_sums"] <= 0.0)


@pytest.mark.parametrize("n,l,k", [(200, 64, 3), (1000, 40, 1), (1030, 33, 8), (4099, 24, 20), (2050, 16, 32), (700, 12, 33),
                                   (600, 8, 128)])
def test_parity_with_numpy(ts, n, l, k):
    with synth_engine(ts, n, l, k, 40 + k) as eng:
        rng = np.random.default_rng(k)
        locs = rng.permutation(l)[:max(3, l // 2)].astype(np.uint32)
        locs = np.concatenate([locs, locs[1:2], [l - 1]]).astype(np.uint32)  # unsorted, with a repeat (two when l - 1 was drawn)
        assert len(set(locs.tolist())) < len(locs)
        assert_matches(eng.train_loglik(locs), reference(eng, locs), "list ")
        got = eng.train_loglik()
        assert_matches(got, reference(eng, np.arange(l)), "all ")
        # the optional outputs
        only = eng.train_loglik(per_loc=False, per_indiv=False)
        assert set(only) == {"sum", "count"} and only["sum"] == got["sum"] and only["count"] == got["count"]


def test_heldout_entries_move_from_the_training_sum_to_the_heldout_sum(ts):
    n, l, k = 1030, 12, 4
    with synth_engine(ts, n, l, k, 7, train=False) as eng:
        rng = np.random.default_rng(3)
        for loc in range(l):
            eng.set_lambda(loc, rng.gamma(2.0, 1.0, size=(k, 2)) + 0.05)
        locs = np.array([2, 9, 5], dtype=np.uint32)
        before = eng.train_loglik(locs)
        for loc in locs:
            y = unpack_bed(eng.download_bed(int(loc))[None, :], n)[0]
            eng.set_heldout(int(loc), np.sort(rng.choice(np.nonzero(y != 3)[0], size=50, replace=False)).astype(np.uint32))
        after = eng.train_loglik(locs)
        for i, loc in enumerate(locs):
            h, ch = eng.heldout_loglik(int(loc))
            a, b = before["loc_sums"][i], after["loc_sums"][i]
            assert ch == 50 and int(before["loc_counts"][i]) == int(after["loc_counts"][i]) + ch
            print("loc", loc, "A", a, "B + H", b + h, "rel", abs(a - (b + h)) / abs(a))
            assert abs(a - (b + h)) <= 1e-11 * abs(a)


def test_the_call_changes_no_state(ts):
    n, l, k = 1030, 20, 5
    tail = np.array([4, 4, 17, 0, 9], dtype=np.uint32)
    with synth_engine(ts, n, l, k, 11) as eng, synth_engine(ts, n, l, k, 11) as twin:
        s0, p0 = eng.state_export(), eng.total_passes()
        eng.train_loglik()
        eng.train_loglik(np.array([3, 1], dtype=np.uint32))
        s1 = eng.state_export()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        assert eng.total_passes() == p0
        for e in (eng, twin):  # the pending gamma step is still pending: the next schedule applies it in both alike
            e.run_schedule(tail)
            e.synchronize()
        a, b = eng.state_export(), twin.state_export()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_locations_sum_does_not_depend_on_the_rest_of_the_call(ts, monkeypatch):
    n, l, k = 2050, 64, 8
    monkeypatch.delenv("TSAMD_TEST_LOGLIK_CHUNK", raising=False)
    with synth_engine(ts, n, l, k, 21, flags=ts.FLAG_TEST_HOOKS) as eng:
        full = eng.train_loglik()
        again = eng.train_loglik()
        for key in ("loc_sums", "loc_counts", "indiv_sums", "indiv_counts"):
            assert full[key].tobytes() == again[key].tobytes(), key
        assert full["sum"] == again["sum"] and full["count"] == again["count"]
        for loc in (0, 13, 37, 63):
            alone = eng.train_loglik(np.array([loc], dtype=np.uint32))
            assert alone["loc_sums"].tobytes() == full["loc_sums"][loc:loc + 1].tobytes(), loc
            assert int(alone["loc_counts"][0]) == int(full["loc_counts"][loc])
        monkeypatch.setenv("TSAMD_TEST_LOGLIK_CHUNK", "5")  # 13 chunks, the last one of 4
        cut = eng.train_loglik()
        assert cut["loc_sums"].tobytes() == full["loc_sums"].tobytes()
        assert np.array_equal(cut["loc_counts"], full["loc_counts"]) and np.array_equal(cut["indiv_counts"], full["indiv_counts"])
        assert close(cut["indiv_sums"], full["indiv_sums"])  # (added chunk after chunk: another association)


def test_segments_and_tiles_on_a_small_shard(ts, monkeypatch):
    """three tiles: as on a two-unit device one segment covers the 600 locations, on the real one the grid also cuts them
    into segments; the per-location sums are the same bits, everything matches the reference"""
    n, l, k = 4099, 600, 8
    monkeypatch.delenv("TSAMD_TEST_MAX_WORKGROUPS", raising=False)
    with synth_engine(ts, n, l, k, 31, flags=ts.FLAG_TEST_HOOKS) as eng:
        state = eng.state_export()
        ref = reference(eng, np.arange(l))
        wide = eng.train_loglik()
        assert_matches(wide, ref, "device ")
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "2")
        with synth_engine(ts, n, l, k, 31, flags=ts.FLAG_TEST_HOOKS, train=False) as small:
            small.state_import(*state)
            narrow = small.train_loglik()
        assert_matches(narrow, ref, "two units ")
        assert narrow["loc_sums"].tobytes() == wide["loc_sums"].tobytes()


def test_clamp_and_extremes(ts):
    n, l, k = 530, 6, 3
    with synth_engine(ts, n, l, k, 5, train=False) as eng:
        y = np.full((4, n), 3, dtype=np.uint8)
        y[0, 17] = 2      # location 0: one individual, y = 2, q = 1e-18: the product 1e-36 is clamped
        y[1, :] = 2       # location 1: everybody
        y[2, 400] = 0     # location 2: y = 0 at q = 1: (1 - q)^2 is clamped
        eng.upload_bed(pack_bed(y))  # location 3: all missing
        tiny, one = np.full(k, 1e-18), np.ones(k)
        eng.set_lambda(0, np.stack([tiny, one], axis=1))
        eng.set_lambda(1, np.stack([tiny, one], axis=1))
        eng.set_lambda(2, np.stack([one, tiny], axis=1))
        got = eng.train_loglik()
        floor = math.log(1e-30)
        assert [int(c) for c in got["loc_counts"][:4]] == [1, n, 1, 0]
        assert abs(got["loc_sums"][0] - floor) <= 2 * np.spacing(abs(floor))  # (the device log's own rounding)
        assert abs(got["loc_sums"][2] - floor) <= 2 * np.spacing(abs(floor))
        assert close(got["loc_sums"][1], n * floor)
        assert got["loc_sums"][3] == 0.0
        assert_matches(got, reference(eng, np.arange(l)))
        g = init_gamma(n, k, 9)
        g[::7] = 1e-8  # the smallest gamma the setters take
        g[3, 1:] = 1e-8
        eng.set_gamma(g)
        got = eng.train_loglik()
        assert np.all(np.isfinite(got["loc_sums"])) and np.all(np.isfinite(got["indiv_sums"])) and math.isfinite(got["sum"])
        assert_matches(got, reference(eng, np.arange(l)), "tiny gamma ")


def test_bad_arguments_are_refused_and_the_context_stays_usable(ts):
    n, l, k = 200, 9, 2
    with synth_engine(ts, n, l, k, 2, train=False) as eng:
        with pytest.raises(ts.TsamdError) as e:
            eng.train_loglik(np.array([1, l], dtype=np.uint32))
        assert e.value.code == EINVAL and "locs[1]" in str(e.value)
        with pytest.raises(ts.TsamdError) as e:
            eng.train_loglik(np.array([], dtype=np.uint32))
        assert e.value.code == EINVAL and "n_locs" in str(e.value)
        assert_matches(eng.train_loglik(), reference(eng, np.arange(l)))


def test_two_shards_add_up_to_the_one_shard_answer(ts):
    n, l, k = 1030, 10, 6
    rng = np.random.default_rng(8)
    lam = rng.gamma(2.0, 1.0, size=(l, k, 2)) + 0.05
    locs = np.array([7, 0, 3, 3, 9], dtype=np.uint32)
    engines = [synth_engine(ts, n, l, k, 17, train=False)] + [synth_engine(ts, n, l, k, 17, rank=r, world=2, train=False) for r in (0, 1)]
    try:
        for eng in engines:
            for loc in range(l):
                eng.set_lambda(loc, lam[loc])
        one, a, b = [eng.train_loglik(locs) for eng in engines]
        assert_matches(one, reference(engines[0], locs), "one shard ")
        assert engines[1].shard_count + engines[2].shard_count == n
        assert close(np.concatenate([a["indiv_sums"], b["indiv_sums"]]), one["indiv_sums"])
        assert np.array_equal(np.concatenate([a["indiv_counts"], b["indiv_counts"]]), one["indiv_counts"])
        assert np.array_equal(a["loc_counts"] + b["loc_counts"], one["loc_counts"])
        assert close(a["loc_sums"] + b["loc_sums"], one["loc_sums"])
        assert a["count"] + b["count"] == one["count"] and close(a["sum"] + b["sum"], one["sum"])
    finally:
        for eng in engines:
            eng.close()
