"""tsamd_kinship: admixture-adjusted relatedness (REAP) of listed individuals on the matrix cores.

The reference is numpy fp64 from reads of the engine only -- get_theta(), get_ebeta() and download_bed() (which shows
held-out entries as missing, as wanted):
    q = theta[n] . Ebeta[j],  r = y - 2q,  s = sqrt(q (1 - q)),  both 0 where the stored code is 01
    num = R R^T,  den = S S^T,  kin = num / (4 den)  (0 where den == 0)

Tolerances: |num - ref| <= 1e-11 sum_j |r_a r_b| and the same for den (its terms are all positive) -- about ten times the
worst-order summation bound (n_locs + 2 K + 10) 2^-53 at these sizes; kin to relative 1e-9 where |kin| > 1e-3; other
geometries (chunks, segments, a four-unit device) and the two-shard context against the default to 1e-12 of sum |terms|;
symmetry, repeatability, kin == NULL and the untouched state bit for bit.
Largest errors observed on one MI355X (2026-10-19), as multiples of sum |terms|: 1.5e-13 for num (K = 33; 4.0e-15 at K <= 32),
1.2e-15 for den, relative 3.8e-13 for kin; other geometries against the default 1.2e-15; rank 1 of two shards 0 (the same bits).

Shapes: the listed counts m = 1, 63, 65, 200, 130, 70, 70, 66 give one tile, a tile that ends in padding, and 2 to 4 tiles of
64 (diagonal and off-diagonal tile pairs with a ragged last tile: with random data a transposed or mis-rowed read-out of the
MFMA accumulators cannot pass); k = 1 .. 32 run the specialised residual kernels, 33 and 128 the run-time-K one; n_locs =
1 and 3 leave a k-step of 4 locations partly empty.

Relatives: 60 unrelated PSD individuals at K = 3 and L = 4096 with 10 % missing, a duplicate of one of them and a child of
two.  The bounds are multiples of sd0 = 1 / (2 sqrt(0.81 L)) = 0.0087, the spread of an unrelated pair's estimate when
both are observed at 81 % of the locations: unrelated pairs within 5 sd0 of 0 (the numpy reference alone: 3.6, their sd
0.99 sd0), self and duplicate within 5 sd0 of 0.5 (reference: 2.8 at most), parent and child within 5 sd0 of 0.25
(reference: 2.5); seeds 6 to 8 of the same sample pass alike."""
import ctypes as C

import numpy as np
import pytest

from helpers import init_gamma, pack_bed, unpack_bed
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(700, 37, 3, 1), (700, 130, 8, 63), (1030, 33, 8, 65), (2100, 64, 1, 200), (1030, 24, 20, 130), (700, 16, 32, 70), (700, 12, 33, 70),
          (600, 8, 128, 66)]


def trained_lambda(rng, beta):
    """lambda as after training: 1 + c beta, 1 + c (1 - beta) with a per-location c in (0, 200)"""
    c = rng.uniform(0.0, 200.0, size=(beta.shape[0], 1))
    return np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2)


def synth_engine(ts, n, l, k, seed, flags=0, rank=0, world=1, held=True):
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.full(k, 0.3), size=n)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    eng = ts.Engine(n, l, k, flags=flags, rank=rank, world=world)
    b, c = eng.shard_begin, eng.shard_count
    eng.synth_genotypes(theta[b:b + c], beta, seed=seed, missing_rate=0.1)
    eng.set_lambda_range(trained_lambda(rng, beta))
    eng.set_gamma(init_gamma(n, k, seed + 1)[b:b + c])
    if held:  # a held-out fold: global ids, every third individual at two locations
        for loc in sorted({0, l - 1}):
            eng.set_heldout(loc, np.arange(loc % 3, n, 3, dtype=np.uint32))
    return eng


def kin_reference(theta, eb, y):
    """dict(num, den, kin, absn) from theta [m][k], Ebeta [J][k] and genotypes y [m][J] in {0, 1, 2, 3 = no term}"""
    q = theta @ eb.T
    ok = y != 3
    r = np.where(ok, y.astype(np.float64) - 2.0 * q, 0.0)
    s = np.where(ok, np.sqrt(q * (1.0 - q)), 0.0)
    num, den, absn = r @ r.T, s @ s.T, np.abs(r) @ np.abs(r).T
    with np.errstate(divide="ignore", invalid="ignore"):
        kin = np.where(den != 0.0, num / (4.0 * den), 0.0)
    return dict(num=num, den=den, kin=kin, absn=absn)


def reference(eng, indivs, locs):
    locs = np.arange(eng.l) if locs is None else np.asarray(locs, dtype=np.int64)
    rows = np.arange(eng.shard_count) if indivs is None else np.asarray(indivs, dtype=np.int64) - eng.shard_begin
    cols = {int(x): unpack_bed(eng.download_bed(int(x))[None, :], eng.shard_count)[0] for x in set(locs.tolist())}
    y = np.stack([cols[int(x)] for x in locs], axis=1)[rows]  # [m][J]
    return kin_reference(eng.get_theta()[rows], eng.get_ebeta()[locs], y)


def assert_matches(got, ref, what=""):
    kin, num, den = got
    en = float(np.max(np.abs(num - ref["num"]) / np.where(ref["absn"] > 0, ref["absn"], 1.0)))
    ed = float(np.max(np.abs(den - ref["den"]) / np.where(ref["den"] > 0, ref["den"], 1.0)))
    big = np.abs(ref["kin"]) > 1e-3
    ek = float(np.max(np.abs(kin - ref["kin"])[big] / np.abs(ref["kin"])[big])) if big.any() else 0.0
    print(f"{what}max |num - ref| / sum |r r| = {en:.3e}, |den - ref| / den = {ed:.3e}, rel kin = {ek:.3e}")
    assert np.all(np.abs(num - ref["num"]) <= 1e-11 * ref["absn"])
    assert np.all(np.abs(den - ref["den"]) <= 1e-11 * ref["den"])
    assert ek <= 1e-9
    assert np.all(kin[ref["den"] == 0.0] == 0.0)
    for a in got:
        assert a.tobytes() == np.ascontiguousarray(a.T).tobytes()  # exactly symmetric


def assert_close(a, b, scale, bound=1e-12):
    e = float(np.max(np.abs(a - b) / np.where(scale > 0, scale, 1.0)))
    assert np.all(np.abs(a - b) <= bound * scale), e
    return e


def pick_ids(rng, eng, m):
    """m global ids of the engine's shard: random, unsorted, the last one a repeat of the first"""
    ids = eng.shard_begin + rng.choice(eng.shard_count, size=max(1, m - 1), replace=False)
    return (np.concatenate([ids, ids[:1]]) if m > 1 else ids).astype(np.uint32)


def pick_locs(rng, l):
    locs = rng.permutation(l)[:max(3, l // 2)]
    return np.concatenate([locs, locs[1:2], [l - 1]]).astype(np.uint32)  # unsorted, with a repeat


def raw_call(eng, ids, locs, want_kin=True, want_num=True, want_den=True):
    """tsamd_kinship itself, any output NULL: (rc, kin, num, den)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    m = ids.size
    out = [np.zeros((m, m)) if w else None for w in (want_kin, want_num, want_den)]
    dp = C.POINTER(C.c_double)
    rc = eng.h.tsamd_kinship(eng.ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)), m, locs.ctypes.data_as(C.POINTER(C.c_uint32)), locs.size,
                             *[None if a is None else a.ctypes.data_as(dp) for a in out])
    return (rc, *out)


@pytest.mark.parametrize("n,l,k,m", SHAPES)
def test_parity_with_numpy(ts, n, l, k, m):
    with synth_engine(ts, n, l, k, 40 + k + m) as eng:
        rng = np.random.default_rng(m)
        ids, locs = pick_ids(rng, eng, m), pick_locs(rng, l)
        assert m == 1 or len(set(ids.tolist())) < len(ids)
        assert len(set(locs.tolist())) < len(locs)
        for which in (locs, None):
            got = eng.kinship(ids, which, parts=True)
            assert got[0].shape == (m, m)
            assert_matches(got, reference(eng, ids, which), f"N={n} L={l} K={k} m={m} {'list' if which is not None else 'all'}: ")
            assert eng.kinship(ids, which).tobytes() == got[0].tobytes()
        if m > 1:  # a repeated id is a row of its own: the same values as its first appearance, the pair a duplicate
            assert got[1][-1, :-1].tobytes() == got[1][0, :-1].tobytes() and got[1][-1, -1] == got[1][0, 0] == got[1][0, -1]


def test_the_whole_shard_and_short_lists_of_locations(ts):
    """indivs == None: all 700 individuals, 11 tiles and 66 tile pairs; n_locs = 1 and 3: a k-step with 3 and 1 empty slots,
    from lists and as contexts of l = 1 and l = 3"""
    with synth_engine(ts, 700, 37, 3, 7) as eng:
        for locs in (np.array([5], dtype=np.uint32), np.array([36, 0, 9], dtype=np.uint32), None):
            got = eng.kinship(None, locs, parts=True)
            assert got[0].shape == (700, 700)
            assert_matches(got, reference(eng, None, locs), f"whole shard, {'all' if locs is None else len(locs)} locations: ")
    for l in (1, 3):
        with synth_engine(ts, 700, l, 3, 70 + l) as eng:
            ids = pick_ids(np.random.default_rng(l), eng, 130)
            assert_matches(eng.kinship(ids, parts=True), reference(eng, ids, None), f"l = {l}: ")


def test_repeatable_and_the_same_with_kin_null(ts):
    with synth_engine(ts, 1030, 50, 8, 3) as eng:
        rng = np.random.default_rng(1)
        ids, locs = pick_ids(rng, eng, 150), pick_locs(rng, 50)
        a, b = eng.kinship(ids, locs, parts=True), eng.kinship(ids, locs, parts=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        rc, _, num, den = raw_call(eng, ids, locs, want_kin=False)
        assert rc == 0 and num.tobytes() == a[1].tobytes() and den.tobytes() == a[2].tobytes()
        rc, kin, _, _ = raw_call(eng, ids, locs, want_num=False, want_den=False)
        assert rc == 0 and kin.tobytes() == a[0].tobytes()


def test_the_call_changes_no_state_in_any_launch_mode(ts):
    n, l, k = 1030, 40, 5
    head, tail = np.array([3, 8, 1], dtype=np.uint32), np.array([4, 4, 17, 0, 9, 33], dtype=np.uint32)
    ids = np.array([5, 900, 17, 5, 64], dtype=np.uint32)
    for mode in (ts.LAUNCH_PER_PASS, ts.LAUNCH_PER_SNP, ts.LAUNCH_PER_SCHEDULE):
        outs = []
        for call in (True, False):
            with synth_engine(ts, n, l, k, 23) as e:
                e.set_launch_mode(mode)
                e.run_schedule(head)  # ends in a training update: its gamma step is pending
                e.synchronize()
                if call:
                    s0, p0, h0, c0 = e.state_export(), e.total_passes(), e.pass_histogram(), e.get_counts()
                    e.kinship(ids, np.array([5, 1, 1, 39], dtype=np.uint32))
                    e.kinship()
                    s1 = e.state_export()
                    assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes(), mode
                    assert e.total_passes() == p0 and e.pass_histogram().tobytes() == h0.tobytes() and e.get_counts().tobytes() == c0.tobytes()
                e.run_schedule(tail)  # applies the pending step: exactly as without the call
                e.run_schedule(tail[:2], 1)
                e.synchronize()
                outs.append(e.state_export())
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), mode


def test_other_geometries_agree(ts, monkeypatch):
    """chunks of 1 and 5 locations (130 and 26 chunks, tails of 3 and 3 empty slots), 1 and 3 segments against the device's
    choice, and the geometry of a four-unit device: the same sums in another association"""
    n, l, k, m = 700, 130, 8, 130
    for var in ("TSAMD_TEST_KIN_CHUNK", "TSAMD_TEST_KIN_SEGMENTS", "TSAMD_TEST_MAX_WORKGROUPS"):
        monkeypatch.delenv(var, raising=False)
    with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as eng:
        ids = pick_ids(np.random.default_rng(2), eng, m)
        ref = reference(eng, ids, None)
        base = eng.kinship(ids, parts=True)
        assert_matches(base, ref, "device: ")
        for var, values in (("TSAMD_TEST_KIN_CHUNK", ("1", "5")), ("TSAMD_TEST_KIN_SEGMENTS", ("1", "3"))):
            for v in values:
                monkeypatch.setenv(var, v)
                got = eng.kinship(ids, parts=True)
                e = max(assert_close(got[1], base[1], ref["absn"]), assert_close(got[2], base[2], ref["den"]))
                print(f"{var}={v}: max |difference| / sum |terms| = {e:.3e}")
                assert_matches(got, ref, f"{var}={v}: ")
            monkeypatch.delenv(var)
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
        with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as small:  # (the same seed: the same state)
            assert small.state_export()[0].tobytes() == eng.state_export()[0].tobytes()
            got = small.kinship(ids, parts=True)
        e = max(assert_close(got[1], base[1], ref["absn"]), assert_close(got[2], base[2], ref["den"]))
        print(f"four units: max |difference| / sum |terms| = {e:.3e}")
        assert_matches(got, ref, "four units: ")


def test_a_shard_answers_for_global_ids(ts):
    n, l, k = 1030, 33, 6
    with synth_engine(ts, n, l, k, 17) as one, synth_engine(ts, n, l, k, 17, rank=1, world=2) as shard:
        assert shard.shard_begin > 0 and shard.shard_begin + shard.shard_count == n
        ids = pick_ids(np.random.default_rng(3), shard, 100)
        assert ids.min() >= shard.shard_begin
        a, b = one.kinship(ids, parts=True), shard.kinship(ids, parts=True)
        ref = reference(shard, ids, None)
        e = max(assert_close(b[1], a[1], ref["absn"]), assert_close(b[2], a[2], ref["den"]))
        print(f"rank 1 of 2 against one context: max |difference| / sum |terms| = {e:.3e}")
        assert_matches(b, ref, "rank 1 of 2: ")
        with pytest.raises(ts.TsamdError) as err:  # an id of the other shard
            shard.kinship(np.array([ids[0], 0], dtype=np.uint32))
        assert err.value.code == EINVAL and "indivs[1]" in str(err.value)


def test_bad_arguments_are_refused_and_the_context_stays_usable(ts):
    n, l, k = 200, 9, 2
    with synth_engine(ts, n, l, k, 2) as eng:
        s0 = eng.state_export()
        some, all_locs = np.array([3, 1], dtype=np.uint32), np.arange(l, dtype=np.uint32)
        for kwargs, word in ((dict(indivs=np.array([], dtype=np.uint32)), "m must be positive"),
                             (dict(indivs=np.zeros(ts._lib.KIN_MAX_M + 1, dtype=np.uint32)), "TSAMD_KIN_MAX_M"),
                             (dict(indivs=some, locs=np.array([], dtype=np.uint32)), "n_locs"),
                             (dict(indivs=some, locs=np.array([1, l], dtype=np.uint32)), "locs[1]"),
                             (dict(indivs=np.array([3, n], dtype=np.uint32)), "indivs[1]")):
            with pytest.raises(ts.TsamdError) as e:
                eng.kinship(**kwargs)
            assert e.value.code == EINVAL and word in str(e.value), kwargs
        rc, *_ = raw_call(eng, some, all_locs, want_kin=False, want_num=False, want_den=False)
        assert rc == EINVAL and "all NULL" in eng.last_error()
        dp = C.POINTER(C.c_double)
        one = np.zeros((1, 1))
        assert eng.h.tsamd_kinship(eng.ctx, None, n + 1, None, l, one.ctypes.data_as(dp), None, None) == EINVAL  # (NULL: the first m of 200)
        assert eng.h.tsamd_kinship(eng.ctx, None, 1, None, l + 1, one.ctypes.data_as(dp), None, None) == EINVAL  # (NULL: locations 0 .. n_locs-1)
        s1 = eng.state_export()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        assert_matches(eng.kinship(some, parts=True), reference(eng, some, None))
        assert eng.kinship(some, all_locs).tobytes() == eng.kinship(some).tobytes()


def relatives(seed=5, n0=60, l=4096, k=3, missing=0.1):
    """(y [n0 + 2][l] in {0, 1, 2, 3 = missing}, theta, beta): n0 unrelated PSD individuals, then a duplicate of individual 0
    (missing on its own) and a child of individuals 1 and 2"""
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.full(k, 0.5), size=n0)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    p = theta @ beta.T  # [n0][l]
    g = (rng.random((n0, l)) < p).astype(np.uint8) + (rng.random((n0, l)) < p).astype(np.uint8)
    child = (rng.random(l) < g[1] / 2.0).astype(np.uint8) + (rng.random(l) < g[2] / 2.0).astype(np.uint8)  # one allele of each parent
    y = np.concatenate([g, g[:1], child[None, :]])
    theta = np.concatenate([theta, theta[:1], 0.5 * (theta[1:2] + theta[2:3])])
    y[rng.random(y.shape) < missing] = 3
    return y, theta, beta


def check_relatives(kin, n0, l):
    """the estimator's own claims, on any [n0 + 2]^2 kinship matrix of the relatives() sample; returns the figures"""
    sd0 = 1.0 / (2.0 * np.sqrt(0.81 * l))
    iu = np.triu_indices(n0, 1)
    unrelated, selfs = kin[:n0, :n0][iu], np.diag(kin)
    out = dict(sd0=sd0, unrelated_mean=float(unrelated.mean()), unrelated_sd=float(unrelated.std()), unrelated_max=float(np.abs(unrelated).max()),
               self_mean=float(selfs.mean()), self_worst=float(np.abs(selfs - 0.5).max()), duplicate=float(kin[n0, 0]),
               child=(float(kin[n0 + 1, 1]), float(kin[n0 + 1, 2])))
    assert out["unrelated_max"] <= 5 * sd0 and abs(out["unrelated_mean"]) <= sd0 / 5
    assert 0.8 * sd0 <= out["unrelated_sd"] <= 1.25 * sd0
    assert out["self_worst"] <= 5 * sd0 and abs(out["duplicate"] - 0.5) <= 5 * sd0
    assert all(abs(c - 0.25) <= 5 * sd0 for c in out["child"])
    others = np.concatenate([kin[n0, 1:n0], kin[n0 + 1, 3:n0], kin[n0 + 1, :1]])  # the duplicate and the child against everybody else
    assert np.abs(others).max() <= 5 * sd0
    return out


def test_relatives_are_found(ts):
    n0, l, k = 60, 4096, 3
    y, theta, beta = relatives(n0=n0, l=l, k=k)
    n = n0 + 2
    with ts.Engine(n, l, k) as eng:
        eng.upload_bed(pack_bed(np.ascontiguousarray(y.T)))
        eng.set_gamma(100.0 * theta + 1e-6)
        eng.set_lambda_range(np.stack([1000.0 * beta, 1000.0 * (1.0 - beta)], axis=2))
        got = eng.kinship(parts=True)
        ref = reference(eng, None, None)
    assert_matches(got, ref, "relatives: ")
    print(check_relatives(ref["kin"], n0, l))
    check_relatives(got[0], n0, l)
