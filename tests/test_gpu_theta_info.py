"""tsamd_theta_info / tsamd_theta_se: the information matrices of theta on the matrix cores, and its standard errors.

The reference is numpy fp64 from reads of the engine only -- get_theta(), get_ebeta() and download_bed() (which shows held-out
entries as missing, as wanted):
    q = theta[n] . Ebeta[j],  c_obs = y / q^2 + (2 - y) / (1 - q)^2,  c_exp = 2 / (q (1 - q)),  both 0 where the stored code is 01
    H[n][(a <= b)] = sum_j c(n, j) Ebeta[j][a] Ebeta[j][b]

Tolerance: |H - ref| <= 1e-11 ref entrywise -- every term is positive, and this is the margin tsamd_kinship uses for its
positive-term product, about ten times the worst-order summation bound at these sizes.  Other geometries (chunks, blocks, a
four-unit device), additivity over location lists and the two-shard context against the default to 1e-12 H; repeatability, the
repeated id, a permuted list and the untouched state bit for bit.
Largest errors observed on one MI355X (2026-10-21), as multiples of ref: 1.9e-15 over the shapes (K = 128; 1.3e-15 at most at
every other K); other geometries against the default 1.3e-15 (chunks of 1 location), additivity 4.2e-16, rank 1 of two shards 0
(the same bits).  Calibration on the device, seed 6: sd / mean se = (0.996, 1.075, 1.004), coverage 0.932, for both kinds of
information -- the figures of the numpy reference.

Shapes: the listed counts m = 1, 63, 65, 200, 130, 70, 70, 66 give one tile, a tile that ends in padding, and 2 to 4 ragged
tiles of 64 individuals; k = 3, 8, 8, 1, 11, 32, 33, 128 give P = 6, 36, 36, 1, 66 (two column tiles), 528, 561 and 8256 packed
columns and run the specialised and the run-time-K coefficient kernel; n = 1030 covers the word that straddles a column's end.
With random data and ragged tiles a transposed or mis-rowed read-out of the MFMA accumulators cannot pass.

Calibration: the CPU fixture of theta_info_refs (seed 6) on the device, within the same two bands."""
import ctypes as C

import numpy as np
import pytest

import theta_info_refs as tr
from helpers import pack_bed, unpack_bed
from test_gpu_kinship import pick_ids, pick_locs, synth_engine
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(700, 37, 3, 1), (700, 130, 8, 63), (1030, 33, 8, 65), (2100, 64, 1, 200), (1030, 24, 11, 130), (700, 16, 32, 70), (700, 12, 33, 70),
          (600, 8, 128, 66)]
HOOKS = ("TSAMD_TEST_INFO_CHUNK", "TSAMD_TEST_INFO_BLOCK", "TSAMD_TEST_MAX_WORKGROUPS")


def genotypes(eng, rows, locs):
    cols = {int(x): unpack_bed(eng.download_bed(int(x))[None, :], eng.shard_count)[0] for x in set(locs.tolist())}
    return np.stack([cols[int(x)] for x in locs], axis=1)[rows]  # [m][J]


def reference(eng, indivs, locs):
    locs = np.arange(eng.l) if locs is None else np.asarray(locs, dtype=np.int64)
    rows = np.arange(eng.shard_count) if indivs is None else np.asarray(indivs, dtype=np.int64) - eng.shard_begin
    return tr.info_fp64(eng.get_theta()[rows], eng.get_ebeta()[locs], genotypes(eng, rows, locs))


def assert_matches(got, ref, what="", bound=1e-11):
    worst = 0.0
    for key in ("obs", "exp"):
        g, r = got[key], ref[key]
        assert g.shape == r.shape and np.all(r >= 0.0)
        worst = max(worst, float(np.max(np.abs(g - r) / np.where(r > 0, r, 1.0))))
        assert np.all(np.abs(g - r) <= bound * r), (what, key, worst)
    print(f"{what}max |H - ref| / ref = {worst:.3e}")
    return worst


def assert_close(a, b, bound=1e-12):
    worst = 0.0
    for key in ("obs", "exp"):
        scale = np.abs(b[key])
        worst = max(worst, float(np.max(np.abs(a[key] - b[key]) / np.where(scale > 0, scale, 1.0))))
        assert np.all(np.abs(a[key] - b[key]) <= bound * scale), (key, worst)
    return worst


def same_bits(a, b):
    return all(a[key].tobytes() == b[key].tobytes() for key in ("obs", "exp"))


def raw_call(eng, ids, locs, want_obs=True, want_exp=True, m=None, n_locs=None):
    """tsamd_theta_info itself, any output NULL: (rc, obs, exp)"""
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    locs = None if locs is None else np.ascontiguousarray(locs, dtype=np.uint32)
    m = ids.size if m is None else m
    n_locs = locs.size if n_locs is None else n_locs
    P = eng.k * (eng.k + 1) // 2
    out = [np.zeros((max(m, 1), P)) if w else None for w in (want_obs, want_exp)]
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    rc = eng.h.tsamd_theta_info(eng.ctx, None if ids is None else ids.ctypes.data_as(up), m, None if locs is None else locs.ctypes.data_as(up), n_locs,
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
            got = eng.theta_info(ids, which)
            assert got["obs"].shape == got["exp"].shape == (m, k * (k + 1) // 2)
            assert_matches(got, reference(eng, ids, which), f"N={n} L={l} K={k} m={m} {'list' if which is not None else 'all'}: ")
        if m > 1:  # a repeated id is a row of its own, the same bits as its first appearance
            assert got["obs"][-1].tobytes() == got["obs"][0].tobytes() and got["exp"][-1].tobytes() == got["exp"][0].tobytes()
        u = ts.info_unpack(got["obs"], k)
        assert u.shape == (m, k, k) and u.tobytes() == np.ascontiguousarray(u.transpose(0, 2, 1)).tobytes()
        assert u[:, 0, k - 1].tobytes() == got["obs"][:, k - 1].tobytes() and u[:, k - 1, k - 1].tobytes() == got["obs"][:, -1].tobytes()


def test_the_whole_shard_and_short_lists_of_locations(ts):
    """indivs == None: the contiguous path, all 1030 individuals in 17 tiles, the last column word straddling the column's end;
    n_locs = 1 and 3: a k-step with 3 and 1 empty slots, from lists and as contexts of l = 1 and l = 3"""
    with synth_engine(ts, 1030, 37, 3, 7) as eng:
        for locs in (np.array([5], dtype=np.uint32), np.array([36, 0, 9], dtype=np.uint32), None):
            got = eng.theta_info(None, locs)
            assert got["obs"].shape == (1030, 6)
            assert_matches(got, reference(eng, None, locs), f"whole shard, {'all' if locs is None else len(locs)} locations: ")
        # the first m of the shard (indivs == NULL, m < the shard) and the same ids listed: two paths to the columns, the same bits
        rc, obs, exp = raw_call(eng, None, None, m=333, n_locs=37)
        assert rc == 0
        listed = eng.theta_info(np.arange(333, dtype=np.uint32), None)
        assert obs.tobytes() == listed["obs"].tobytes() and exp.tobytes() == listed["exp"].tobytes()
    for l in (1, 3):
        with synth_engine(ts, 700, l, 3, 70 + l) as eng:
            ids = pick_ids(np.random.default_rng(l), eng, 130)
            assert_matches(eng.theta_info(ids), reference(eng, ids, None), f"l = {l}: ")


def test_repeatable_permutable_and_either_output_null(ts):
    with synth_engine(ts, 1030, 50, 8, 3) as eng:
        rng = np.random.default_rng(1)
        ids, locs = pick_ids(rng, eng, 150), pick_locs(rng, 50)
        a, b = eng.theta_info(ids, locs), eng.theta_info(ids, locs)
        assert same_bits(a, b)
        perm = rng.permutation(ids.size)  # a list of the same length: every row the same bits wherever it stands
        c = eng.theta_info(ids[perm], locs)
        assert c["obs"].tobytes() == a["obs"][perm].tobytes() and c["exp"].tobytes() == a["exp"][perm].tobytes()
        rc, obs, none = raw_call(eng, ids, locs, want_exp=False)
        assert rc == 0 and none is None and obs.tobytes() == a["obs"].tobytes()
        rc, none, exp = raw_call(eng, ids, locs, want_obs=False)
        assert rc == 0 and none is None and exp.tobytes() == a["exp"].tobytes()
        rc, *_ = raw_call(eng, ids, locs, want_obs=False, want_exp=False)
        assert rc == EINVAL and "both NULL" in eng.last_error()


def test_the_call_changes_no_state_and_a_pending_step_stays_pending(ts):
    n, l, k = 1030, 40, 5
    head, tail = np.array([3, 8, 1], dtype=np.uint32), np.array([4, 4, 17, 0, 9, 33], dtype=np.uint32)
    ids = np.array([5, 900, 17, 5, 64], dtype=np.uint32)
    outs = []
    for call in (True, False):
        with synth_engine(ts, n, l, k, 23) as e:
            e.run_schedule(head)  # ends in a training update: its gamma step is pending
            e.synchronize()
            if call:
                s0, p0, h0, c0 = e.state_export(), e.total_passes(), e.pass_histogram(), e.get_counts()
                e.theta_info(ids, np.array([5, 1, 1, 39], dtype=np.uint32))
                e.theta_info()
                s1 = e.state_export()
                assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
                assert e.total_passes() == p0 and e.pass_histogram().tobytes() == h0.tobytes() and e.get_counts().tobytes() == c0.tobytes()
            e.run_schedule(tail)  # applies the pending step: exactly as without the call
            e.run_schedule(tail[:2], 1)
            e.synchronize()
            outs.append(e.state_export())
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


def test_other_geometries_and_additivity(ts, monkeypatch):
    """chunks of 8 locations (17 chunks, the last of 2 with half a k-step empty), blocks of 64 and of 20 individuals (a block that
    starts off a multiple of 16 on the contiguous path), the geometry of a four-unit device: the same sums in another
    association; and H(A) + H(B) = H(A || B)"""
    n, l, k, m = 700, 130, 8, 130
    for var in HOOKS:
        monkeypatch.delenv(var, raising=False)
    with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as eng:
        ids = pick_ids(np.random.default_rng(2), eng, m)
        ref, ref_all = reference(eng, ids, None), reference(eng, None, None)
        base, base_all = eng.theta_info(ids), eng.theta_info()
        assert_matches(base, ref, "device: ")
        assert_matches(base_all, ref_all, "device, whole shard: ")
        for var, values in (("TSAMD_TEST_INFO_CHUNK", ("8", "1")), ("TSAMD_TEST_INFO_BLOCK", ("64", "20"))):
            for v in values:
                monkeypatch.setenv(var, v)
                got, got_all = eng.theta_info(ids), eng.theta_info()
                e = max(assert_close(got, base), assert_close(got_all, base_all))
                print(f"{var}={v}: max |difference| / H = {e:.3e}")
                assert_matches(got, ref, f"{var}={v}: ")
                assert_matches(got_all, ref_all, f"{var}={v}, whole shard: ")
            monkeypatch.delenv(var)
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
        with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as small:  # (the same seed: the same state)
            assert small.state_export()[0].tobytes() == eng.state_export()[0].tobytes()
            got = small.theta_info(ids)
        print(f"four units: max |difference| / H = {assert_close(got, base):.3e}")
        assert_matches(got, ref, "four units: ")
        monkeypatch.delenv("TSAMD_TEST_MAX_WORKGROUPS")
        # additivity over disjoint location lists
        la, lb = np.arange(0, 71, dtype=np.uint32), np.arange(71, l, dtype=np.uint32)
        ha, hb, hab = eng.theta_info(ids, la), eng.theta_info(ids, lb), eng.theta_info(ids, np.concatenate([la, lb]))
        e = assert_close({key: ha[key] + hb[key] for key in ha}, hab)
        print(f"additivity: max |H(A) + H(B) - H(A || B)| / H = {e:.3e}")


def test_a_shard_answers_for_global_ids(ts):
    n, l, k = 1030, 33, 6
    with synth_engine(ts, n, l, k, 17) as one, synth_engine(ts, n, l, k, 17, rank=1, world=2) as shard:
        assert shard.shard_begin > 0 and shard.shard_begin + shard.shard_count == n
        ids = pick_ids(np.random.default_rng(3), shard, 100)
        assert ids.min() >= shard.shard_begin
        a, b = one.theta_info(ids), shard.theta_info(ids)
        print(f"rank 1 of 2 against one context: max |difference| / H = {assert_close(b, a):.3e}")
        assert_matches(b, reference(shard, ids, None), "rank 1 of 2: ")
        whole = shard.theta_info()  # indivs == NULL: the shard's own individuals
        rows = one.theta_info(np.arange(shard.shard_begin, n, dtype=np.uint32))
        assert_close(whole, rows)
        with pytest.raises(ts.TsamdError) as err:  # an id of the other shard
            shard.theta_info(np.array([ids[0], 0], dtype=np.uint32))
        assert err.value.code == EINVAL and "indivs[1]" in str(err.value)


def test_bad_arguments_are_refused_and_the_context_stays_usable(ts):
    n, l, k = 200, 9, 2
    with synth_engine(ts, n, l, k, 2) as eng:
        s0 = eng.state_export()
        some = np.array([3, 1], dtype=np.uint32)
        for kwargs, word in ((dict(indivs=np.array([], dtype=np.uint32)), "m must be positive"),
                             (dict(indivs=some, locs=np.array([], dtype=np.uint32)), "n_locs"),
                             (dict(indivs=some, locs=np.array([1, l], dtype=np.uint32)), "locs[1]"),
                             (dict(indivs=np.array([3, n], dtype=np.uint32)), "indivs[1]")):
            with pytest.raises(ts.TsamdError) as e:
                eng.theta_info(**kwargs)
            assert e.value.code == EINVAL and word in str(e.value), kwargs
        assert raw_call(eng, None, None, m=n + 1, n_locs=l)[0] == EINVAL  # (NULL: the first m of 200)
        assert raw_call(eng, None, None, m=1, n_locs=l + 1)[0] == EINVAL  # (NULL: locations 0 .. n_locs-1)
        assert raw_call(eng, None, None, m=0, n_locs=l)[0] == EINVAL
        assert raw_call(eng, some, None, n_locs=0)[0] == EINVAL
        s1 = eng.state_export()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        assert_matches(eng.theta_info(some), reference(eng, some, None))


def test_held_out_entries_drop_out_by_their_term(ts):
    """holding out an individual's entry at a location changes exactly that individual's rows, by that term"""
    n, l, k = 700, 20, 4
    with synth_engine(ts, n, l, k, 31, held=False) as eng:
        who, loc = 333, 7
        y = genotypes(eng, np.arange(n), np.arange(l))
        assert y[who, loc] != 3
        before = eng.theta_info()
        eng.set_heldout(loc, np.array([who], dtype=np.uint32))
        after = eng.theta_info()
        others = np.arange(n) != who
        term = tr.info_fp64(eng.get_theta()[who:who + 1], eng.get_ebeta()[loc:loc + 1], y[who:who + 1, loc:loc + 1])
        for key in ("obs", "exp"):
            assert after[key][others].tobytes() == before[key][others].tobytes()
            assert np.all(term[key] > 0)
            d = before[key][who] - after[key][who]
            assert np.all(np.abs(d - term[key][0]) <= 1e-12 * before[key][who]), key
        assert_matches(after, reference(eng, None, None), "one entry held out: ")


def test_an_individual_without_entries_is_not_identified(ts):
    n, l, k = 300, 24, 3
    rng = np.random.default_rng(8)
    y = rng.integers(0, 3, size=(l, n)).astype(np.uint8)
    locs = np.array([2, 5, 11, 17, 5], dtype=np.uint32)
    y[locs, 77] = 3  # every listed location missing
    with ts.Engine(n, l, k) as eng:
        eng.upload_bed(pack_bed(y))
        eng.set_gamma(rng.gamma(2.0, 1.0, size=(n, k)))
        beta = rng.uniform(0.05, 0.95, size=(l, k))
        eng.set_lambda_range(np.stack([50.0 * beta, 50.0 * (1.0 - beta)], axis=2))
        got = eng.theta_info(None, locs)
        assert not got["obs"][77].any() and not got["exp"][77].any()
        assert_matches(got, reference(eng, None, locs), "one individual empty: ")
        se = ts.theta_se(got["obs"], k)
    assert se["status"][77] == 1 and np.isnan(se["se"][77]).all() and np.isnan(se["cov"][77]).all()
    rest = np.arange(n) != 77
    assert np.all(se["status"][rest] == 0) and np.all(se["se"][rest] > 0)


def test_calibration_on_the_device(ts):
    """the CPU fixture for seed 6: fold-in from gamma = 1 for 200 updates, then the information at the result; the spread of the
    fitted theta over the 256 replicates against the mean standard error, and the coverage of the nominal 95 % intervals"""
    case = tr.calibration_case(6)
    n, l, k = tr.CAL_N, tr.CAL_L, tr.CAL_K
    with ts.Engine(n, l, k) as eng:
        eng.upload_bed(pack_bed(case["y"]))
        eng.set_lambda_range(case["lam"])
        eng.set_gamma(np.ones((n, k)))
        eng.fold_in(max_iters=200)
        theta = eng.get_theta()
        info = eng.theta_info()
        assert_matches(info, reference(eng, None, None), "calibration: ")
    for key in ("obs", "exp"):
        out = ts.theta_se(info[key], k)
        assert np.all(out["status"] == 0)
        tr.assert_calibrated(theta, out["se"], f"device, {key}: ")
        cov = ts.info_unpack(out["cov"], k)
        assert np.all(np.abs(cov.sum(axis=2)) <= 1e-12 * np.abs(cov).max(axis=(1, 2))[:, None])
