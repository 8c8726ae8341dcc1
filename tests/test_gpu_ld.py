"""tsamd_ld: structure-adjusted LD of nearby listed locations on the matrix cores, and the pruning built on it.

The reference is numpy fp64 from reads of the engine only -- get_theta(), get_ebeta() and download_bed() (which shows held-out
entries as missing, as wanted; tests/test_gpu_ld_refs.py holds the call to a long-double reference from the planted inputs alone,
within a derived bound, at every K and from a late-training state):
    q = theta[n] . Ebeta[j],  h = 2q (1 - q),  z = (y - 2q) / sqrt(h),  m = 1,  both 0 where the stored code is 01 or h <= 0
    num[i][d] = sum_n z(n, i) z(n, i + d),  cnt[i][d] = sum_n m(n, i) m(n, i + d),  0 where i + d is past the list

Tolerances: cnt exact; |num - ref| <= 1e-11 sum_n |z_i z_j|, kinship's bound.  For this call: one factor of one term carries a
relative error of (2 K q / (1 - q) + 10) 2^-53 -- with q <= 0.95 at most about 5e-13 at K = 128, hence about 1e-12 for a
two-factor term -- and the sum adds n 2^-53, so 1e-11 leaves about 8x at worst.  Other geometries (chunks of 64 and 128
locations, blocks of 64 and 260 individuals, a four-unit device) and the sum of two shards against one context to 1e-12 of
sum |terms|, cnt equal; repeatability, either output NULL and the untouched state bit for bit.  n = 1024 with blocks of 260
and 100 individuals: the shard fills its padded column and the later blocks start off a dword, so a workgroup's word straddles
the column's end with live individuals in the bytes before it (2.2e-15 of sum |terms|, cnt exact).
Largest errors observed on one MI355X (2026-10-21), as multiples of sum |terms|: 4.1e-14 for num at K = 1 (every individual
shares q there, so the rounding of q does not average out over the sum; 1.5e-14 in the every-K file's K = 1) and 2.5e-15 at
most at every other K, 33 and 128 included; other geometries against the default 2.3e-15 (chunks alone: the same bits); the
sum of two shards against one context 6.1e-16; the planted sample 3.9e-15.

Shapes (n, l, k, W): W = 1 and 5 keep the band inside a tile pair's diagonal neighbourhood, 63 / 64 / 65 sit around the tile
edge (1 and 2 overlap tiles), 130 is wider than the list of 70 (every row ends in zero columns), 70 spans two tiles at l = 66;
l = 37 is one ragged tile, 130 / 150 / 200 are 3 and 4 tiles with a ragged last one; n = 700 .. 2100 are 3 to 9 workgroups of
ts_ld_resid with a ragged last one and a last k-step of 4 partly empty at n = 1030; k = 1 .. 32 run the specialised residual
kernels, 33 and 128 the run-time-K one.  With random data a transposed or mis-rowed read-out of the MFMA accumulators, or a
band column taken from the wrong tile pair, cannot pass.

Planted LD: n = 2000, l = 192, K = 3, W = 32, 10 % missing, theta ~ Dirichlet(0.3), beta ~ U(0.05, 0.95), the model set from the
truth; four planted pairs (10, 11), (40, 45), (100, 132), (150, 151) share beta and each haplotype of the second copies the
first with probability 0.9.  With t = r sqrt(cnt), on the numpy reference alone and on the device's output alike: the 5 612
unlinked band pairs have max |t| <= 5 and an sd of t in [0.9, 1.1]; planted r lies in [0.7, 1.1]; ld_prune at r2_max = 0.5 drops
exactly {11, 45, 132, 151}.  On the numpy reference, seeds 5 to 10 of this sample: max |t| 3.6 to 4.1, sd 1.000 to 1.016, planted r
0.82 to 0.96, largest unlinked r^2 0.008 to 0.010.  RAW genotype r^2 (plain correlation of the genotypes, the usual pruning tools'
measure) among the unlinked pairs averages 0.011 to 0.020 against 0.0006 adjusted: population structure alone makes unlinked
ancestry-informative SNPs look linked, which is the point of the call.  The test computes both on its sample (seed 5: raw 0.0142,
adjusted 0.00062) and asserts the adjusted mean within half of 1 / cnt = 1 / (0.81 n), an unlinked pair's expectation under
the model, and the raw mean above ten times that."""
import ctypes as C

import numpy as np
import pytest

from helpers import pack_bed, unpack_bed
from test_gpu_kinship import assert_close, pick_locs, synth_engine
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(700, 37, 3, 1), (700, 130, 8, 63), (1030, 200, 8, 65), (2100, 70, 1, 130), (1030, 150, 20, 64), (700, 100, 32, 5), (700, 66, 33, 70),
          (600, 40, 128, 8)]


def ld_reference(theta, eb, y, window):
    """dict(num, cnt, absn), bands [J][window + 1], from theta [n][k], Ebeta [J][k] and genotypes y [n][J] in {0, 1, 2, 3 = no term}"""
    q = theta @ eb.T
    h = 2.0 * q * (1.0 - q)
    ok = (y != 3) & (h > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(ok, (y.astype(np.float64) - 2.0 * q) / np.sqrt(h), 0.0)
    m = ok.astype(np.float64)
    J = y.shape[1]
    num, absn, cnt = (np.zeros((J, window + 1)) for _ in range(3))
    for d in range(min(window, J - 1) + 1):
        num[:J - d, d] = np.sum(z[:, :J - d] * z[:, d:], axis=0)
        absn[:J - d, d] = np.sum(np.abs(z[:, :J - d] * z[:, d:]), axis=0)
        cnt[:J - d, d] = np.sum(m[:, :J - d] * m[:, d:], axis=0)
    return dict(num=num, cnt=cnt.astype(np.uint32), absn=absn)


def reference(eng, locs, window):
    locs = np.arange(eng.l) if locs is None else np.asarray(locs, dtype=np.int64)
    cols = {int(x): unpack_bed(eng.download_bed(int(x))[None, :], eng.shard_count)[0] for x in set(locs.tolist())}
    y = np.stack([cols[int(x)] for x in locs], axis=1)  # [n][J]
    return ld_reference(eng.get_theta(), eng.get_ebeta()[locs], y, window)


def assert_matches(got, ref, what=""):
    num, cnt = got["num"], got["cnt"]
    assert num.shape == ref["num"].shape and cnt.shape == ref["cnt"].shape and cnt.dtype == np.uint32
    e = float(np.max(np.abs(num - ref["num"]) / np.where(ref["absn"] > 0, ref["absn"], 1.0)))
    print(f"{what}max |num - ref| / sum |z z| = {e:.3e}")
    assert cnt.tobytes() == ref["cnt"].tobytes()
    assert np.all(np.abs(num - ref["num"]) <= 1e-11 * ref["absn"])
    J, w1 = num.shape
    past = np.add.outer(np.arange(J), np.arange(w1)) >= J  # columns beyond the list's end: exactly 0
    assert np.all(num[past] == 0.0) and np.all(cnt[past] == 0)
    return e


def raw_call(eng, locs, window, want_num=True, want_cnt=True):
    """tsamd_ld itself, either output NULL: (rc, num, cnt)"""
    locs = np.ascontiguousarray(locs, dtype=np.uint32)
    num = np.zeros((locs.size, window + 1)) if want_num else None
    cnt = np.zeros((locs.size, window + 1), dtype=np.uint32) if want_cnt else None
    rc = eng.h.tsamd_ld(eng.ctx, locs.ctypes.data_as(C.POINTER(C.c_uint32)), locs.size, window,
                        None if num is None else num.ctypes.data_as(C.POINTER(C.c_double)),
                        None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
    return rc, num, cnt


@pytest.mark.parametrize("n,l,k,w", SHAPES)
def test_parity_with_numpy(ts, n, l, k, w):
    with synth_engine(ts, n, l, k, 40 + k + w) as eng:
        locs = pick_locs(np.random.default_rng(w), l)
        assert len(set(locs.tolist())) < len(locs) and list(locs) != sorted(locs)
        for which in (None, locs):
            got = eng.ld(which, w)
            ref = reference(eng, which, w)
            assert got["num"].shape == ((l if which is None else len(locs)), w + 1)
            assert_matches(got, ref, f"N={n} L={l} K={k} W={w} {'list' if which is not None else 'all'}: ")
        # a repeated location is a row of its own: its column 0 is that of its first appearance (another chunk column: to rounding)
        rep, first = len(locs) - 2, 1
        assert locs[rep] == locs[first]
        assert got["cnt"][rep, 0] == got["cnt"][first, 0]
        assert abs(got["num"][rep, 0] - got["num"][first, 0]) <= 1e-11 * ref["absn"][first, 0]
        if rep - first <= w:  # the pair of the two: a location with itself again
            assert got["cnt"][first, rep - first] == got["cnt"][first, 0]


def test_repeatable_and_the_same_with_either_output_null(ts):
    with synth_engine(ts, 1030, 150, 8, 3) as eng:
        locs, w = pick_locs(np.random.default_rng(1), 150), 70
        a, b = eng.ld(locs, w), eng.ld(locs, w)
        assert a["num"].tobytes() == b["num"].tobytes() and a["cnt"].tobytes() == b["cnt"].tobytes()
        rc, num, _ = raw_call(eng, locs, w, want_cnt=False)
        assert rc == 0 and num.tobytes() == a["num"].tobytes()
        rc, _, cnt = raw_call(eng, locs, w, want_num=False)
        assert rc == 0 and cnt.tobytes() == a["cnt"].tobytes()


def test_the_call_changes_no_state_in_any_launch_mode(ts):
    n, l, k = 1030, 40, 5
    head, tail = np.array([3, 8, 1], dtype=np.uint32), np.array([4, 4, 17, 0, 9, 33], dtype=np.uint32)
    for mode in (ts.LAUNCH_PER_PASS, ts.LAUNCH_PER_SNP, ts.LAUNCH_PER_SCHEDULE):
        outs = []
        for call in (True, False):
            with synth_engine(ts, n, l, k, 23) as e:
                e.set_launch_mode(mode)
                e.run_schedule(head)  # ends in a training update: its gamma step is pending
                e.synchronize()
                if call:
                    s0, p0, h0, c0 = e.state_export(), e.total_passes(), e.pass_histogram(), e.get_counts()
                    e.ld(np.array([5, 1, 1, 39], dtype=np.uint32), 2)
                    e.ld()
                    s1 = e.state_export()
                    assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes(), mode
                    assert e.total_passes() == p0 and e.pass_histogram().tobytes() == h0.tobytes() and e.get_counts().tobytes() == c0.tobytes()
                e.run_schedule(tail)  # applies the pending step: exactly as without the call
                e.run_schedule(tail[:2], 1)
                e.synchronize()
                outs.append(e.state_export())
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), mode


def test_other_geometries_agree(ts, monkeypatch):
    """chunks of 64 and 128 locations (4 and 2 chunks of the 200: pairs straddle chunks, 2 overlap tiles at W = 65), blocks of 64
    and 260 individuals (11 and 3 blocks, the last ragged) and the geometry of a four-unit device: the same sums in another
    association"""
    n, l, k, w = 700, 200, 8, 65
    for var in ("TSAMD_TEST_LD_CHUNK", "TSAMD_TEST_LD_BLOCK", "TSAMD_TEST_MAX_WORKGROUPS"):
        monkeypatch.delenv(var, raising=False)
    with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as eng:
        ref = reference(eng, None, w)
        base = eng.ld(None, w)
        assert_matches(base, ref, "device: ")
        for var, values in (("TSAMD_TEST_LD_CHUNK", ("64", "128")), ("TSAMD_TEST_LD_BLOCK", ("64", "260"))):
            for v in values:
                monkeypatch.setenv(var, v)
                got = eng.ld(None, w)
                assert got["cnt"].tobytes() == base["cnt"].tobytes()
                e = assert_close(got["num"], base["num"], ref["absn"])
                print(f"{var}={v}: max |difference| / sum |terms| = {e:.3e}")
                assert_matches(got, ref, f"{var}={v}: ")
            monkeypatch.delenv(var)
        monkeypatch.setenv("TSAMD_TEST_LD_CHUNK", "64")  # both at once, on a list
        monkeypatch.setenv("TSAMD_TEST_LD_BLOCK", "64")
        locs = pick_locs(np.random.default_rng(4), l)
        assert_matches(eng.ld(locs, w), reference(eng, locs, w), "chunk 64, block 64, a list: ")
        monkeypatch.delenv("TSAMD_TEST_LD_CHUNK")
        monkeypatch.delenv("TSAMD_TEST_LD_BLOCK")
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
        with synth_engine(ts, n, l, k, 29, flags=ts.FLAG_TEST_HOOKS) as small:  # (the same seed: the same state)
            assert small.state_export()[0].tobytes() == eng.state_export()[0].tobytes()
            got = small.ld(None, w)
        assert got["cnt"].tobytes() == base["cnt"].tobytes()
        e = assert_close(got["num"], base["num"], ref["absn"])
        print(f"four units: max |difference| / sum |terms| = {e:.3e}")
        assert_matches(got, ref, "four units: ")


@pytest.mark.parametrize("block", [260, 100])
def test_a_block_that_starts_off_a_dword_reads_the_columns_last_bytes(ts, monkeypatch, block):
    """n = 1024 fills the padded column (npad = 1024, 256 bytes) to its last byte.  Blocks of 260 (100) individuals start at
    780 (1000), not a multiple of 16, so the workgroup's words of 16 individuals lie off the dword boundaries and one of them
    straddles the column's end with 1 (2) of its bytes inside: individuals 1020 .. 1023 (1016 .. 1023) live in those bytes.
    Taking such a word as missing loses them: cnt comes out 4 (8) short, less the missing entries, in every entry."""
    n, l, k, w = 1024, 70, 4, 9
    monkeypatch.setenv("TSAMD_TEST_LD_BLOCK", str(block))
    with synth_engine(ts, n, l, k, 31, flags=ts.FLAG_TEST_HOOKS) as eng:
        assert eng.shard_count == n
        assert_matches(eng.ld(None, w), reference(eng, None, w), f"N={n}, blocks of {block}: ")


def test_two_shards_add_up_to_one_context(ts):
    n, l, k, w = 1030, 70, 6, 9
    with synth_engine(ts, n, l, k, 17) as one, synth_engine(ts, n, l, k, 17, rank=0, world=2) as r0, \
            synth_engine(ts, n, l, k, 17, rank=1, world=2) as r1:
        assert r0.shard_count + r1.shard_count == n and r1.shard_begin == r0.shard_count
        whole, a, b = one.ld(None, w), r0.ld(None, w), r1.ld(None, w)
        ref = reference(one, None, w)
        assert (a["cnt"] + b["cnt"]).tobytes() == whole["cnt"].tobytes()
        e = assert_close(a["num"] + b["num"], whole["num"], ref["absn"])
        print(f"rank 0 + rank 1 against one context: max |difference| / sum |terms| = {e:.3e}")
        assert_matches(b, reference(r1, None, w), "rank 1 of 2: ")


def test_bad_arguments_are_refused_and_the_context_stays_usable(ts):
    n, l, k = 200, 9, 2
    with synth_engine(ts, n, l, k, 2) as eng:
        s0 = eng.state_export()
        some = np.array([3, 1, 8], dtype=np.uint32)
        for kwargs, word in ((dict(locs=np.array([], dtype=np.uint32)), "n_locs"),
                             (dict(locs=some, window=0), "window"),
                             (dict(locs=some, window=ts._lib.LD_MAX_WINDOW + 1), "TSAMD_LD_MAX_WINDOW"),
                             (dict(locs=np.array([1, l], dtype=np.uint32)), "locs[1]")):
            with pytest.raises(ts.TsamdError) as e:
                eng.ld(**kwargs)
            assert e.value.code == EINVAL and word in str(e.value), kwargs
        rc, _, _ = raw_call(eng, some, 2, want_num=False, want_cnt=False)
        assert rc == EINVAL and "both NULL" in eng.last_error()
        one = np.zeros((l + 1, 2))
        assert eng.h.tsamd_ld(eng.ctx, None, l + 1, 1, one.ctypes.data_as(C.POINTER(C.c_double)), None) == EINVAL  # (NULL: locations 0 .. n_locs-1)
        s1 = eng.state_export()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        assert_matches(eng.ld(some, ts._lib.LD_MAX_WINDOW), reference(eng, some, ts._lib.LD_MAX_WINDOW))
        assert eng.ld(np.arange(l, dtype=np.uint32), 3)["num"].tobytes() == eng.ld(None, 3)["num"].tobytes()


PLANTED = [(10, 11), (40, 45), (100, 132), (150, 151)]


def planted_sample(seed=5, n=2000, l=192, k=3, missing=0.1):
    """(y [n][l] in {0, 1, 2, 3 = missing}, theta, beta): a PSD sample whose PLANTED pairs (a, b) share beta, each haplotype of
    b a copy of a's with probability 0.9 and a fresh draw otherwise"""
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.full(k, 0.3), size=n)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    for a, b in PLANTED:
        beta[b] = beta[a]
    p = theta @ beta.T  # [n][l]
    hap = rng.random((2, n, l)) < p
    for a, b in PLANTED:
        copy = rng.random((2, n)) < 0.9
        hap[:, :, b] = np.where(copy, hap[:, :, a], hap[:, :, b])
    y = hap[0].astype(np.uint8) + hap[1].astype(np.uint8)
    y[rng.random(y.shape) < missing] = 3
    return y, theta, beta


def check_planted(ts, num, cnt, window=32):
    """the call's own claims, on any band of the planted_sample(); returns the figures"""
    r, _ = ts.ld_statistics(num, cnt)
    J = r.shape[0]
    t = r * np.sqrt(cnt.astype(np.float64))
    i, d = np.meshgrid(np.arange(J), np.arange(window + 1), indexing="ij")
    unlinked = (d >= 1) & (i + d < J)
    for a, b in PLANTED:
        unlinked[a, b - a] = False
    assert int(unlinked.sum()) == 5612
    planted = np.array([r[a, b - a] for a, b in PLANTED])
    out = dict(max_t=float(np.abs(t[unlinked]).max()), sd_t=float(t[unlinked].std()), planted_r=planted.tolist(),
               max_unlinked_r2=float((r[unlinked] ** 2).max()), mean_unlinked_r2=float((r[unlinked] ** 2).mean()))
    assert out["max_t"] <= 5.0 and 0.9 <= out["sd_t"] <= 1.1
    assert np.all((planted >= 0.7) & (planted <= 1.1))
    keep = ts.ld_prune(r, 0.5)
    assert sorted(np.flatnonzero(~keep).tolist()) == [11, 45, 132, 151]
    return out


def raw_r2(y, window=32):
    """mean plain genotype r^2 (pairwise complete) of the unlinked band pairs"""
    J = y.shape[1]
    vals = []
    for i in range(J):
        for d in range(1, min(window, J - 1 - i) + 1):
            if (i, i + d) in PLANTED:
                continue
            ok = (y[:, i] != 3) & (y[:, i + d] != 3)
            vals.append(np.corrcoef(y[ok, i].astype(np.float64), y[ok, i + d].astype(np.float64))[0, 1] ** 2)
    return float(np.mean(vals))


def test_planted_ld_is_found_and_structure_is_not(ts):
    n, l, k, w = 2000, 192, 3, 32
    y, theta, beta = planted_sample(n=n, l=l, k=k)
    with ts.Engine(n, l, k) as eng:
        eng.upload_bed(pack_bed(np.ascontiguousarray(y.T)))
        eng.set_gamma(100.0 * theta + 1e-6)
        eng.set_lambda_range(np.stack([1000.0 * beta, 1000.0 * (1.0 - beta)], axis=2))
        got = eng.ld(None, w)
        ref = reference(eng, None, w)
    assert_matches(got, ref, "planted: ")
    print("reference:", check_planted(ts, ref["num"], ref["cnt"]))
    dev = check_planted(ts, got["num"], got["cnt"])
    print("device:", dev)
    # the point of the call: without the adjustment unlinked pairs look linked.  Under the model an unlinked pair's r^2 has the
    # mean 1 / cnt, about 1 / (0.81 n) = 0.0006 here; the raw figure is the docstring's
    raw = raw_r2(y, w)
    print(f"mean r^2 of the unlinked pairs: raw genotypes {raw:.4f}, adjusted {dev['mean_unlinked_r2']:.5f}")
    assert 0.5 / (0.81 * n) <= dev["mean_unlinked_r2"] <= 1.5 / (0.81 * n)
    assert raw >= 10.0 / (0.81 * n)
