"""tsamd_state_export / tsamd_state_import: a cut of the schedule that goes through two blobs and a NEW context is
invisible bit for bit -- the contract include/tsamd.h states for cuts into calls ("each mode is bitwise reproducible and
independent of how a schedule is cut into calls").

Every case is the same experiment on seeded PSD data (3 % missing, held-out entries on two locations):
  A  runs S1 then S2, uninterrupted;
  B  runs S1, exports, is closed;
  C  a new engine with the same config: same genotypes and held-out sets, but NOT B's gamma -- imports, runs S2.
A and C then agree BITWISE (np.array_equal on the raw float64 arrays) in gamma, c_n, lambda over all l, Elogtheta, the
pass counters, and the inner passes of one more update.  Shapes are the smallest at which each path can go wrong: one
workgroup with row padding (203, 3), several workgroups with an in-launch exchange (4096, 8), rows that do not fill a
tile of the pack kernel (K = 5, 20, 32), the run-time-K kernels (K = 40) and ts_hybrid with streamed items on four
workgroups.  w is saved, not recomputed: the late-state case and every case whose S1 ends in a training call would
differ in the last bits otherwise (ts_refresh_w scales by the row maximum, the gamma steps by exp(a - a_max))."""
import struct

import numpy as np
import pytest

import late_state
from helpers import init_gamma, pack_bed, psd_genotypes, rel_err
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

HDR = 128                        # sizeof(tsamd_state_header)
OFF_N, OFF_K, OFF_CHECKSUM = 12, 20, 104
S1_TRAIN = np.array([3, 7, 7, 1, 0, 9, 4, 11, 2, 5], dtype=np.uint32)       # ends on location 5
VAL = np.array([1, 6, 8, 10], dtype=np.uint32)                               # held-out sets at 1 and 6
S2_TAIL = np.array([8, 2, 2, 10, 6, 0, 3], dtype=np.uint32)


def fnv1a_words(payload):
    h = 14695981039346656037
    for w in np.frombuffer(payload, dtype="<u8"):
        h = ((h ^ int(w)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class Data:
    def __init__(self, n, l, k, seed):
        y, _, _ = psd_genotypes(n, l, k, seed, 0.03)
        self.n, self.l, self.k = n, l, k
        self.payload = pack_bed(y)
        self.gamma = init_gamma(n, k, seed + 1)
        rng = np.random.default_rng(seed + 2)
        self.held = {}
        for loc in (1, 6):
            cand = np.nonzero(y[loc] != 3)[0]
            self.held[loc] = np.sort(rng.choice(cand, size=min(7, len(cand)), replace=False)).astype(np.uint32)


def new_engine(ts, d, mode=None, flags=0, with_gamma=True, **over):
    eng = ts.Engine(d.n, d.l, d.k, flags=flags, **over)
    eng.upload_bed(d.payload)
    for loc, ind in d.held.items():
        eng.set_heldout(loc, ind)
    if with_gamma:
        eng.set_gamma(d.gamma)
    if mode is not None:
        eng.set_launch_mode(mode)
    return eng


def run_s1(eng, pending):
    if pending == "empty":
        return None
    eng.run_schedule(S1_TRAIN)
    if pending == "hol":
        eng.run_schedule(VAL, 1)
        return int(VAL[-1])
    if pending == "clear":
        eng.clear_pending()
    return int(S1_TRAIN[-1])


def run_s2(eng, first):
    eng.run_schedule(np.concatenate([[first], S2_TAIL]).astype(np.uint32))
    eng.run_schedule(VAL, 1)
    eng.run_schedule(S2_TAIL[:3])
    eng.synchronize()


def observe(eng):
    """everything the issue lists, then the inner passes of one more update"""
    out = [eng.get_gamma(), eng.get_counts(), eng.get_lambda(), eng.get_elogtheta(), np.uint64(eng.total_passes()),
           eng.pass_histogram()]
    out.append(np.uint32(eng.snp_update(4)))
    out += [eng.get_gamma(), eng.get_lambda()]
    return out


def assert_bitwise(a, c, what):
    names = ("gamma", "c_n", "lambda", "Elogtheta", "total_passes", "pass_histogram", "inner_iters", "gamma after", "lambda after")
    for x, y, name in zip(a, c, names):
        assert np.array_equal(x, y), f"{what}: {name} differs"


def experiment(ts, d, what, mode=None, pending="train", flags=0, prepare=None, check_s1=None, **over):
    """A against C for S2 beginning at the location S1 ended on (the NextSnp hazard: its values are not taken from the
    one-ahead capture) and at another one"""
    for same in (True, False):
        def start():
            eng = new_engine(ts, d, mode, flags, **over)
            if prepare:
                prepare(eng)
            return eng
        with start() as a:
            last = run_s1(a, pending)
            first = (last if last is not None else 5) if same else 9
            run_s2(a, first)
            want = observe(a)
        with start() as b:
            run_s1(b, pending)
            if check_s1:
                check_s1(b)
            sizes = b.state_sizes()
            indiv, loc = b.state_export()
            assert (indiv.size, loc.size) == sizes
        with new_engine(ts, d, mode, flags, with_gamma=False, **over) as c:
            c.state_import(indiv, loc)
            run_s2(c, first)
            got = observe(c)
        assert_bitwise(want, got, f"{what} pending={pending} same_loc={same}")


SMALL = [(203, 3), (4096, 8)]


@pytest.mark.parametrize("mode_name", ["LAUNCH_PER_PASS", "LAUNCH_PER_SNP", "LAUNCH_PER_SCHEDULE"])
@pytest.mark.parametrize("n,k", SMALL)
def test_resume_is_bitwise_in_every_launch_mode(ts, n, k, mode_name):
    d = Data(n, 12, k, 7000 + n)
    mode = getattr(ts, mode_name)

    def check(eng):
        want = {ts.LAUNCH_PER_PASS: eng.cfg.max_inner, ts.LAUNCH_PER_SNP: 2, ts.LAUNCH_PER_SCHEDULE: 0}[mode]
        assert eng.launch_info()["kernels_per_snp"] == want
    experiment(ts, d, f"{mode_name} n={n} K={k}", mode=mode, check_s1=check)


@pytest.mark.parametrize("pending", ["hol", "empty", "clear"])
@pytest.mark.parametrize("n,k", SMALL)
def test_resume_pending_record(ts, n, k, pending):
    """S1 ends in a validation-mode call (no step pending), is empty (a fresh context), or is followed by clear_pending"""
    experiment(ts, Data(n, 12, k, 7100 + n), f"n={n} K={k}", pending=pending)


@pytest.mark.parametrize("thresh,passes", [(1e9, 1), (0.0, 10)])
@pytest.mark.parametrize("n,k", SMALL)
def test_resume_after_one_pass_and_at_the_pass_cap(ts, n, k, thresh, passes):
    """the last update of S1 stops after its first pass (every mean |dlambda| is below 1e9) / runs into max_inner (none is
    below 0)"""
    def check(eng):
        hist = eng.pass_histogram()
        assert hist[passes] == len(S1_TRAIN) and hist.sum() == len(S1_TRAIN)
    experiment(ts, Data(n, 12, k, 7200 + n), f"n={n} K={k} thresh={thresh}", check_s1=check, conv_thresh=thresh)


@pytest.mark.parametrize("n,k", [(1000, 5), (700, 20), (520, 32), (300, 40)])
def test_resume_tile_edges_and_wide_k(ts, n, k):
    """odd K and rows that do not fill a tile of ts_state_pack / ts_state_unpack (256 individuals at K <= 8, 128 to K = 16,
    64 to K = 32, 32 above); K = 40 runs ts_pass_wide / ts_refresh_w_wide"""
    def check(eng):
        if k > 32:
            assert eng.launch_info()["kernels_per_snp"] == eng.cfg.max_inner
    experiment(ts, Data(n, 16, k, 7300 + n), f"n={n} K={k}", check_s1=check)


def test_resume_hybrid_with_streamed_items(ts, monkeypatch):
    """ts_hybrid on four workgroups: weights split over registers, LDS and HBM (sized as tests/test_gpu_late_state.py does)"""
    monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
    k = 8
    chip = 16 + min(16, (160 * 1024 - 1024 - 200 * k) // (k * 8 * 256))
    n = 4 * 256 * (chip + 3) - 37

    def check(eng):
        geo = eng.schedule_geometry()
        assert geo["workgroups"] == 4 and geo["indivs_per_thread"] == chip + 3 and geo["on_chip_per_thread"] == chip, geo
    experiment(ts, Data(n, 12, k, 7400), "ts_hybrid", flags=ts.FLAG_TEST_HOOKS, check_s1=check)


def test_resume_from_a_late_state(ts):
    """from tests/late_state.py's planted state (gamma rows of ~1e6 with components at the 1e-8 floor, c_n to 1e6, lambda of
    order N): a w that is silently recomputed on import shows here"""
    n, l, k, l_eff = 3000, 12, 8, 5e5
    s = late_state.plant(n, l, k, 7500, l_eff=l_eff, held_locs=(1, 6))
    d = Data.__new__(Data)
    d.n, d.l, d.k, d.payload, d.gamma, d.held = n, l, k, s.payload, s.gamma, s.held

    def prepare(eng):
        eng.set_counts(s.counts)
        for loc in range(l):
            eng.set_lambda(loc, s.lam[loc])
    experiment(ts, d, "late state", prepare=prepare, gamma_scale=l_eff)


@pytest.mark.parametrize("n,k", [(203, 3), (700, 20), (300, 40)])
def test_round_trip_gives_identical_bytes(ts, n, k):
    d = Data(n, 12, k, 7600 + n)
    with new_engine(ts, d) as eng:
        run_s1(eng, "train")
        indiv, loc = eng.state_export()
        assert (indiv.size, loc.size) == eng.state_sizes()
        assert indiv.size == HDR + 16 * n * k + (4 * n + 7) // 8 * 8
        assert loc.size == HDR + 32 * d.l * k + 32 + 32 * k + 8 + 8 * 128
        for blob in (indiv, loc):
            assert struct.unpack_from("<Q", blob, OFF_CHECKSUM)[0] == fnv1a_words(blob[HDR:].tobytes())
        # the rows are the getters' (gamma first, c_n last), the location part starts with lambda
        assert np.array_equal(np.frombuffer(indiv[HDR:HDR + 8 * n * k].tobytes()).reshape(n, k), eng.get_gamma())
        assert np.array_equal(np.frombuffer(indiv[HDR + 16 * n * k:HDR + 16 * n * k + 4 * n].tobytes(), dtype=np.uint32), eng.get_counts())
        assert np.array_equal(np.frombuffer(loc[HDR:HDR + 16 * d.l * k].tobytes()).reshape(d.l, k, 2), eng.get_lambda())
        eng.state_import(indiv, loc)
        indiv2, loc2 = eng.state_export()
        assert np.array_equal(indiv, indiv2) and np.array_equal(loc, loc2)
        # one part at a time
        only_i, none = eng.state_export(loc=False)
        none2, only_l = eng.state_export(indiv=False)
        assert none is None and none2 is None and np.array_equal(only_i, indiv) and np.array_equal(only_l, loc)
        eng.state_import(loc=loc)
        eng.state_import(indiv=indiv)
        indiv3, loc3 = eng.state_export()
        assert np.array_equal(indiv, indiv3) and np.array_equal(loc, loc3)


def test_import_refuses_and_leaves_the_context_unchanged(ts):
    n, l, k = 203, 12, 3
    d = Data(n, l, k, 7700)
    with new_engine(ts, d, nodetau0=3.0) as other:
        run_s1(other, "train")
        tau_indiv, tau_loc = other.state_export()
    with new_engine(ts, d) as src:
        run_s1(src, "train")
        indiv, loc = src.state_export()

    def patched(blob, off, fmt, value):
        out = blob.copy()
        struct.pack_into(fmt, out, off, value)
        return out

    flipped_i, flipped_l = indiv.copy(), loc.copy()
    flipped_i[HDR + 8 * 17 + 3] ^= 0x10
    flipped_l[-5] ^= 0x01
    nan_gamma = indiv.copy()
    struct.pack_into("<d", nan_gamma, HDR + 8 * 5, float("nan"))
    struct.pack_into("<Q", nan_gamma, OFF_CHECKSUM, fnv1a_words(nan_gamma[HDR:].tobytes()))
    cases = {
        "flipped payload byte (indiv)": (flipped_i, loc, "checksum"),
        "flipped payload byte (loc)": (indiv, flipped_l, "checksum"),
        "truncated blob": (indiv[:-8], loc, "byte count"),
        "truncated loc blob": (indiv, loc[:-100], "byte count"),
        "wrong k": (patched(indiv, OFF_K, "<I", k + 1), loc, " k "),
        "wrong n": (indiv, patched(loc, OFF_N, "<I", n + 1), " n "),
        "changed nodetau0": (tau_indiv, tau_loc, "nodetau0"),
        "changed nodetau0 (loc only)": (None, tau_loc, "nodetau0"),
        "swapped parts": (loc, indiv, "part"),
        "NaN in gamma under a recomputed checksum": (nan_gamma, loc, "gamma[5]"),
    }
    with new_engine(ts, d) as eng:
        eng.run_schedule(S2_TAIL)
        eng.run_schedule(VAL, 1)
        eng.synchronize()

        def snapshot():
            return [eng.get_gamma(), eng.get_counts(), eng.get_lambda(), eng.get_elogtheta(), np.uint64(eng.total_passes()),
                    eng.pass_histogram()] + list(eng.state_export())
        before = snapshot()
        for name, (a, b, word) in cases.items():
            with pytest.raises(ts.TsamdError) as ei:
                eng.state_import(a, b)
            assert ei.value.code == -1 and word in str(ei.value), (name, str(ei.value))
            for x, y in zip(before, snapshot()):
                assert np.array_equal(x, y), name
        eng.state_import(indiv, loc)          # and the good blobs still go in
        got = eng.state_export()
        assert np.array_equal(got[0], indiv) and np.array_equal(got[1], loc)


def test_export_in_one_mode_import_in_another(ts):
    """exported under LAUNCH_PER_SCHEDULE, imported into a context lowered to LAUNCH_PER_PASS: the bound include/tsamd.h gives
    between modes (rel 1e-11)"""
    d = Data(4096, 12, 8, 7800)
    with new_engine(ts, d, ts.LAUNCH_PER_SCHEDULE) as a:
        last = run_s1(a, "train")
        run_s2(a, last)
        want = observe(a)
    with new_engine(ts, d, ts.LAUNCH_PER_SCHEDULE) as b:
        run_s1(b, "train")
        indiv, loc = b.state_export()
    with new_engine(ts, d, ts.LAUNCH_PER_PASS, with_gamma=False) as c:
        c.state_import(indiv, loc)
        assert c.launch_info()["kernels_per_snp"] == c.cfg.max_inner
        run_s2(c, last)
        got = observe(c)
    for i in (0, 2, 7, 8):
        e = rel_err(got[i], want[i])
        print(f"cross-mode rel err [{i}] = {e:.3e}")
        assert e <= 1e-11
    assert np.array_equal(got[1], want[1]) and got[4] == want[4] and np.array_equal(got[5], want[5]) and got[6] == want[6]
