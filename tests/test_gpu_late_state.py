"""Every kernel family from a planted late-training state (tests/late_state.py) against the CPU oracle.

The other parity tests start from the reference's initial state (gamma ~ 1, c_n = 0, lambda = eta, gamma_scale = l), so
their gammas stay below ~100, rho above ~0.15 and Ebeta inside (0.05, 0.95).  Here gamma_scale = L_eff = 5e5 or 1e6 in
the engine and the oracle, rows sum to ~2 L_eff with components down to the 1e-8 floor, c_n runs to 1e6 and lambda is of
order N with sides pinned at eta: the regime a production run spends its updates in, where exp_nonpos, exp_digamma_split,
fast_rcp and the families' own copies of the gamma step (the literal one at K <= 8, the lean one above, ts_hybrid's)
meet large exponents and extreme gammas.  Tolerances are the suite's: lambda and gamma rel 1e-9, c_n, pass counts and
the pass histogram exact; theta rel 1e-11 and Elogtheta abs 1e-12 (relative beyond magnitude 1: the 1e-8 floor gives
Elogtheta ~ -1e8) from the planted gamma; held-out log-likelihood rel 1e-10; one single update rel 1e-11.
"""
import numpy as np
import pytest

import late_state
import oracle_py as op
from helpers import rel_err, slow_params, usable_cores
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

TRAIN = np.array([3, 3, 7, 1, 7, 0, 2, 5, 9, 4, 4, 6], dtype=np.uint32)
VAL = np.array([0, 1, 2, 4, 6, 8], dtype=np.uint32)   # validation-mode entries (held-out sets at 1, 4, 6)
TRAIN2 = np.array([8, 2, 2, 5], dtype=np.uint32)
L = 10


def slow_cases(values, fast):
    """slow_params for several argnames: the cases not in `fast` carry the `slow` marker"""
    return [v if v in fast else pytest.param(*v, marks=pytest.mark.slow) for v in values]


def hist_of(its, bins):
    h = np.zeros(bins, dtype=np.uint64)
    for i in its:
        h[min(i, bins - 1)] += 1
    return h


def pair(ts, n, k, seed, l_eff=5e5, flags=0, eng_over=None, orc_over=None):
    s = late_state.plant(n, L, k, seed, l_eff=l_eff)
    eng = ts.Engine(n, L, k, flags=flags, gamma_scale=l_eff, **(eng_over or {}))
    late_state.load_engine(eng, s)
    orc = op.Oracle(n, L, k, nthreads=usable_cores() if n * k > 100_000 else 1, gamma_scale=l_eff, **(orc_over or {}))
    late_state.load_oracle(orc, s)
    return s, eng, orc


def check_theta(eng, orc):
    """theta and Elogtheta of the planted gamma (before any update: both sides read the same gamma)"""
    assert rel_err(eng.get_theta(), orc.theta()) < 1e-11
    e, o = eng.get_elogtheta(), orc.elogtheta()
    assert np.max(np.abs(e - o) / np.maximum(1.0, np.abs(o))) < 1e-12


def run_and_check(eng, orc, what, val=VAL):
    """training, a validation-mode block, training again; then the held-out log-likelihood both ways"""
    eng.run_schedule(TRAIN)
    eng.run_schedule(val, 1)
    eng.run_schedule(TRAIN2)
    eng.synchronize()
    its = [orc.snp_update(int(x)) for x in TRAIN] + [orc.snp_update(int(x), 1) for x in val] + [orc.snp_update(int(x)) for x in TRAIN2]
    hist = eng.pass_histogram()
    assert eng.total_passes() == sum(its) and np.array_equal(hist, hist_of(its, len(hist))), (what, its, hist[:12])
    assert rel_err(eng.get_lambda(), orc.lambda_()) < 1e-9, what + " lambda"
    assert rel_err(eng.get_gamma(), orc.gamma()) < 1e-9, what + " gamma"
    assert np.array_equal(eng.get_counts(), orc.c_indiv()), what + " c_n"
    for loc in (1, 4, 6):   # per location, from the state the training left
        s, c = eng.heldout_loglik(loc)
        so, co = orc.heldout_loglik(loc)
        assert c == co and abs(s - so) <= 1e-10 * abs(so), (what, loc, s, so)
    held = np.array([1, 4, 6], dtype=np.uint32)
    s, c, sums, cnts = eng.heldout_eval(held)   # validation updates of the held-out locations, then the sums
    its2 = [orc.snp_update(int(x), 1) for x in held]
    so = [orc.heldout_loglik(int(x)) for x in held]
    assert c == sum(q[1] for q in so) and abs(s - sum(q[0] for q in so)) <= 1e-10 * abs(s), (what, s, so)
    for i, q in enumerate(so):
        assert cnts[i] == q[1] and abs(sums[i] - q[0]) <= 1e-10 * abs(q[0]), (what, i, sums[i], q)
    assert eng.total_passes() == sum(its) + sum(its2)
    assert rel_err(eng.get_lambda(), orc.lambda_()) < 1e-9 and np.array_equal(eng.get_counts(), orc.c_indiv()), what


MODES = [(40_000, 8, "LAUNCH_PER_PASS"), (40_000, 8, "LAUNCH_PER_SNP"), (40_000, 8, "LAUNCH_PER_SCHEDULE"),
         (45_000, 20, "LAUNCH_PER_PASS"), (45_000, 20, "LAUNCH_PER_SNP"), (45_000, 20, "LAUNCH_PER_SCHEDULE"),
         (20_000, 32, "LAUNCH_PER_PASS"), (20_000, 32, "LAUNCH_PER_SNP"), (20_000, 32, "LAUNCH_PER_SCHEDULE")]


@pytest.mark.parametrize("n,k,mode_name", slow_cases(MODES, [MODES[0], MODES[4], MODES[8]]))
def test_late_state_launch_modes(ts, n, k, mode_name):
    """one kernel per pass, ts_resident (per SNP), ts_schedule (per schedule): the literal gamma step (K = 8), the lean one
    (K = 20) and the widest specialised K"""
    mode = getattr(ts, mode_name)
    s, eng, orc = pair(ts, n, k, 5100 + k, l_eff=1e6 if k == 20 else 5e5)
    with eng:
        eng.set_launch_mode(mode)
        want = {ts.LAUNCH_PER_PASS: eng.cfg.max_inner, ts.LAUNCH_PER_SNP: 2, ts.LAUNCH_PER_SCHEDULE: 0}[mode]
        assert eng.launch_info()["kernels_per_snp"] == want
        if mode == ts.LAUNCH_PER_SCHEDULE:
            geo = eng.schedule_geometry()
            assert geo["on_chip_per_thread"] == geo["indivs_per_thread"], geo   # ts_schedule, not ts_hybrid
        check_theta(eng, orc)
        run_and_check(eng, orc, f"{mode_name} n={n} K={k}")
    orc.close()


# (n, k) -> (workgroups, individuals per thread, exchange levels): tests/test_gpu_geometry.py's SHRUNK and ONE_WG
GEOMETRIES = {(10_000, 6): (20, 2, 1), (1_500, 8): (1, 6, 0)}


@pytest.mark.parametrize("n,k", sorted(GEOMETRIES))
def test_late_state_small_shard_geometries(ts, n, k):
    """ts_schedule on the SHRUNK grid and on ONE workgroup: the per-wave (kRepl) form of the epilogue and gamma step"""
    s, eng, orc = pair(ts, n, k, 5300 + k)
    with eng:
        geo = eng.schedule_geometry()
        assert (geo["workgroups"], geo["indivs_per_thread"], geo["exchange_levels"]) == GEOMETRIES[(n, k)], geo
        assert eng.launch_info()["kernels_per_snp"] == 0
        run_and_check(eng, orc, f"geometry n={n} K={k}")
    orc.close()


def _hybrid_on_chip_items(k):
    """(register items, register + LDS items) of ts_hybrid<K> (as in tests/test_gpu_hybrid.py)"""
    reg = 16 if k <= 8 else 13 if k == 9 else 128 // k if k <= 16 else 112 // k if k <= 20 else 112 // k - 1 if k <= 24 else 2 if k <= 28 else 1
    return reg, reg + min(16, (160 * 1024 - 1024 - 200 * k) // (k * 8 * 256))


@pytest.mark.parametrize("k", slow_params([8, 20], [8]))
def test_late_state_hybrid_on_a_small_device(ts, k, monkeypatch):
    """ts_hybrid on four workgroups (TSAMD_TEST_MAX_WORKGROUPS with TSAMD_FLAG_TEST_HOOKS) with three streamed items per thread"""
    monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
    reg, chip = _hybrid_on_chip_items(k)
    n = 4 * 256 * (chip + 3) - 37
    s, eng, orc = pair(ts, n, k, 5500 + k, flags=ts.FLAG_TEST_HOOKS)
    with eng:
        geo = eng.schedule_geometry()
        assert geo["workgroups"] == 4 and geo["indivs_per_thread"] == chip + 3 and geo["on_chip_per_thread"] == chip, geo
        assert eng.launch_info()["kernels_per_snp"] == 0
        run_and_check(eng, orc, f"ts_hybrid K={k}")
    orc.close()


@pytest.mark.parametrize("n,k,flags", slow_cases([(40_000, 8, 0), (45_000, 20, 0), (3_000, 8, "hooks")], [(40_000, 8, 0)]))
def test_late_state_validation_block(ts, n, k, flags, monkeypatch):
    """ts_holblock (and, on four workgroups above ts_schedule's capacity, ts_hybhol): the validation-mode schedule batched,
    against the oracle and bit for bit the entry-by-entry path (TSAMD_HOLBLOCK=0)"""
    fl = 0
    if flags == "hooks":   # above ts_schedule's capacity on four workgroups: ts_hybhol
        monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "4")
        fl = ts.FLAG_TEST_HOOKS
        n = 4 * 256 * (_hybrid_on_chip_items(k)[1] + 3) - 37
    outs = []
    for block in (True, False):
        monkeypatch.setenv("TSAMD_HOLBLOCK", "1" if block else "0")
        s, eng, orc = pair(ts, n, k, 5700 + k, flags=fl)
        with eng:
            assert (eng.holblock_info()["batch"] > 0) == block
            run_and_check(eng, orc, f"validation block={block} n={n} K={k}")
            info = eng.holblock_info()
            assert (info["launches"] > 0) == block, info
            outs.append((eng.get_lambda(), eng.get_gamma(), eng.get_counts(), eng.total_passes(), eng.pass_histogram()))
        orc.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_late_state_wide_k(ts):
    """K = 40: the run-time-K kernels, one launch per pass"""
    n, k = 5_000, 40
    s, eng, orc = pair(ts, n, k, 5900)
    with eng:
        assert eng.launch_info()["kernels_per_snp"] == eng.cfg.max_inner
        check_theta(eng, orc)
        run_and_check(eng, orc, "K = 40")
    orc.close()


def test_late_state_nodekappa(ts):
    """nodekappa = 0.7: the pow() path of the first pass' gamma step (gamma_step_one), where the large planted c_n matter
    (the resident kernels take nodekappa == 0.5 only: one launch per pass)"""
    n, k = 20_000, 8
    s, eng, orc = pair(ts, n, k, 6100, eng_over={"nodekappa": 0.7}, orc_over={"nodekappa": 0.7})
    with eng:
        eng.set_launch_mode(ts.LAUNCH_PER_PASS)
        assert eng.launch_info()["kernels_per_snp"] == eng.cfg.max_inner
        run_and_check(eng, orc, "nodekappa 0.7")
    orc.close()


@pytest.mark.parametrize("n,k", slow_cases([(40_000, 8), (45_000, 20)], [(40_000, 8)]))
def test_late_state_single_update(ts, n, k):
    """max_inner = 1: one SNP, then a validation-mode entry that applies its deferred gamma step -- rel 1e-11"""
    s, eng, orc = pair(ts, n, k, 6300 + k, eng_over={"max_inner": 1}, orc_over={"online_iterations": 1})
    with eng:
        eng.snp_update(3)
        eng.snp_update(5, 1)
        eng.synchronize()
        assert orc.snp_update(3) == 1 and orc.snp_update(5, 1) == 1
        assert eng.total_passes() == 2
        assert rel_err(eng.get_lambda(), orc.lambda_()) < 1e-11
        assert rel_err(eng.get_gamma(), orc.gamma()) < 1e-11
        assert np.array_equal(eng.get_counts(), orc.c_indiv())
        assert not np.array_equal(eng.get_gamma(), s.gamma)
    orc.close()
