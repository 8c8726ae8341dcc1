"""Sharded engine across several processes.  The development box has one GPU, so the
ranks share device 0: that exercises the whole multi-rank protocol (shard slicing, epoch
tagged peer-to-peer exchange through IPC-mapped buffers, replicated epilogue, graph
replay) except the xGMI hop itself.  At most six processes may hold a shared GPU at once, this
one included, so no case runs more than five ranks; the eight-rank shapes of a node
keep their per-rank geometry there (each rank gets 1/world of the device: TSAMD_DEVICE_SHARE)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as op
from helpers import init_gamma, pack_bed, psd_genotypes, rel_err, usable_cores

pytestmark = [pytest.mark.gpu, pytest.mark.spawns]
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _n_devices():
    """GPUs on this box (counting does not initialise HIP in this process on this image)."""
    import torch

    return torch.cuda.device_count()


def _run_ranks(tmp_path, mode, world, n, l, k, seed, nsnp, extra_env=None, ok_codes=(0,), _retry=True):
    port = _free_port()
    procs = []
    distinct = _n_devices() >= world  # a multi-GPU node: one rank per GPU (the xGMI hop); else all share device 0
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), TS_DEVICE=str(rank if distinct else 0), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if not distinct:
            env["TSAMD_DEVICE_SHARE"] = str(world)   # the ranks' resident kernels (ts_schedule) must fit device 0 together
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "multirank_worker.py"), str(tmp_path), mode,
                                       str(n), str(l), str(k), str(seed), str(nsnp)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=110)   # (the slowest case takes 28 s; a rendezvous that never completes must not cost the suite 3 minutes)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            tails = [q.communicate()[0] or "" for q in procs]
            # The ranks' gloo rendezvous (torch.distributed, before any GPU work) hung once in ~150 launches on the GPU box -- no
            # rank ever printed "[Gloo] Rank r is connected to ...".  That is the test harness, not the engine: start the ranks
            # again, once, on a fresh port.  A hang AFTER the rendezvous is the engine's and fails the test.
            if _retry and not any("is connected to" in t for t in tails):
                return _run_ranks(tmp_path, mode, world, n, l, k, seed, nsnp, extra_env, ok_codes, _retry=False)
            raise AssertionError("ranks timed out after their rendezvous:\n" + "\n".join(f"---- rank {r} ----\n{t[-1500:]}" for r, t in enumerate(tails)))
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode in ok_codes, f"rank {rank} failed:\n{out[-3000:]}\n" + "".join(
            f"---- rank {r} (exit code {q.returncode}) ----\n{o[-1500:]}\n" for r, (q, o) in enumerate(zip(procs, outs)) if r != rank)
    if any(p.returncode != 0 for p in procs):
        return [f"[exit code {p.returncode}]\n{o}" for p, o in zip(procs, outs)]
    return [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]


def _oracle_run(n, l, k, seed, nsnp, **over):
    y, _, _ = psd_genotypes(n, l, k, seed, 0.03)
    orc = op.Oracle(n, l, k, nthreads=usable_cores() if n * k > 100_000 else 1, **over)
    orc.load_bed_payload(pack_bed(y))
    orc.set_gamma(init_gamma(n, k, seed + 1))
    rng = np.random.default_rng(seed + 2)
    for loc in rng.choice(l, size=max(1, l // 8), replace=False):
        cand = np.nonzero(y[loc] != 3)[0]
        orc.set_heldout(int(loc), rng.choice(cand, size=max(1, n // 50), replace=False))
    locs = np.random.default_rng(seed + 3).integers(0, l, size=nsnp)
    its = [orc.snp_update(int(loc)) for loc in locs]
    return orc, its


def _assert_ranks_match(res, orc, its):
    for r in res:
        assert rel_err(r["lam"], orc.lambda_()) < 1e-9
        assert rel_err(r["gamma"], orc.gamma()) < 1e-9
        assert np.array_equal(r["cnt"][:, 0], orc.c_indiv())
        assert int(r["its"][0]) == its[5]
        assert int(r["passes"]) == sum(its)
    for r in res[1:]:   # replicated state is bitwise identical on every rank
        assert np.array_equal(r["lam"], res[0]["lam"])


@pytest.mark.parametrize("world,n,k,kps", [(2, 3000, 6, 10), (4, 5003, 8, 10), (3, 1000, 3, 10), (2, 4000, 20, 0), (2, 2500, 40, 10), (5, 5626, 8, 10)])
def test_p2p_sharded_matches_oracle(tmp_path, world, n, k, kps):
    """Small shards over the peer-to-peer exchange.  kps pins the kernel sequence each case means to exercise (asserted in
    the worker): shards that fill fewer than 8 workgroups -- and K = 40, above the specialised kernels -- run ONE LAUNCH PER
    PASS with the rows pushed to every rank (10 kernels per SNP); (2, 4000, 20) fills 8 workgroups per rank and runs
    ts_schedule (0).  A small shard must never be handed to ts_hybrid, which is for shards ABOVE the register capacity."""
    l, seed, nsnp = 32, 91, 40
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env={"TS_EXPECT_KPS": str(kps)})
    orc, its = _oracle_run(n, l, k, seed, nsnp)
    _assert_ranks_match(res, orc, its)
    assert all(int(r["kps"]) == kps for r in res)


def test_p2p_launch_per_pass_with_large_shards_on_a_shared_device(tmp_path):
    """4 ranks x 100 000 individuals, K = 20, one launch per pass -- the sequence a sharded recovery replays through.  A
    first pass at K = 20 is register-bound (one workgroup per compute unit); with all ranks on ONE device each rank's
    first pass used to fill it and keep its peers' previous passes off the device until its bounded wait gave up
    ("timed out waiting for a peer (epoch 2)", round 4's 4-rank rehearsal).  Ranks that share a device now get their share of
    its workgroups (configure_launch); on a node with a GPU per rank nothing changes."""
    world, n, l, k, seed, nsnp = 4, 400_000, 16, 20, 71, 10
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env={"TS_LAUNCH_MODE": "0", "TS_EXPECT_KPS": "10"})
    orc, its = _oracle_run(n, l, k, seed, nsnp)
    _assert_ranks_match(res, orc, its)


@pytest.mark.parametrize("world,flags", [(2, 0), (3, 0), (2, 2), (4, 2)])
def test_p2p_early_convergence_with_a_lagging_rank(tmp_path, world, flags):
    """SNPs that converge after 1..9 passes leave launches that neither wait for nor publish
    rows; the first pass that follows must not overwrite an exchange slot a lagging peer still
    reads (Xchg::prog guard).  One rank is stalled 200 us between every flag wait and its row
    reads; graph replay (flags 0) and eager launches (TSAMD_FLAG_NO_GRAPH = 2)."""
    n, l, k, seed, nsnp = 600, 32, 3, 5, 120
    thresh = 1.0
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp,
                     extra_env={"TS_CONV_THRESH": str(thresh), "TS_DELAY_RANK": str(world - 1), "TS_FLAGS": str(flags)})
    orc, its = _oracle_run(n, l, k, seed, nsnp, meanchangethresh=thresh)
    assert len(set(its)) >= 4 and min(its) < 10, f"pass counts do not vary: {sorted(set(its))}"
    _assert_ranks_match(res, orc, its)


@pytest.mark.parametrize("world,max_inner", [(2, 1), (3, 2)])
def test_p2p_small_pass_caps(tmp_path, world, max_inner):
    """Pass caps of 1 and 2 over the peer-to-peer exchange: every (or every other) launch is a first
    pass, whose workgroups other than 0 store their rows without having waited for peer rows (fast
    path) and therefore rely on the progress guard; one rank lags."""
    n, l, k, seed, nsnp = 3000, 32, 4, 23, 60
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp,
                     extra_env={"TS_MAX_INNER": str(max_inner), "TS_DELAY_RANK": "0", "TS_DELAY_US": "100"})
    orc, its = _oracle_run(n, l, k, seed, nsnp, online_iterations=max_inner)
    _assert_ranks_match(res, orc, its)


@pytest.mark.parametrize("world,n,k,thresh,max_inner", [(2, 40_000, 8, None, None), (4, 70_000, 5, None, None),
                                                        (2, 60_000, 8, 8.0, None), (3, 50_000, 3, None, 3),
                                                        (2, 40_000, 12, None, None), (2, 60_000, 20, 30.0, None),
                                                        (4, 90_000, 16, None, None), (3, 50_000, 32, None, 4),
                                                        (5, 125_000, 20, None, None),
                                                        # round 6 -- what BASELINE config 4 (K = 8) runs on 4 and 8 GPUs: ts_schedule<8, true, 16>,
                                                        # <8, true, 32> (level 2 of the exchange polled in two halves by two waves), K = 6 likewise,
                                                        # and the full-size instantiation <8, false, 32>: 16 individuals per thread on each rank's
                                                        # share of the device (config 4's 130 000 per rank on 8 ranks; 5 ranks get 48 workgroups each here: 196 000 per rank)
                                                        (4, 120_000, 8, None, None), (5, 200_000, 8, None, None), (5, 200_000, 6, 20.0, None),
                                                        (5, 980_000, 8, None, None),
                                                        # the polls that take their row pairs in two goes (res_seq_halves; 5 ranks: 40 rows, the second half
                                                        # partly filled; a node's 8 ranks fill both): K = 16 (two waves per block, 8 + 8 pairs), K = 18 (one
                                                        # wave per block, 16 + 16), and K = 14 (8 items per thread when sharded), on the 12 500-individual
                                                        # shards of the 8-rank shape -- slow: TS_RUN_SLOW=1
                                                        pytest.param(5, 62_500, 16, None, None, marks=pytest.mark.slow),
                                                        pytest.param(5, 62_500, 18, None, None, marks=pytest.mark.slow),
                                                        pytest.param(5, 62_500, 14, None, None, marks=pytest.mark.slow)])
def test_sharded_schedule_kernel_matches_oracle(tmp_path, world, n, k, thresh, max_inner):
    """Shards of at least 8 workgroups, K <= 32: every rank runs the whole schedule as ONE launch (ts_schedule) whose
    in-launch exchange spans the ranks -- group sums stored into every rank's buffer, each rank polls its own copy.
    Against the oracle; replicated state bitwise equal on all ranks; with SNPs that stop after differing pass counts and
    with a pass cap of 3.  The same shards with one launch per pass (TS_LAUNCH_MODE=0) must agree to rounding."""
    l, seed, nsnp = 24, 77, 40
    env, over = {"TS_EXPECT_KPS": "0", "TS_EXPECT_RECOVERIES": "0"}, {}   # (a launch that was silently replayed one launch per pass would not test ts_schedule)
    if world >= 5:
        nsnp = 24   # (five or more processes time-slicing one GPU's queues run a few updates per second: the suite's time budget)
    if n > 500_000:     # (the full-size case)
        if _n_devices() >= world:
            pytest.skip("the full-size K <= 8 instantiation needs the ranks to share one device (16 individuals per thread)")
        nsnp = 24
        env["TS_EXPECT_PER_THREAD"] = "16"   # ts_schedule<8, false, 32>: no item of a thread unused
    if thresh is not None:
        env["TS_CONV_THRESH"] = str(thresh)
        over["meanchangethresh"] = thresh
    if max_inner is not None:
        env["TS_MAX_INNER"] = str(max_inner)
        over["online_iterations"] = max_inner
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env=env)
    orc, its = _oracle_run(n, l, k, seed, nsnp, **over)
    if thresh is not None:
        assert len(set(its)) >= 2 and min(its) < 10, f"pass counts do not vary: {sorted(set(its))}"
    _assert_ranks_match(res, orc, its)
    assert all(int(r["kps"]) == 0 for r in res)
    if world == 2 and thresh is None and n < 100_000:
        (tmp_path / "pp").mkdir()
        ref = _run_ranks(tmp_path / "pp", "p2p", world, n, l, k, seed, nsnp,
                         extra_env={"TS_LAUNCH_MODE": "0", "TS_EXPECT_KPS": "10"})
        assert rel_err(res[0]["lam"], ref[0]["lam"]) < 1e-11 and rel_err(res[0]["gamma"], ref[0]["gamma"]) < 1e-11
        assert np.array_equal(res[0]["cnt"], ref[0]["cnt"])


@pytest.mark.parametrize("world,n,k,thresh", [(2, 60_000, 8, 8.0), (4, 90_000, 16, None), (3, 40_000, 5, None)])
def test_sharded_schedule_kernel_three_levels(tmp_path, world, n, k, thresh):
    """The same with TSAMD_SCHEDULE_GATHER=leaders: only a rank's eight group leaders poll the world x 8 rows the ranks send
    each other; every other workgroup takes the total from its own group's leader (one local hop more, far less polling of
    the fine-grained buffer).  Against the oracle; replicated state bitwise equal on all ranks; the same bits as the
    two-level exchange (both add the rows in (rank, group) order)."""
    l, seed, nsnp = 24, 77, 40
    env, over = {"TS_EXPECT_KPS": "0", "TS_EXPECT_RECOVERIES": "0", "TSAMD_SCHEDULE_GATHER": "leaders"}, {}
    if thresh is not None:
        env["TS_CONV_THRESH"] = str(thresh)
        over["meanchangethresh"] = thresh
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env=env)
    orc, its = _oracle_run(n, l, k, seed, nsnp, **over)
    _assert_ranks_match(res, orc, its)
    if world == 2:
        (tmp_path / "two").mkdir()
        env2 = dict(env, TSAMD_SCHEDULE_GATHER="all")
        ref = _run_ranks(tmp_path / "two", "p2p", world, n, l, k, seed, nsnp, extra_env=env2)
        assert np.array_equal(res[0]["lam"], ref[0]["lam"]) and np.array_equal(res[0]["gamma"], ref[0]["gamma"])


@pytest.mark.parametrize("world,n,k,thresh", [(2, 600_000, 20, None),
                                              # K <= 16 on 3 ranks: ts_hybhol<8, 16> adds the ranks' rows in ts_hybrid<8, 16>'s order (halves of 16 rows) -- slow
                                              pytest.param(3, 1_200_000, 8, None, marks=pytest.mark.slow)])
def test_sharded_hybrid_validation_block_is_batched_and_matches(tmp_path, world, n, k, thresh):
    """The same on shards ABOVE the register capacity (every rank runs ts_hybrid): the block runs as ts_hybhol<K, WR> launches --
    a sub-batch of locations shares one sweep of the streamed weights, the batch one exchange across the ranks.  Against the
    oracle, and bit for bit against the same run with TSAMD_HOLBLOCK=0 (entry by entry inside ts_hybrid)."""
    l, seed, nsnp, nhol = 16, 83, 12, 14
    env, over = {"TS_EXPECT_KPS": "0", "TS_EXPECT_HYBRID": "1", "TS_EXPECT_RECOVERIES": "0", "TS_HOL_LOCS": str(nhol), "TS_EXPECT_HOLBLOCKS": "1"}, {}
    if thresh is not None:
        env["TS_CONV_THRESH"] = str(thresh)
        over["meanchangethresh"] = thresh
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env=env)
    orc, its = _oracle_run(n, l, k, seed, nsnp, **over)
    locs = np.random.default_rng(seed + 3).integers(0, l, size=nsnp)
    its_hol = [orc.snp_update(int(x), 1) for x in range(nhol)]
    its2 = its + its_hol + [orc.snp_update(int(x)) for x in locs[:4]]
    for r in res:
        assert rel_err(r["lam"], orc.lambda_()) < 1e-9 and rel_err(r["gamma"], orc.gamma()) < 1e-9
        assert np.array_equal(r["cnt"][:, 0], orc.c_indiv()) and int(r["passes"]) == sum(its2)
    for r in res[1:]:
        assert np.array_equal(r["lam"], res[0]["lam"])
    (tmp_path / "single").mkdir()
    ref = _run_ranks(tmp_path / "single", "p2p", world, n, l, k, seed, nsnp,
                     extra_env=dict(env, TSAMD_HOLBLOCK="0", TS_EXPECT_HOLBLOCKS="0"))
    assert not any(int(r["recoveries"]) for r in res + ref)   # (a replayed launch would compare the launch-per-pass path, not ts_hybhol)
    assert np.array_equal(res[0]["lam"], ref[0]["lam"]) and np.array_equal(res[0]["gamma"], ref[0]["gamma"])


@pytest.mark.parametrize("world,n,k,thresh", [(2, 600_000, 20, 15.0), (3, 1_200_000, 8, None)])
def test_sharded_hybrid_kernel_matches_oracle(tmp_path, world, n, k, thresh):
    """Shards above ts_schedule's register capacity (with the ranks sharing one GPU each gets CUs / world workgroups: 128 x 256 x 5
    individuals at K = 20 for two ranks): every rank runs ts_hybrid<K, WR> -- weights in registers + LDS, the rest streamed
    (600 000 at K = 20: two of a thread's ten individuals; 1 200 000 at K = 8 on three ranks: none, LDS items only) -- with the
    in-launch exchange spanning the ranks.  BASELINE config 5's 2-GPU point (500 000 per rank) takes this route on a node."""
    l, seed, nsnp = 24, 79, 24
    env, over = {"TS_EXPECT_KPS": "0", "TS_EXPECT_HYBRID": "1", "TS_EXPECT_RECOVERIES": "0"}, {}   # (round 6: until the workgroup cap of ranks sharing a device became
    # XCD-aware, the 3-rank case lost its launch to the co-residency check and silently tested the REPLAY, not ts_hybrid)
    if thresh is not None:
        env["TS_CONV_THRESH"] = str(thresh)
        over["meanchangethresh"] = thresh
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env=env)
    orc, its = _oracle_run(n, l, k, seed, nsnp, **over)
    if thresh is not None:
        assert len(set(its)) >= 2, f"pass counts do not vary: {sorted(set(its))}"
    _assert_ranks_match(res, orc, its)


@pytest.mark.parametrize("world,n,k,thresh", [(2, 40_000, 8, None), (4, 90_000, 16, None), (3, 50_000, 5, 6.0),
                                              # round 6: ts_holblock<8, 32> / <20, 32> on 5 ranks (configs 4 and 5 run 8; the wide rows' level 2
                                              # polled in two halves of 32 rows)
                                              (5, 200_000, 8, None), (5, 125_000, 20, 8.0),
                                                        pytest.param(5, 62_500, 16, None, marks=pytest.mark.slow),     # halves of 32 rows, K <= 16: segmented order
                                                        pytest.param(5, 100_000, 12, None, marks=pytest.mark.slow)])   # 5 ranks: 40 rows, the second half partly filled
def test_sharded_validation_block_is_batched_and_matches(tmp_path, world, n, k, thresh):
    """A validation-mode schedule on a sharded context that runs ts_schedule: every rank runs it as ts_holblock<K, WR> launches
    (wide rows exchanged across the ranks through Xchg::res_wide).  Against the oracle, and bit for bit against the same run
    with TSAMD_HOLBLOCK=0 (entry by entry inside ts_schedule)."""
    l, seed, nsnp, nhol = 24, 81, 20, 21
    if world >= 5:
        nsnp, nhol = 12, 18   # (see test_sharded_schedule_kernel_matches_oracle: a few updates per second with 5+ ranks on one GPU)
    env, over = {"TS_EXPECT_KPS": "0", "TS_EXPECT_RECOVERIES": "0", "TS_HOL_LOCS": str(nhol), "TS_EXPECT_HOLBLOCKS": "1"}, {}
    if thresh is not None:
        env["TS_CONV_THRESH"] = str(thresh)
        over["meanchangethresh"] = thresh
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env=env)
    orc, its = _oracle_run(n, l, k, seed, nsnp, **over)
    locs = np.random.default_rng(seed + 3).integers(0, l, size=nsnp)
    its_hol = [orc.snp_update(int(x), 1) for x in range(nhol)]
    its2 = its + its_hol + [orc.snp_update(int(x)) for x in locs[:4]]
    if thresh is not None:
        assert len(set(its_hol)) >= 2, its_hol
    for r in res:
        assert rel_err(r["lam"], orc.lambda_()) < 1e-9 and rel_err(r["gamma"], orc.gamma()) < 1e-9
        assert np.array_equal(r["cnt"][:, 0], orc.c_indiv()) and int(r["passes"]) == sum(its2)
    for r in res[1:]:
        assert np.array_equal(r["lam"], res[0]["lam"])
    if world >= 5 and k > 16:
        return   # (the suite's time budget: rows of K >= 17 are added in one order everywhere -- no halves; 5 ranks x K = 8 runs the comparison)
    (tmp_path / "single").mkdir()
    ref = _run_ranks(tmp_path / "single", "p2p", world, n, l, k, seed, nsnp,
                     extra_env=dict(env, TSAMD_HOLBLOCK="0", TS_EXPECT_HOLBLOCKS="0"))
    assert np.array_equal(res[0]["lam"], ref[0]["lam"]) and np.array_equal(res[0]["gamma"], ref[0]["gamma"])


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_switch_launch_modes_mid_run(tmp_path, world):
    """ts_schedule (in-launch exchange across the ranks) -> one launch per pass (epoch-tagged peer-to-peer rows with the
    progress guard) -> ts_schedule again on the same contexts: the State and the epoch one sequence leaves are the other's
    start on every rank."""
    n, l, k, seed, nsnp = 50_000, 24, 6, 19, 44
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, extra_env={"TS_SWITCH_MODES": "1", "TS_EXPECT_KPS": "0"})
    orc, its = _oracle_run(n, l, k, seed, nsnp)
    _assert_ranks_match(res, orc, its)


@pytest.mark.parametrize("world,n,k", [(2, 40_000, 8), (3, 30_000, 20)])
def test_sharded_schedule_that_cannot_be_resident_is_replayed_on_every_rank(tmp_path, world, n, k):
    """A tenant holds compute units when the ranks' ts_schedule launches start: the entry exchange (which spans the ranks)
    times out on every rank with every rank's state intact; every rank lowers itself to one launch per pass and replays the
    same schedule from its journal -- the results are those of an undisturbed run."""
    l, seed, nsnp = 32, 93, 30
    res = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp,
                     extra_env={"TS_EXPECT_KPS": "0", "TS_OCCUPY": "200,4500", "TS_EXPECT_RECOVERIES": "1"})
    orc, its = _oracle_run(n, l, k, seed, nsnp)
    _assert_ranks_match(res, orc, its)


def test_split_commit_verdict_is_never_silent(tmp_path):
    """The residual window of the sharded recovery (include/tsamd.h: best effort): one rank posts its commit exchange 1.3 s
    late (test hook), after its peer's bounded wait of 1 s has given up "intact".  The late rank finds the peer's row, passes,
    starts to modify state and times out at its first real exchange; the peer replays and waits for a rank that does not.
    EVERY rank must end with an error (TSAMD_ECOMM) -- no rank may finish as if nothing had happened."""
    world, n, l, k, seed, nsnp = 2, 40_000, 16, 8, 97, 12
    outs = _run_ranks(tmp_path, "p2p", world, n, l, k, seed, nsnp, ok_codes=(0, 1),
                      extra_env={"TS_EXPECT_KPS": "0", "TS_DELAY_RANK": "1", "TS_DELAY_US": "1300000"})
    assert isinstance(outs[0], str), "a rank finished with exit code 0 although the commit verdict was split"
    for rank, out in enumerate(outs):
        assert not out.startswith("[exit code 0]") and "TsamdError" in out, f"rank {rank}:\n{out[-1500:]}"


def test_rccl_two_ranks_matches_oracle(tmp_path):
    """The RCCL all-reduce exchange with more than one rank.  On a box with fewer GPUs than ranks
    RCCL refuses the communicator (two ranks on one device): skipped there, with RCCL's message."""
    world, n, l, k, seed, nsnp = 2, 3000, 32, 6, 91, 40
    res = _run_ranks(tmp_path, "rccl", world, n, l, k, seed, nsnp, ok_codes=(0, 77))
    if isinstance(res[0], str):
        pytest.skip("RCCL communicator with 2 ranks unavailable on this box: " + " | ".join(ln for ln in res[0].splitlines() if "unavailable" in ln or "WARN" in ln or "rror" in ln)[:600])
    orc, its = _oracle_run(n, l, k, seed, nsnp)
    _assert_ranks_match(res, orc, its)


def test_p2p_long_schedule_matches_single_gpu(tmp_path):
    """Stress: 2 ranks, 100K individuals, 300 updates through the graph-replayed
    peer-to-peer path (3000 epoch-tagged exchanges) against the single-GPU engine."""
    n, l, k, seed, nsnp = 100_000, 48, 8, 17, 300
    res = _run_ranks(tmp_path, "p2p", 2, n, l, k, seed, nsnp)   # children first: this process has not touched HIP yet
    import terastructure_amd as ts

    y, _, _ = psd_genotypes(n, l, k, seed, 0.03)
    with ts.Engine(n, l, k) as eng:
        eng.upload_bed(pack_bed(y))
        eng.set_gamma(init_gamma(n, k, seed + 1))
        rng = np.random.default_rng(seed + 2)
        for loc in rng.choice(l, size=max(1, l // 8), replace=False):
            cand = np.nonzero(y[loc] != 3)[0]
            eng.set_heldout(int(loc), rng.choice(cand, size=max(1, n // 50), replace=False))
        locs = np.random.default_rng(seed + 3).integers(0, l, size=nsnp).astype(np.uint32)
        eng.run_schedule(locs)
        eng.synchronize()
        lam, gam, cnt, passes = eng.get_lambda(), eng.get_gamma(), eng.get_counts(), eng.total_passes()
    for r in res:
        assert rel_err(r["lam"], lam) < 1e-9
        assert rel_err(r["gamma"], gam) < 1e-9
        assert np.array_equal(r["cnt"][:, 0], cnt)
        assert int(r["passes"]) == passes
    assert np.array_equal(res[0]["lam"], res[1]["lam"])
