"""tsamd_fold_in: fit the individuals' gamma against a fixed lambda; tsamd_set_lambda_range.

The reference is numpy fp64 with scipy.special.digamma, from reads of the engine only -- get_gamma(), get_elogbeta()
(exponentiated: the eb the context stores) and download_bed() (which shows held-out entries as missing, as wanted):
    w_k = exp(psi(gamma_k) - psi(sum_k gamma_k)),  S0_j = sum_k w_k eb[j][k][0],  S1_j = sum_k w_k eb[j][k][1]
    gamma'_k = alpha + w_k sum_{j listed, code != 01} (y eb[j][k][0] / S0_j + (2 - y) eb[j][k][1] / S1_j)
    change = mean_k |gamma' - gamma| / mean_k gamma';  an individual is frozen once change < tol.

Tolerances: gamma to relative 1e-9 (the project's GPU <-> oracle parity tolerance; the numpy fixed point computed in two
summation orders differs by 6e-15 ... 3e-14 after 30 iterations and <= 1e-12 after 100); the invariant sum_k gamma =
k alpha + 2 M to relative 1e-11 (the bound of the loglik tests for <= 4 099 terms); segment counts and shards against each
other to relative 1e-12; everything else bit for bit.

Shapes: the issue's list, with N raised so that every individuals-per-thread figure (16 / 8 / 4 / 2 / 1 at K <= 2 / 4 / 8 /
16 / 32, tiles of 4096 / 2048 / 1024 / 512 / 256) sees more than one tile and a tile that ends in padding, plus one shape
at K = 12 for the figure 2, and the run-time-K kernel at K = 33 and 128.  The state export carries the real individuals
only; that the padding individuals keep their state is part of the bit-for-bit comparison of the schedules that follow."""
import numpy as np
import pytest
from scipy.special import digamma

from helpers import init_gamma, unpack_bed
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

EINVAL = -1
SHAPES = [(2100, 64, 3), (4200, 40, 1), (1030, 33, 8), (4099, 24, 20), (2050, 16, 32), (700, 12, 33), (600, 8, 128), (700, 20, 12)]


def trained_lambda(rng, beta):
    """lambda as after training: 1 + c beta, 1 + c (1 - beta) with a per-location c in (0, 200)"""
    c = rng.uniform(0.0, 200.0, size=(beta.shape[0], 1))
    return np.stack([1.0 + c * beta, 1.0 + c * (1.0 - beta)], axis=2)


def synth_engine(ts, n, l, k, seed, flags=0, rank=0, world=1, gamma=True):
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.full(k, 0.3), size=n)
    beta = rng.uniform(0.05, 0.95, size=(l, k))
    eng = ts.Engine(n, l, k, flags=flags, rank=rank, world=world)
    b, c = eng.shard_begin, eng.shard_count
    eng.synth_genotypes(theta[b:b + c], beta, seed=seed, missing_rate=0.1)
    eng.set_lambda_range(trained_lambda(rng, beta))
    if gamma:
        eng.set_gamma(init_gamma(n, k, seed + 1)[b:b + c])
    return eng


def reference(eng, locs, max_iters, tol, snapshots=()):
    """dict(gamma, iters, change, near, snaps): the fixed-point iteration on the engine's own gamma, eb and stored codes;
    near[n]: some change of n up to its stopping update lies within relative 1e-6 of tol; snaps[i]: gamma after i updates"""
    locs = np.arange(eng.l) if locs is None else np.asarray(locs, dtype=np.int64)
    g = eng.get_gamma().copy()
    eb = np.exp(eng.get_elogbeta())[locs]  # [J][k][2]
    e0, e1 = eb[:, :, 0], eb[:, :, 1]
    cols = {int(x): unpack_bed(eng.download_bed(int(x))[None, :], eng.shard_count)[0] for x in set(locs.tolist())}
    y = np.stack([cols[int(x)] for x in locs], axis=1)  # [n][J]
    mom = np.where(y == 3, 0.0, y.astype(np.float64))
    dad = np.where(y == 3, 0.0, 2.0 - y.astype(np.float64))
    alpha = eng.cfg.alpha
    n = g.shape[0]
    act = np.ones(n, dtype=bool)
    iters, change, near, snaps = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n, dtype=bool), {}
    for it in range(1, max_iters + 1):
        idx = np.nonzero(act)[0]
        if idx.size == 0:
            break
        ga = g[idx]
        w = np.exp(digamma(ga) - digamma(ga.sum(axis=1, keepdims=True)))
        c0, c1 = mom[idx] / (w @ e0.T), dad[idx] / (w @ e1.T)
        gn = alpha + w * (c0 @ e0 + c1 @ e1)
        ch = np.mean(np.abs(gn - ga), axis=1) / np.mean(gn, axis=1)
        g[idx], change[idx] = gn, ch
        iters[idx] += 1
        if tol > 0:
            near[idx] |= np.abs(ch - tol) <= 1e-6 * tol
            act[idx[ch < tol]] = False
        if it in snapshots:
            snaps[it] = g.copy()
    return dict(gamma=g, iters=iters, change=change, near=near, snaps=snaps)


def max_rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("n,l,k", SHAPES)
def test_parity_at_a_fixed_iteration_count(ts, n, l, k):
    with synth_engine(ts, n, l, k, 60 + k) as eng:
        rng = np.random.default_rng(k)
        locs = rng.permutation(l)[:max(3, l // 2)].astype(np.uint32)
        locs = np.concatenate([locs, locs[1:2], [l - 1]]).astype(np.uint32)  # unsorted, with a repeat
        assert len(set(locs.tolist())) < len(locs)
        g0 = eng.get_gamma()
        for which in (locs, None):
            ref = reference(eng, which, 30, 0.0, snapshots=(1, 5, 30))
            for iters in (1, 5, 30):
                eng.set_gamma(g0)
                out = eng.fold_in(which, max_iters=iters, tol=0.0)
                got = eng.get_gamma()
                err = max_rel(got, ref["snaps"][iters])
                print(f"N={n} L={l} K={k} {'list' if which is not None else 'all'} iters={iters}: max rel |gpu - ref| = {err:.3e}")
                assert err <= 1e-9
                assert np.all(out["iters"] == iters) and out["iters_run"] == iters and out["n_converged"] == 0
            eng.set_gamma(g0)


@pytest.mark.parametrize("n,l,k", [(4200, 40, 1), (1030, 33, 8), (700, 12, 33)])
def test_invariant_sum_of_gamma(ts, n, l, k):
    with synth_engine(ts, n, l, k, 80 + k, gamma=(k != 8)) as eng:  # (K = 8: from tsamd_create's gamma = 1)
        locs = np.array([5, 2, 2, l - 1, 0, 7], dtype=np.uint32)
        alpha = eng.cfg.alpha
        # individual 3: every listed entry held out; individual n - 1: one of them
        for loc in sorted(set(locs.tolist())):
            eng.set_heldout(loc, np.array([3, n - 1] if loc == 2 else [3], dtype=np.uint32))
        m = eng.train_loglik(locs)["indiv_counts"].astype(np.float64)
        assert m[3] == 0 and m.max() > 0
        for iters in (1, 4):
            out = eng.fold_in(locs, max_iters=iters, tol=0.0)
            g = eng.get_gamma()
            want = k * alpha + 2.0 * m
            err = max_rel(g.sum(axis=1), want)
            print(f"K={k} iters={iters}: max rel |sum_k gamma - (k alpha + 2 M)| = {err:.3e}")
            assert err <= 1e-11
            if k == 1:
                assert max_rel(g[:, 0], alpha + 2.0 * m) <= 1e-11
            assert np.all(g[3] == alpha)
        # with tol > 0 the individual without entries moves to alpha, then not at all: frozen by its second update
        eng.set_gamma(np.full((n, k), 2.5))
        out = eng.fold_in(locs, max_iters=50, tol=1e-6)
        assert out["iters"][3] == 2 and out["change"][3] == 0.0 and np.all(eng.get_gamma()[3] == alpha)


def test_convergence_and_freezing(ts):
    n, l, k, tol = 300, 257, 8, 1e-4
    with synth_engine(ts, n, l, k, 91) as eng:
        g0 = eng.get_gamma()
        ref = reference(eng, None, 400, tol)
        out = eng.fold_in(max_iters=400, tol=tol)
        got = eng.get_gamma()
        keep = ~ref["near"]
        print(f"left out (a change within 1e-6 of tol): {int((~keep).sum())} of {n}; iterations {out['iters'].min()} .. {out['iters'].max()}, "
              f"run {out['iters_run']}, converged {out['n_converged']}")
        assert (~keep).mean() <= 0.05
        assert np.array_equal(out["iters"][keep], ref["iters"][keep])
        err = max_rel(got[keep], ref["gamma"][keep])
        print(f"max rel |gpu - ref| at convergence = {err:.3e}")
        assert err <= 1e-9
        assert out["iters_run"] == out["iters"].max() and out["n_converged"] == int((out["change"] < tol).sum())
        assert np.all((out["change"] < tol) | (out["iters"] == 400))
        # freezing: an individual's result is what the same call gives when it stops at that individual's last update
        for v in np.unique(out["iters"]):
            eng.set_gamma(g0)
            cut = eng.fold_in(max_iters=int(v), tol=tol)
            rows = out["iters"] == v
            assert eng.get_gamma()[rows].tobytes() == got[rows].tobytes(), v
            assert np.array_equal(cut["iters"][rows], out["iters"][rows]) and cut["change"][rows].tobytes() == out["change"][rows].tobytes()


def test_reproducible_and_independent_of_segments_and_shards(ts, monkeypatch):
    n, l, k = 1030, 300, 8
    monkeypatch.delenv("TSAMD_TEST_FOLDIN_SEGMENTS", raising=False)
    engines = [synth_engine(ts, n, l, k, 17, flags=ts.FLAG_TEST_HOOKS)] + [synth_engine(ts, n, l, k, 17, rank=r, world=2) for r in (0, 1)]
    try:
        eng = engines[0]
        g0 = eng.get_gamma()
        res = {}
        for name, segs in (("device", None), ("again", None), ("one", "1"), ("many", "37")):
            if segs is None:
                monkeypatch.delenv("TSAMD_TEST_FOLDIN_SEGMENTS", raising=False)
            else:
                monkeypatch.setenv("TSAMD_TEST_FOLDIN_SEGMENTS", segs)
            eng.set_gamma(g0)
            out = eng.fold_in(max_iters=12, tol=1e-3)
            res[name] = (eng.get_gamma(), out)
        monkeypatch.delenv("TSAMD_TEST_FOLDIN_SEGMENTS", raising=False)
        assert res["device"][0].tobytes() == res["again"][0].tobytes()
        for key in ("iters", "change"):
            assert res["device"][1][key].tobytes() == res["again"][1][key].tobytes()
        err = max_rel(res["many"][0], res["one"][0])
        print(f"1 segment against 37: max rel = {err:.3e}; device default against 1: {max_rel(res['device'][0], res['one'][0]):.3e}")
        assert err <= 1e-12 and max_rel(res["device"][0], res["one"][0]) <= 1e-12
        assert max_rel(res["one"][0], reference_from(eng, g0, 12, 1e-3)) <= 1e-9
        # two shards, no exchange set up: each folds in its own rows
        parts = []
        for e in engines[1:]:
            e.fold_in(max_iters=12, tol=1e-3)
            parts.append(e.get_gamma())
        assert engines[1].shard_count + engines[2].shard_count == n
        err = max_rel(np.concatenate(parts), res["device"][0])
        print(f"two shards against one context: max rel = {err:.3e}")
        assert err <= 1e-12
    finally:
        for e in engines:
            e.close()


def reference_from(eng, g0, max_iters, tol):
    now = eng.get_gamma()
    eng.set_gamma(g0)
    ref = reference(eng, None, max_iters, tol)["gamma"]
    eng.set_gamma(now)
    return ref


def test_nothing_but_gamma_moves_and_every_launch_mode_accepts_the_state(ts):
    n, l, k = 1030, 40, 5
    tail = np.array([4, 4, 17, 0, 9, 33], dtype=np.uint32)
    with synth_engine(ts, n, l, k, 23) as eng:
        eng.run_schedule(np.array([3, 8, 1], dtype=np.uint32))  # ends in a training update: its gamma step is pending
        eng.synchronize()
        _, loc0 = eng.state_export()
        lam0, eb0, elb0, cn0, p0, h0 = eng.get_lambda(), eng.get_ebeta(), eng.get_elogbeta(), eng.get_counts(), eng.total_passes(), eng.pass_histogram()
        eng.fold_in(np.array([5, 1, 1, 39], dtype=np.uint32), max_iters=7, tol=1e-5)
        eng.fold_in(max_iters=3)
        _, loc1 = eng.state_export()
        arr = 128 + 2 * l * 2 * k * 8  # the header, lambda and the stored exp(Elogbeta)
        assert loc0[128:arr].tobytes() == loc1[128:arr].tobytes()
        for a, b in ((lam0, eng.get_lambda()), (eb0, eng.get_ebeta()), (elb0, eng.get_elogbeta()), (cn0, eng.get_counts()), (h0, eng.pass_histogram())):
            assert a.tobytes() == b.tobytes()
        assert eng.total_passes() == p0
        modes = [ts.LAUNCH_PER_PASS, ts.LAUNCH_PER_SNP, ts.LAUNCH_PER_SCHEDULE]
        for mode in modes:
            outs, mid = [], None  # (the schedule before the fold-in rounds differently from mode to mode: each mode has its own twin)
            for how in ("fold_in", "set_gamma"):
                with synth_engine(ts, n, l, k, 23) as e:
                    e.set_launch_mode(mode)
                    e.run_schedule(np.array([3, 8, 1], dtype=np.uint32))
                    e.synchronize()
                    if how == "fold_in":
                        e.fold_in(np.array([5, 1, 1, 39], dtype=np.uint32), max_iters=7, tol=1e-5)
                        e.fold_in(max_iters=3)
                        mid = e.get_gamma()
                    else:
                        e.clear_pending()
                        e.set_gamma(mid)
                    e.run_schedule(tail)
                    e.run_schedule(tail[:2], 1)
                    e.synchronize()
                    outs.append((e.get_gamma(), e.get_lambda(), e.get_counts(), e.state_export()[0]))
            for a, b in zip(*outs):
                assert a.tobytes() == b.tobytes(), mode


def test_set_lambda_range_equals_a_loop_of_set_lambda(ts):
    n, l, k = 530, 37, 6
    rng = np.random.default_rng(4)
    lam = rng.gamma(2.0, 30.0, size=(l, k, 2)) + 1e-3
    with ts.Engine(n, l, k) as a, ts.Engine(n, l, k) as b:
        a.set_lambda_range(lam[3:30], first_loc=3)
        a.set_lambda_range(lam[30:], first_loc=30)
        a.set_lambda_range(lam[:3])
        for loc in range(l):
            b.set_lambda(loc, lam[loc])
        assert a.get_lambda().tobytes() == lam.tobytes()
        for f in ("get_lambda", "get_ebeta", "get_elogbeta"):
            assert getattr(a, f)().tobytes() == getattr(b, f)().tobytes(), f
        before = a.state_export()[1].tobytes()
        bad = lam[:4].copy()
        bad[2, 1, 0] = 0.0
        for args in ((lam[:4], l - 3), (bad, 0), (-bad, 0), (np.where(bad == 0.0, np.inf, bad), 0), (np.where(bad == 0.0, np.nan, bad), 0)):
            with pytest.raises(ts.TsamdError) as e:
                a.set_lambda_range(args[0], first_loc=args[1])
            assert e.value.code == EINVAL
        assert a.state_export()[1].tobytes() == before


def test_bad_arguments_are_refused_and_the_context_stays_usable(ts):
    n, l, k = 200, 9, 2
    with synth_engine(ts, n, l, k, 2) as eng:
        g0 = eng.get_gamma()
        for kwargs, word in ((dict(locs=np.array([1, l], dtype=np.uint32)), "locs[1]"), (dict(locs=np.array([], dtype=np.uint32)), "n_locs"),
                             (dict(max_iters=0), "max_iters"), (dict(tol=-1e-9), "tol"), (dict(tol=float("inf")), "tol"), (dict(tol=float("nan")), "tol")):
            with pytest.raises(ts.TsamdError) as e:
                eng.fold_in(**kwargs)
            assert e.value.code == EINVAL and word in str(e.value), kwargs
        assert eng.get_gamma().tobytes() == g0.tobytes()
        out = eng.fold_in(max_iters=3)
        assert out["iters_run"] == 3 and max_rel(eng.get_gamma(), reference_from(eng, g0, 3, 0.0)) <= 1e-9
