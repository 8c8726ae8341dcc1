"""The four analysis calls -- tsamd_train_loglik, tsamd_snp_scan, tsamd_kinship, tsamd_fold_in -- at EVERY K, against
extended-precision references from the planted inputs alone (tests/analysis_refs.py), within that module's derived bounds.

One test per K = 1 .. 32 (every specialised instantiation of ts_loglik<K>, ts_scan<K, TRAIT>, ts_kin_resid<K> and
ts_foldin_sweep<K>, among them 7, 9, the individuals-per-thread boundary 16 | 17 and the K >= 29 branch of the fold-in
sweep) and K = 33, 64, 128 (the run-time-K kernels).  n = 4611 / 2563 / 1539 / 1027 at K <= 4 / 8 / 16 / above: the largest
tile of the four families (256 threads x 16 / 8 / 4 / 2 individuals) and a second, ragged one.  Kinship runs on 130 listed
ids: three tiles of 64, the last one ragged.  l = 150, on two engines, because the real device cuts so short a list into
segments of one batch (loglik_segments, scan_segments: 19 segments of 8 locations):
  * the device's own geometry: three fold-in segments of 64 locations at every K (two batches of 32 each, four of 16 on
    ts_foldin_sweep_wide, whose read-modify-write of the partials across batches runs), 19 segments of the two sweeps;
  * the geometry of a two-unit device (TSAMD_TEST_MAX_WORKGROUPS = 2 with TSAMD_FLAG_TEST_HOOKS; every family has two tiles or
    more here, so the list stays whole): ONE segment of 150 locations, five LDS batches of 32, the last of 22, in ts_loglik<K>,
    ts_scan<K, TRAIT> and ts_foldin_sweep<K>; ten of 16, the last of 6, in ts_foldin_sweep_wide.

Genotypes are uploaded as PLINK bytes (no synth_genotypes), with held-out lists at locations 0, l / 2 and l - 1 that hold
individuals 0 and n - 1.  Before any call the reads are pinned to the planted values: download_bed byte for byte (held-out
entries as 01), get_theta within (K + 1) u, get_ebeta within 3 u.  No reference takes a value read from the engine.

Each call runs on the full list and on an unsorted list with a repeat; snp_scan with a trait and without; fold_in for 1
and 3 updates at tol = 0 (gamma to relative 1e-9, sum_k gamma = K alpha + 2 M to relative 1e-11).  Counts are exact, kin is
exactly symmetric.  Every test prints its worst |gpu - ref| / bound per family.

Measured once on one MI355X (2026-10-20), worst |gpu - ref| / bound over the 35 tests and both geometries: train_loglik
2.3e-2 (K = 2), snp_scan 1.2e-3 (K = 1), kinship 8.0e-2 (K = 1; its bound carries no factor 4), fold_in gamma 1.6e-5 of the
relative 1e-9 (K = 128), sum_k gamma 5.0e-4 of the relative 1e-11 (K = 1); get_theta at most 9.6 u (K = 128, allowed 129),
get_ebeta 1.9 u (allowed 3).  The 35 tests took 17.9 s together in a run of the whole suite (0.3 to 1.3 s each), most of it the long-double references.
"""
import numpy as np
import pytest

import analysis_refs as ar
from helpers import pack_bed
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

LD = np.longdouble


def pin_reads(eng, c, shard=None):
    """the engine's reads against the planted values; returns the worst theta and Ebeta errors in units of u"""
    b, n = (0, c.n) if shard is None else shard
    want = ar.bed_bytes(ar.stored_genotypes(c.y, c.held, shard))
    for loc in range(c.l):
        assert eng.download_bed(loc).tobytes() == want[loc].tobytes(), ("download_bed", loc)
    theta, eb = ar.theta_ref(c.gamma[b:b + n]), ar.ebeta_ref(c.lam)
    et = float(np.max(np.abs(eng.get_theta().astype(LD) - theta) / theta) / ar.U)
    ee = float(np.max(np.abs(eng.get_ebeta().astype(LD) - eb) / eb) / ar.U)
    assert et <= c.k + 1 and ee <= 3, (et, ee)
    return et, ee


def two_geometries(ts, monkeypatch, n, l, k, rank=0, world=1):
    """[the device's own geometry, that of a two-unit device]: two engines of the same shard (the hook is read at creation)"""
    monkeypatch.delenv("TSAMD_TEST_MAX_WORKGROUPS", raising=False)
    for var in ("TSAMD_TEST_LOGLIK_CHUNK", "TSAMD_TEST_SCAN_CHUNK", "TSAMD_TEST_KIN_CHUNK", "TSAMD_TEST_KIN_SEGMENTS", "TSAMD_TEST_FOLDIN_SEGMENTS"):
        monkeypatch.delenv(var, raising=False)
    wide = ts.Engine(n, l, k, rank=rank, world=world)
    monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "2")
    try:
        narrow = ts.Engine(n, l, k, rank=rank, world=world, flags=ts.FLAG_TEST_HOOKS)
    except Exception:
        wide.close()
        raise
    return [wide, narrow]


def run_families(engines, c, iters, shard=None):
    """one call per family, list and engine against analysis_refs (each reference computed once); returns {family: worst
    |gpu - ref| / bound} and the first engine's results of the full list (the fold-in leaves the planted gamma in place)"""
    b, n = (0, c.n) if shard is None else shard
    trait = c.trait[b:b + n]
    g0 = np.ascontiguousarray(c.gamma[b:b + n])
    args = (c.y, c.gamma, c.lam)
    every = ar.Entries(*args, c.held, None, shard)
    worst = dict(loglik=0.0, scan=0.0, kin=0.0, foldin=0.0, foldin_sum=0.0)
    full = {}
    for which in (c.locs, None):
        ll_ref, ll_bound = ar.loglik_ref(*args, c.held, which, shard, entries=every)
        sc_ref, sc_bound = ar.scan_ref(*args, c.held, which, shard, trait, entries=every)
        fit_ref = {key: v for key, v in sc_ref.items() if key.startswith("fit")}
        kin_ref, kin_bound = ar.kin_ref(*args, c.ids, c.held, which, shard, entries=every)
        fi_ref = ar.foldin_ref(*args, c.alpha, iters, c.held, which, shard)
        for eng in engines:
            got = eng.train_loglik(which)
            worst["loglik"] = max(worst["loglik"], ar.compare_loglik(got, ll_ref, ll_bound))
            only = eng.train_loglik(which, per_loc=False, per_indiv=False)
            assert only["sum"] == got["sum"] and only["count"] == got["count"]
            scan = eng.snp_scan(which, trait)
            worst["scan"] = max(worst["scan"], ar.compare_scan(scan, sc_ref, sc_bound), ar.compare_scan(eng.snp_scan(which), fit_ref, sc_bound))
            kin = eng.kinship(c.ids, which, parts=True)
            for a in kin:
                assert a.shape == (ar.KIN_M, ar.KIN_M) and a.tobytes() == np.ascontiguousarray(a.T).tobytes()  # exactly symmetric
            worst["kin"] = max(worst["kin"], ar.compare_kin(kin, kin_ref, kin_bound))
            gammas = {}
            for i in iters:
                eng.set_gamma(g0)
                out = eng.fold_in(which, max_iters=i, tol=0.0)
                gammas[i] = eng.get_gamma()
                assert out["iters_run"] == i and out["n_converged"] == 0
                worst["foldin"] = max(worst["foldin"], ar.compare_foldin(gammas[i], out, fi_ref[i]))
                err = ar.foldin_sum_error(gammas[i], c.k, c.alpha, ll_ref["indiv_counts"])
                worst["foldin_sum"] = max(worst["foldin_sum"], err / ar.FOLDIN_SUM_TOL)
                assert err <= ar.FOLDIN_SUM_TOL, ("sum_k gamma", err)
            eng.set_gamma(g0)
            if which is None and eng is engines[0]:
                full = dict(loglik=got, scan=scan, kin=kin, foldin=gammas)
    return worst, full


@pytest.mark.parametrize("k", ar.EVERY_K)
def test_every_k(ts, k, monkeypatch):
    c = ar.plant_every_k(k)
    assert c.n > 256 * (16 if k <= 4 else 8 if k <= 8 else 4 if k <= 16 else 2) and c.l == 150
    engines = two_geometries(ts, monkeypatch, c.n, c.l, k)
    try:
        for eng in engines:
            assert eng.cfg.alpha == c.alpha
            eng.upload_bed(pack_bed(c.y))
            eng.set_gamma(c.gamma)
            eng.set_lambda_range(c.lam)
            for loc, ids in c.held.items():
                eng.set_heldout(loc, ids)
            et, ee = pin_reads(eng, c)
        worst, _ = run_families(engines, c, (1, 3))
    finally:
        for eng in engines:
            eng.close()
    print(f"K={k} n={c.n}: theta {et:.2f} u, Ebeta {ee:.2f} u; worst |gpu - ref| / bound: " + ", ".join(f"{f} {v:.3e}" for f, v in worst.items()))
