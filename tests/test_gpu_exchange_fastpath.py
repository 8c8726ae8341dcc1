"""ts_schedule's in-launch exchange at K <= 8 on one GPU, where a sweep whose rows and granules all exist takes the words
as loaded and compares tags only (csrc/tsamd_resident_kernels.h: res_sweep's FULL path, kXchgFull), against the CPU
oracle.  That path needs 32 members in a leader's group (level 1) and 8 groups (level 2) with 32 valid granules
(K = 8), i.e. many workgroups -- tests/test_gpu_sched_diet.py stops at 40 -- so the cases are small shards on 248 ... 256
workgroups:

  * 256 workgroups, K = 8: every leader and both levels take the select-free path;
  * 255 workgroups, K = 8: the group of blockIdx % 8 == 7 has 31 members, its leader takes the general path, the
    other seven leaders and level 2 the select-free one;
  * 248 workgroups, K = 8: every group has 31 members -- level 1 general, level 2 select-free;
  * 256 workgroups, K = 5: 20 valid granules -- the general path at both levels, although all rows exist.

The workgroup count follows from N (tsamd_plan.h, resident_geometry: a workgroup takes whole rounds of 256 individuals
of the shard padded to 512): 256 workgroups of one individual per thread at 65 024 < N <= 65 536; 255 and 248 workgroups
are only reached with two individuals per thread, at 130 048 < N <= 130 560 and 126 464 < N <= 126 976.  The cases set
TSAMD_SCHED_WORKGROUPS to their count all the same (a cap; the geometry is asserted from schedule_geometry()).  N is
no multiple of 256, so the shard's last threads own fewer items than the others.

Structure, schedule and tolerances are those of tests/test_gpu_sched_diet.py: missing genotypes in every column,
held-out entries at two locations, back-to-back revisits between SNPs whose capped last pass is deferred into the next
SNP's first exchange (an exchange of width 2: workgroup 0 sweeps a second region on the same path); lambda and gamma rel
1e-9; c_n, the pass total and the pass histogram exact; no recovery.

The threshold of a case is a fraction of N / K picked by running the ORACLE alone over the grid 3e-4, 5e-4, 7e-4, 1e-3,
3e-3, 1e-2 and taking one at which its pass counts include 1, 2 and 10 -- asserted on the oracle's counts before the
device is looked at."""
import numpy as np
import pytest

import oracle_py as op
from helpers import init_gamma, pack_bed, psd_genotypes, rel_err, usable_cores

pytestmark = pytest.mark.gpu

L = 8
# back-to-back revisits (3 3, 5 5 5, 1 1), a revisit one SNP later (6 2 6: not deferred either), SNPs followed by two others
SCHED = np.array([3, 3, 0, 7, 5, 5, 5, 4, 6, 2, 6, 1, 1, 0, 3, 7, 2], dtype=np.uint32)
HELD_LOCS = (3, 5)


@pytest.fixture(scope="module")
def ts():
    import terastructure_amd as t

    t.load()
    return t


# n, k, TSAMD_SCHED_WORKGROUPS (None: the default geometry), the geometry the case is about (workgroups, individuals per
# thread, exchange levels), threshold as a fraction of n / k
@pytest.mark.parametrize("n,k,workgroups,geometry,frac", [(65_500, 8, None, (256, 1, 2), 1e-3),
                                                          (130_500, 8, 255, (255, 2, 2), 3e-4),
                                                          (126_900, 8, 248, (248, 2, 2), 1e-3),
                                                          (65_500, 5, None, (256, 1, 2), 5e-4)])
def test_schedule_kernel_matches_oracle(ts, monkeypatch, n, k, workgroups, geometry, frac):
    y, _, _ = psd_genotypes(n, L, k, 6100 + k, 0.03)
    assert all((y[loc] == 3).any() for loc in range(L))  # missing genotypes in every column
    payload = pack_bed(y)
    g = init_gamma(n, k, 6101 + k)
    rng = np.random.default_rng(6102 + k)
    held = {loc: np.sort(rng.choice(np.nonzero(y[loc] != 3)[0], size=n // 50, replace=False)).astype(np.uint32) for loc in HELD_LOCS}
    thresh = frac * n / k

    orc = op.Oracle(n, L, k, nthreads=usable_cores(), meanchangethresh=thresh)
    orc.load_bed_payload(payload)
    orc.set_gamma(g)
    for loc, ids in held.items():
        orc.set_heldout(loc, ids)
    its = [orc.snp_update(int(loc)) for loc in SCHED]
    lam_o, gam_o, cnt_o = orc.lambda_(), orc.gamma(), orc.c_indiv()
    orc.close()
    assert {1, 2, 10} <= set(its), its
    # a capped SNP followed by two SNPs elsewhere (its last pass is deferred) and a SNP whose successor revisits it
    capped_then_elsewhere = [i for i in range(len(SCHED) - 2) if its[i] == 10 and SCHED[i] not in (SCHED[i + 1], SCHED[i + 2])]
    assert capped_then_elsewhere and any(SCHED[i] == SCHED[i + 1] for i in range(len(SCHED) - 1)), its

    if workgroups is not None:
        monkeypatch.setenv("TSAMD_SCHED_WORKGROUPS", str(workgroups))
    with ts.Engine(n, L, k, conv_thresh=thresh) as eng:
        assert eng.launch_info()["kernels_per_snp"] == 0  # ts_schedule
        geo = eng.schedule_geometry()
        assert (geo["workgroups"], geo["indivs_per_thread"], geo["exchange_levels"]) == geometry, geo
        assert geo["on_chip_per_thread"] == geo["indivs_per_thread"]  # (not ts_hybrid)
        eng.upload_bed(payload)
        eng.set_gamma(g)
        for loc, ids in held.items():
            eng.set_heldout(loc, ids)
        eng.run_schedule(SCHED)
        eng.synchronize()
        assert eng.recoveries() == 0  # (the one-launch kernel ran, not its launch-per-pass replay)
        assert eng.total_passes() == sum(its)
        assert np.array_equal(eng.pass_histogram(), np.bincount(its, minlength=128).astype(np.uint64))
        lam_d, gam_d, cnt_d = eng.get_lambda(), eng.get_gamma(), eng.get_counts()
    assert np.array_equal(cnt_d, cnt_o)
    e_lam, e_gam = rel_err(lam_d, lam_o), rel_err(gam_d, gam_o)
    print(f"n={n} k={k}: passes {its}, lambda rel err {e_lam:.2e}, gamma rel err {e_gam:.2e}")
    assert e_lam < 1e-9 and e_gam < 1e-9, (e_lam, e_gam)
