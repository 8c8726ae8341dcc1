"""ts_schedule at K <= 8 after its "instruction diet" (csrc/tsamd_resident_kernels.h, kDietSel / kDietConst: the gamma
step's selects are arithmetic -- the step size times exactly 1.0 or 0.0, c_n plus 1 or 0 --, exp_digamma_split's two
constants sit in registers through the gamma step and the epilogues) against the CPU oracle, at the geometries whose
code the diet touches:

  * N = 32 768 on 8 workgroups: 16 individuals per thread, the straight-line instantiation <K, false, 0> the benchmark
    runs at N = 1M, with the one-level exchange -- K = 8 and K = 5;
  * N = 163 840 on 40 workgroups: the same instantiation with the two-level exchange -- K = 8;
  * N = 10 000 in the default geometry: the PARTIAL instantiation <K, true, 0>, most of a thread's items unused and
    skipped, the shard's last threads owning fewer items than the others -- K = 8 and K = 3.

Every case has missing genotypes in every column (a step size of exactly 0; c_n does not count them), held-out entries
at two locations, a convergence threshold under which SNPs stop after 1, 2 and 10 passes, and a schedule with
back-to-back revisits (the SNP's end is published at once) between SNPs whose capped last pass is deferred into the next
SNP's first exchange.

Tolerances: lambda and gamma rel 1e-9; c_n, the pass total and the pass histogram exact.

The threshold of a case is a fraction of N / K, the scale of a lambda entry after one SNP; the fraction (1e-3, 3e-3 for
N = 10 000 at K = 8) was picked by running the ORACLE alone over a grid of fractions and taking one at which its pass
counts include 1, 2 and 10 -- which the test asserts on the oracle's counts before it looks at the device."""
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
@pytest.mark.parametrize("n,k,workgroups,geometry,frac", [(32_768, 8, 8, (8, 16, 1), 1e-3),
                                                          (32_768, 5, 8, (8, 16, 1), 1e-3),
                                                          (163_840, 8, 40, (40, 16, 2), 1e-3),
                                                          (10_000, 8, None, (20, 2, 1), 3e-3),
                                                          (10_000, 3, None, (20, 2, 1), 1e-3)])
def test_schedule_kernel_matches_oracle(ts, monkeypatch, n, k, workgroups, geometry, frac):
    y, _, _ = psd_genotypes(n, L, k, 5100 + k, 0.03)
    assert all((y[loc] == 3).any() for loc in range(L))  # missing genotypes in every column
    payload = pack_bed(y)
    g = init_gamma(n, k, 5101 + k)
    rng = np.random.default_rng(5102 + k)
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
