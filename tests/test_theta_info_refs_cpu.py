"""tests/theta_info_refs.py on the CPU alone: a plain fp64 numpy restatement of the device terms and of the library's Cholesky
algorithm stays inside every derived bound, on the every-K fixtures and on the late-state fixtures of analysis_refs; the bounds
can tell a wrong kernel; and the calibration claim of the standard errors holds on numpy alone.

Measured here (worst |fp64 - ref| / bound): the information sums 4.9e-2 on the every-K fixtures (K = 2) and 3.7e-2 on the
late-state ones (the bound carries the project's factor 4); theta_se 1.2e-1 on the every-K fixtures (K = 2; 2e-2 at K = 4 and
falling with K, as the K^2 of the bound grows faster than the error) and 4.6e-2 on the late-state ones (n = 4200, K = 3), with
the constant 8 as stated -- it did not have to move.

Calibration (K = 3, theta = (0.5, 0.3, 0.2) for 256 replicates, L = 4096, 10 % missing, 200 fold-in updates from gamma = 1;
seeds 6 to 13, observed and expected information): sd over replicates / mean se between 0.923 and 1.075, coverage of the
nominal 95 % intervals between 0.932 and 0.958; the bands [0.80, 1.25] and [0.89, 0.995] are about four sampling standard
deviations wide at 256 replicates."""
import numpy as np
import pytest

import analysis_refs as ar
import theta_info_refs as tr

LD = np.longdouble


def check_case(c, shard=None):
    """(worst information ratio, worst theta_se ratio, identified rows) of the fp64 restatements on a planted case, full list
    and the case's unsorted list with a repeat"""
    every = ar.Entries(c.y, c.gamma, c.lam, c.held, None, shard)
    wi = ws = 0.0
    identified = 0
    for which in (c.locs, None):
        ref, bound = tr.info_ref(c.y, c.gamma, c.lam, c.ids, c.held, which, shard, entries=every)
        got = tr.info_numpy(c.y, c.gamma, c.lam, c.ids, c.held, which, shard)
        for key in ("obs", "exp"):
            assert got[key].shape == (len(c.ids), tr.packed(c.k)) and np.all(np.isfinite(got[key])) and np.all(got[key] >= 0)
        wi = max(wi, tr.compare_info(got, ref, bound, limit=0.5))
        for key in ("obs", "exp"):
            out = tr.se_numpy(got[key], c.k)
            rows = out["status"] == 0
            identified += int(rows.sum())
            if rows.any():
                sref, sbound = tr.se_ref(got[key][rows], c.k)
                ws = max(ws, tr.compare_se({k2: v[rows] for k2, v in out.items()}, sref, sbound, limit=0.5))
                cov = tr.unpack(out["cov"][rows], c.k, np.float64)
                assert np.all(np.abs(cov.sum(axis=2)) <= 1e-9 * np.abs(cov).max(axis=(1, 2))[:, None])
    return wi, ws, identified


@pytest.mark.parametrize("k", [1, 2, 4, 9, 17, 32, 33])
def test_fp64_numpy_lies_within_half_of_every_bound_every_k(k):
    c = ar.plant_every_k(k, n=600, l=70)
    wi, ws, identified = check_case(c)
    print(f"K={k}: information {wi:.3e}, theta_se {ws:.3e} of their bounds; {identified} rows identified")
    if k <= 17:
        assert identified == 4 * len(c.ids)  # interior theta, 38 listed loci or more against K - 1 directions: every row
    else:
        assert identified >= 2 * len(c.ids)  # (the full list of 70 loci identifies every row; the short list not all at K - 1 >= 31)


@pytest.mark.parametrize("shape", ar.LATE_SHAPES)
def test_fp64_numpy_lies_within_half_of_every_bound_late_state(shape):
    c, _ = ar.plant_late(*shape)
    e = ar.Entries(c.y, c.gamma, c.lam, c.held, None, c.shard)
    wi, ws, identified = check_case(c, c.shard)
    print(shape, "min q %.2e min 1-q %.2e: information %.3e, theta_se %.3e of their bounds; %d rows identified"
          % (float(e.q.min()), float(e.omq.min()), wi, ws, identified))


def test_the_bounds_can_tell_a_wrong_kernel():
    c = ar.plant_every_k(8, n=600, l=70)
    ref, bound = tr.info_ref(c.y, c.gamma, c.lam, c.ids, c.held, c.locs)
    good = tr.info_numpy(c.y, c.gamma, c.lam, c.ids, c.held, c.locs)
    assert tr.compare_info(good, ref, bound) <= 0.5

    def leaves(bad):
        try:
            tr.compare_info(bad, ref, bound)
        except AssertionError:
            return True
        return False

    assert leaves(dict(obs=good["exp"], exp=good["exp"]))                      # the expected information in the observed one's place
    assert leaves(dict(obs=good["obs"] * (1 + 1e-12), exp=good["exp"]))        # a relative 1e-12
    nolast = tr.info_numpy(c.y, c.gamma, c.lam, c.ids, c.held, c.locs[:-1])    # one location dropped
    assert leaves(nolast)
    noheld = tr.info_numpy(c.y, c.gamma, c.lam, c.ids, None, c.locs)           # the held-out entries counted
    assert leaves(noheld)
    swapped = {key: v[:, ::-1] for key, v in good.items()}                     # the packed order reversed
    assert leaves(swapped)
    # theta_se: a relative 1e-9 of a standard error leaves its bound at these condition numbers
    sref, sbound = tr.se_ref(good["obs"], c.k)
    out = tr.se_numpy(good["obs"], c.k)
    assert tr.compare_se(out, sref, sbound) <= 0.5
    with pytest.raises(AssertionError):
        tr.compare_se(dict(out, se=out["se"] * (1 + 1e-9)), sref, sbound)


@pytest.mark.parametrize("seed", tr.CAL_SEEDS)
def test_the_standard_errors_are_calibrated(seed):
    case = tr.calibration_case(seed)
    k = tr.CAL_K
    gamma = tr.numpy_fold_in(case["y"], case["lam"], k, iters=200)
    theta = gamma / gamma.sum(axis=1, keepdims=True)
    eb = case["lam"][:, :, 0] / case["lam"].sum(axis=2)
    assert np.max(np.abs(eb - case["beta"])) <= 1e-12
    info = tr.info_fp64(theta, eb, case["y"].T)
    for key in ("obs", "exp"):
        out = tr.se_numpy(info[key], k)
        assert np.all(out["status"] == 0)
        tr.assert_calibrated(theta, out["se"], f"seed {seed}, {key}: ")
