"""The oracle from a planted late-training state (tests/late_state.py): orc_set_counts sets c_n, and the next gamma step
uses rho = (nodetau0 + c_n)^-nodekappa from the planted counts (update_rho_indiv, src/snpsamplinge.cc:688-693)."""
import numpy as np
import pytest

import late_state
import oracle_py as op


@pytest.mark.parametrize("kappa", [0.5, 0.7])
def test_late_state_oracle_gamma_step_uses_planted_counts(kappa):
    n, l, k = 600, 8, 5
    s = late_state.plant(n, l, k, 41, l_eff=5e5)
    orc = op.Oracle(n, l, k, gamma_scale=s.l_eff, nodekappa=kappa)
    late_state.load_oracle(orc, s)
    assert np.array_equal(orc.c_indiv(), s.counts)
    loc = 2
    lt = orc.pass_partial(loc, 0, n)      # phi of every individual from the planted gamma and lambda
    assert np.all(np.isfinite(lt))
    g0, elt, elb = orc.gamma(), orc.elogtheta(), orc.elogbeta()[loc]
    orc.gamma_step(loc)

    def phi(t):
        e = elt + elb[None, :, t]
        e = np.exp(e - e.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    # the same step in numpy, rho from the planted counts
    y = s.y[loc].astype(np.float64)
    ok = s.y[loc] != 3
    cfg = orc.cfg
    rho = (cfg.nodetau0 + s.counts.astype(np.float64)) ** -kappa
    target = cfg.alpha + s.l_eff * (y[:, None] * phi(0) + (2.0 - y[:, None]) * phi(1))
    want = np.where(ok[:, None], g0 + rho[:, None] * (target - g0), g0)
    got = orc.gamma()
    assert np.max(np.abs(got - want) / (np.abs(want) + 1e-300)) < 1e-9
    assert np.array_equal(orc.c_indiv(), s.counts + ok.astype(np.uint32))
    # a step with rho from fresh counts would differ: the planted counts were used
    rho0 = cfg.nodetau0 ** -kappa
    fresh = np.where(ok[:, None], g0 + rho0 * (target - g0), g0)
    assert np.max(np.abs(got - fresh) / np.abs(fresh)) > 1e-3
    orc.close()


def test_late_state_plant_is_deterministic_and_late():
    a = late_state.plant(2000, 10, 8, 7)
    b = late_state.plant(2000, 10, 8, 7)
    for x, z in ((a.gamma, b.gamma), (a.counts, b.counts), (a.lam, b.lam), (a.y, b.y)):
        assert np.array_equal(x, z)
    rows = a.gamma.sum(axis=1)
    assert np.median(rows) > 5e5 and a.gamma.min() == 1e-8
    assert a.counts.max() >= 999_000 and (a.counts == 0).sum() >= 8 and np.median(a.counts) > 5000
    assert (a.lam == 1.0).any() and a.lam.max() > 0.1 * a.n
    assert len(a.held) == 3
