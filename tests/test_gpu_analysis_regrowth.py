"""The analysis calls' scratch buffers grow on demand and never shrink (DevBuf, csrc/tsamd.hip): a call on an engine whose
buffers an earlier call left smaller, or larger, than it needs must give what the same call gives on a fresh engine --
byte for byte, since the summation order is fixed and the geometry is equal.

n = 1027, l = 40, at k = 3 and at k = 33 (the run-time-K theta scratch).  TSAMD_FLAG_TEST_HOOKS with
TSAMD_TEST_MAX_WORKGROUPS = 2 and chunks of 7 locations for train_loglik, snp_scan and kinship: the full list is six chunks
and the geometry does not depend on the device.  On ONE engine, each of the six calls on a 3-location list, then on the
full list, then on the 3-location list again; kinship and theta_info with 5 listed individuals, then 70 (mpad 64 -> 128),
then 5; snp_scan without a trait, with one, without; fold_in for 2 updates at tol = 0 from the planted gamma; ld at window 2,
then 130 (the overlap goes from 1 tile to 3: lpad, the accumulators and the band's rows grow and are then under-used), then
2.  Each result against a fresh engine created under the same hooks (one per distinct step; the families share no buffer
but the theta scratch, whose size is fixed)."""
import numpy as np
import pytest

import analysis_refs as ar
from helpers import pack_bed
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu

N, L = 1027, 40


def load(eng, c):
    eng.upload_bed(pack_bed(c.y))
    eng.set_gamma(c.gamma)
    eng.set_lambda_range(c.lam)
    for loc, ids in c.held.items():
        eng.set_heldout(loc, ids)


def six_calls(eng, c, locs, ids, trait, window):
    out = dict(loglik=eng.train_loglik(locs), scan=eng.snp_scan(locs, trait), kin=eng.kinship(ids, locs, parts=True),
               ld=eng.ld(locs, window), info=eng.theta_info(ids, locs))
    eng.set_gamma(c.gamma)
    fi = eng.fold_in(locs, max_iters=2, tol=0.0)
    assert fi["iters_run"] == 2 and fi["n_converged"] == 0
    out["foldin"] = dict(fi, gamma=eng.get_gamma())
    eng.set_gamma(c.gamma)
    return out


def frozen(x):
    """a result with every array as its bytes"""
    if isinstance(x, dict):
        return {key: frozen(v) for key, v in x.items()}
    if isinstance(x, tuple):
        return [frozen(v) for v in x]
    return (x.dtype.str, x.shape, x.tobytes()) if isinstance(x, np.ndarray) else x


@pytest.mark.parametrize("k", [3, 33])
def test_calls_after_smaller_and_larger_calls_match_a_fresh_engine(ts, k, monkeypatch):
    c = ar.plant_every_k(k, n=N, l=L)
    monkeypatch.setenv("TSAMD_TEST_MAX_WORKGROUPS", "2")
    for var in ("TSAMD_TEST_LOGLIK_CHUNK", "TSAMD_TEST_SCAN_CHUNK", "TSAMD_TEST_KIN_CHUNK"):
        monkeypatch.setenv(var, "7")
    for var in ("TSAMD_TEST_KIN_SEGMENTS", "TSAMD_TEST_FOLDIN_SEGMENTS", "TSAMD_TEST_LD_CHUNK", "TSAMD_TEST_LD_BLOCK", "TSAMD_TEST_INFO_CHUNK",
                "TSAMD_TEST_INFO_BLOCK"):
        monkeypatch.delenv(var, raising=False)
    short, full = c.locs[:3], np.arange(L, dtype=np.uint32)
    assert len(set(short.tolist())) == 3
    steps = [(short, c.ids[:5], None, 2), (full, c.ids[:70], c.trait, 130), (short, c.ids[:5], None, 2)]

    def fresh(step):
        with ts.Engine(N, L, k, flags=ts.FLAG_TEST_HOOKS) as eng:
            load(eng, c)
            return frozen(six_calls(eng, c, *step))

    want = [fresh(steps[0]), fresh(steps[1])]
    want.append(want[0])
    with ts.Engine(N, L, k, flags=ts.FLAG_TEST_HOOKS) as eng:
        load(eng, c)
        for i, step in enumerate(steps):
            got = frozen(six_calls(eng, c, *step))
            assert set(got) == {"loglik", "scan", "kin", "foldin", "ld", "info"}
            for family in got:
                assert got[family] == want[i][family], (k, "step", i, family)
    # the steps differ: the second one's results are not the first one's cut short
    assert want[1]["loglik"]["loc_sums"][1] == (L,) and want[0]["loglik"]["loc_sums"][1] == (3,)
    assert "trait_sums" in want[1]["scan"] and "trait_sums" not in want[0]["scan"] and want[1]["kin"][0][1] == (70, 70)
    assert want[1]["ld"]["num"][1] == (L, 131) and want[0]["ld"]["num"][1] == (3, 3)
    p = k * (k + 1) // 2
    assert want[1]["info"]["obs"][1] == (70, p) and want[0]["info"]["obs"][1] == (5, p)
