"""tsamd_theta_info at EVERY K and from a late-training state, against the long-double references of tests/theta_info_refs.py from
the planted inputs alone, within that module's derived bounds; tsamd_theta_se on the device's rows against pinv(P H P) in long
double.

One test per K = 1 .. 32 (every specialised instantiation of ts_info_coef<K>) and K = 33, 64, 128 (the run-time-K form), at
n = 600, l = 70 and m = 130 listed ids (three tiles of 64 individuals, the last one ragged; 1 to 129 column tiles), on the full
list and on an unsorted list with a repeat, with held-out lists at locations 0, l / 2 and l - 1.  The late-state shapes are
analysis_refs.LATE_SHAPES: Ebeta within 1e-6 of 0 and 1, gamma from the 1e-8 floor -- the hard case for 1 / q^2 -- among them
rank 1 of 3, whose shard begins at individual 344 (no multiple of 16), where the whole shard goes the contiguous way too.

Measured once on one MI355X (2026-10-21), worst |gpu - ref| / bound: 4.9e-2 over the 35 every-K tests (K = 2; about 1e-2 from
K = 5 on) and 7.0e-2 over the five late-state shapes (n = 4200, K = 3); theta_se on the device's rows 2.8e-1 of its bound at
K = 2 (its K^2 is smallest there), 2.7e-2 at K = 3 and falling with K, 3.1e-2 at the late state.  The 40 tests took 7 s
together (K = 128: 1.5 s, most of it the long-double reference of 8 256 columns)."""
import numpy as np
import pytest

import analysis_refs as ar
import late_state
import theta_info_refs as tr
from helpers import pack_bed
from test_gpu_analysis_every_k import pin_reads
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu


def run_info(ts, eng, c, shard=None):
    """worst |gpu - ref| / bound of theta_info over both lists, worst theta_se ratio over the identified rows"""
    every = ar.Entries(c.y, c.gamma, c.lam, c.held, None, shard)
    wi = ws = 0.0
    for which in (c.locs, None):
        ref, bound = tr.info_ref(c.y, c.gamma, c.lam, c.ids, c.held, which, shard, entries=every)
        got = eng.theta_info(c.ids, which)
        assert all(np.all(np.isfinite(got[key])) and np.all(got[key] >= 0) for key in got)
        wi = max(wi, tr.compare_info(got, ref, bound))
        out = ts.theta_se(got["obs"], c.k)
        rows = out["status"] == 0
        if rows.any() and c.k <= 33:  # (the long-double elimination of 130 matrices is the test's cost)
            sref, sbound = tr.se_ref(got["obs"][rows], c.k)
            ws = max(ws, tr.compare_se({key: v[rows] for key, v in out.items()}, sref, sbound))
        assert np.isnan(out["se"][~rows]).all()
    return wi, ws


@pytest.mark.parametrize("k", ar.EVERY_K)
def test_every_k(ts, k):
    c = ar.plant_every_k(k, n=600, l=70)
    with ts.Engine(c.n, c.l, k) as eng:
        eng.upload_bed(pack_bed(c.y))
        eng.set_gamma(c.gamma)
        eng.set_lambda_range(c.lam)
        for loc, ids in c.held.items():
            eng.set_heldout(loc, ids)
        pin_reads(eng, c)
        wi, ws = run_info(ts, eng, c)
    print(f"K={k}: worst |gpu - ref| / bound: theta_info {wi:.3e}, theta_se {ws:.3e}")


@pytest.mark.parametrize("n,l,k,world,rank", ar.LATE_SHAPES)
def test_late_state(ts, n, l, k, world, rank):
    c, s = ar.plant_late(n, l, k, world, rank)
    b, cnt = c.shard
    with ts.Engine(n, l, k, rank=rank, world=world) as eng:
        assert (eng.shard_begin, eng.shard_count) == c.shard
        late_state.load_engine(eng, s)
        pin_reads(eng, c, c.shard)
        before = eng.state_export()
        wi, ws = run_info(ts, eng, c, c.shard)
        # the whole shard (indivs == NULL, the contiguous way to the columns) against the same ids listed
        whole = eng.theta_info()
        ref, bound = tr.info_ref(c.y, c.gamma, c.lam, np.arange(b, b + cnt), c.held, None, c.shard)
        wi = max(wi, tr.compare_info(whole, ref, bound))
        after = eng.state_export()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    print(f"late n={n} l={l} K={k} rank {rank} of {world}: worst |gpu - ref| / bound: theta_info {wi:.3e}, theta_se {ws:.3e}")
