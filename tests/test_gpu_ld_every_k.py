"""tsamd_ld at every K = 1 .. 32 -- each its own instantiation of ts_ld_resid -- once, at n = 600, l = 70, W = 9: three workgroups
of individuals with a ragged last one, two location tiles with a ragged last one, one overlap tile.  The reference, the
fixtures and the bounds are those of tests/test_gpu_ld.py: cnt exact, |num - ref| <= 1e-11 sum |z z|."""
import pytest

from test_gpu_kinship import synth_engine
from test_gpu_ld import assert_matches, reference
from test_gpu_parity import ts  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(1, 33))
def test_every_specialised_k(ts, k):
    n, l, w = 600, 70, 9
    with synth_engine(ts, n, l, k, 300 + k) as eng:
        assert_matches(eng.ld(None, w), reference(eng, None, w), f"K={k}: ")
