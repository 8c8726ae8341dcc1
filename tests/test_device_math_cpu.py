"""CPU checks of the device-math test material: the committed references (tests/golden/device_math_refs.npz) still
follow from their generator (tests/golden/make_math_refs.py, mpmath at 50 digits), and the GPU probe
(tests/device_math_probe.hip) still compiles with the library's flags -- so a broken probe shows before a GPU run."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _generator():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_math_refs", os.path.join(GOLDEN, "make_math_refs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture_and_generator():
    gen = _generator()
    with np.load(gen.OUT) as z:
        refs = {k: z[k] for k in z.files}
    return refs, gen


def test_device_math_refs_inputs_are_the_generators(fixture_and_generator):
    refs, gen = fixture_and_generator
    inp = gen.inputs()
    for k, v in inp.items():
        assert np.array_equal(refs[k], v), k


def test_device_math_refs_rederived(fixture_and_generator):
    """a random sample of every table, recomputed with mpmath: hi bit for bit, lo to a few units of its last place"""
    refs, gen = fixture_and_generator
    rng = np.random.default_rng()

    def sample(n):
        return rng.choice(n, size=min(n, 25), replace=False)

    def same(got, want, what):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got[..., 0].tobytes() == want[..., 0].tobytes(), (what, got, want)
        assert np.allclose(got[..., 1:], want[..., 1:], rtol=1e-12, atol=0.0, equal_nan=True), (what, got, want)

    for i in sample(len(refs["digamma_x"])):
        same(gen.ref_digamma(refs["digamma_x"][i]), refs["digamma_ref"][i], ("digamma", i))
    for i in sample(len(refs["split_x"])):
        e, a = gen.ref_exp_digamma_split(refs["split_x"][i])
        same(e, refs["split_expsi"][i], ("split exp", i))
        same(a, refs["split_a"][i], ("split a", i))
    for i in sample(len(refs["exp_d"])):
        same(gen.ref_exp(refs["exp_d"][i]), refs["exp_ref"][i], ("exp", i))
    for i in sample(len(refs["rcp_x"])):
        same(gen.ref_rcp(refs["rcp_x"][i]), refs["rcp_ref"][i], ("rcp", i))
    for i in sample(len(refs["rsqrt_x"])):
        same(gen.ref_rsqrt(refs["rsqrt_x"][i]), refs["rsqrt_ref"][i], ("rsqrt", i))
    for i in sample(len(refs["ebeta_l"])):
        same(gen.ref_ebeta(*refs["ebeta_l"][i]), refs["ebeta_ref"][i], ("ebeta", i))
    for k in gen.GAMMA_KS:
        for i in sample(len(refs[f"gamma{k}_g"]))[:4]:
            d, r = gen.ref_gamma_row(refs[f"gamma{k}_g"][i])
            assert d.tobytes() == refs[f"gamma{k}_d"][i].tobytes() and r.tobytes() == refs[f"gamma{k}_ratio"][i].tobytes(), (k, i)


def test_device_math_refs_cover_the_late_regime(fixture_and_generator):
    refs, _ = fixture_and_generator
    assert refs["digamma_x"].min() <= 1e-8 and refs["digamma_x"].max() >= 1e12
    d = refs["exp_d"]
    assert ((d > -745.2) & (d < -708.4)).sum() >= 1000 and d.min() <= -1.4e9 and 0.0 in d
    e = np.frexp(refs["rcp_x"])[1]
    assert e.min() <= -990 and e.max() >= 990
    for k in (3, 8, 20, 32):
        g = refs[f"gamma{k}_g"]
        assert g.min() <= 1e-8 and g.max() >= 1e6
        assert (refs[f"gamma{k}_d"] < -20.0).any()


def test_device_math_refs_size():
    assert os.path.getsize(os.path.join(GOLDEN, "device_math_refs.npz")) < 1 << 20


@pytest.mark.skipif(not (os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")),
                    reason="hipcc not found")
def test_device_math_probe_compiles(tmp_path):
    import math_probe

    out = math_probe.compile_probe(str(tmp_path))
    assert os.path.getsize(out) > 0
