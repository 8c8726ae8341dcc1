"""The engine's hand-written device math against exact values (tests/golden/device_math_refs.npz, mpmath at 50 digits).

Every primitive runs on the GPU through tests/device_math_probe.hip, compiled with the library's own flags, on inputs
that reach the late-training regime: gammas up to 2e6 and down to the 1e-8 floor, softmax exponents 20 and more apart,
exp results deep in the subnormal band.  Errors are measured against the exact value (the fixture's double-double), in
ulps of the exact result unless said otherwise.

The accuracy claims in csrc/tsamd_device.h cite fitting and micro-benchmark tools that are not in this repository
(tools/fit/psi_tail_minimax.py, tools/fit/exp_minimax.py, tools/ubench/rcp_accuracy.hip, tools/ubench/op_cost.hip);
tools/rcp_acc.hip still describes fast_rcp / fast_rsqrt as two Newton steps, while each now applies ONE third-order step
to the hardware estimate.  These tests are the measured record instead.  Where a primitive missed a bound the comments
imply, the test's docstring says why (cancellation, or an exponent's absolute error turning into a relative one) and
the bound follows from that.  Worst cases measured on an MI355X (gfx950) with these inputs:

    digamma              8.7 ulp of |psi| (tiny x); 1.44e-15 absolute next to the root   (bound 10 ulp + 4 ulp of log(x+10))
    exp_digamma_split a  9.5 ulp of |a|, 0.66 of its bound; z exp(a) 1.3e3 ulp where |a| ~ 600, 0.42 of its bound
    exp_nonpos           0.77 ulp (normal results), 0.5 spacing (subnormal band), exact 0 below -746, exp(0) = 1
    fast_rcp             0.50 ulp over 2^-1000 ... 2^1000
    fast_rsqrt           0.90 ulp
    Ebeta                9.0 ulp (bound 12)
    gamma_to_w<K>        rel / max(1, |D|) <= 1.34e-15 at K = 3, 8, 20, 32 (bound 1e-14); lean == regular bit for bit
    WaveFold<1..64>, code_weights / code_nibble: exact
"""
import os

import numpy as np
import pytest

import math_probe as mp

pytestmark = pytest.mark.gpu

REFS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_math_refs.npz")
TINY = 2.0 ** -1022


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return mp.Probe(mp.compile_probe(str(tmp_path_factory.mktemp("math_probe"))))


@pytest.fixture(scope="module")
def refs():
    with np.load(REFS) as z:
        return {k: z[k] for k in z.files}


def ulp_err(dev, ref):
    """|dev - exact| in ulps of the exact value; ref[..., 0] / ref[..., 1] are its hi / lo parts"""
    hi, lo = ref[..., 0], ref[..., 1]
    return np.abs((dev - hi) - lo) / np.spacing(np.abs(hi))


def report(name, v):
    print(f"[device math] {name}: {v:.3g}")


def test_device_math_digamma(probe, refs):
    """psi(x) = [log(z) - 1/(2z) - series] - P'(x)/P(x), z = x + 10: the rational part runs through some twenty roundings
    (two Horner-like chains and a division), so psi carries up to ~9 ulps of itself; and where psi is small against log(z)
    (x of order 1, the root at 1.4616 above all) the two halves cancel, so the error there is a few ulps of log(z).
    Bound: 10 ulp(|psi|) + 4 ulp(log(x + 10))."""
    x, ref = refs["digamma_x"], refs["digamma_ref"]
    dev = probe.run(mp.DIGAMMA, x)
    err = np.abs((dev - ref[:, 0]) - ref[:, 1])
    bound = 10.0 * np.spacing(np.abs(ref[:, 0])) + 4.0 * np.spacing(np.log(x + 10.0))
    near_root = np.abs(x - 1.4616321449683622) < 1e-3
    report("digamma max err / bound", (err / bound).max())
    report("digamma max ulp of |psi| where |psi| >= 1", (err / np.spacing(np.abs(ref[:, 0])))[np.abs(ref[:, 0]) >= 1.0].max())
    report("digamma max abs near the root", err[near_root].max())
    bad = np.where(err > bound)[0]
    assert bad.size == 0, [(x[i], dev[i], ref[i, 0], err[i] / bound[i]) for i in bad[:8]]
    # both sides of the switch to the plain asymptotic series at 1e8 (no recurrence) stay within 4 ulp of psi
    big = (x >= np.nextafter(1e8, 0.0)) & (x <= np.nextafter(1e8, np.inf))
    assert big.sum() == 3 and (err[big] / np.spacing(np.abs(ref[big, 0]))).max() <= 4.0


def test_device_math_exp_digamma_split(probe, refs):
    """a = u - r: r = sum_{i<10} 1/(x+i) is formed as (2x+9) Q'(q) / Q(q) through some ten roundings, so a carries up to
    8 ulps of r <= |a| + 0.06 (|u| <= 0.051), plus the 1e-17 of the tail polynomial.  z * exp(a) then carries that absolute
    error of a as a relative error (|a| reaches ~600 where exp(psi(x)) is still normal, x ~ 1e-3: a thousand ulps there)."""
    x, expsi, aref = refs["split_x"], refs["split_expsi"], refs["split_a"]
    out = probe.run(mp.EXP_DIGAMMA_SPLIT, x, 2.0).reshape(-1, 2)
    z, a = out[:, 0], out[:, 1]
    assert np.array_equal(z, x + 10.0)
    aerr = np.abs((a - aref[:, 0]) - aref[:, 1])
    bound = 8.0 * np.spacing(np.abs(aref[:, 0]) + 0.06) + 2e-17
    report("exp_digamma_split a: max err / bound", (aerr / bound).max())
    report("exp_digamma_split a: max ulp of |a|", (aerr / np.spacing(np.abs(aref[:, 0]))).max())
    bad = np.where(aerr > bound)[0]
    assert bad.size == 0, [(x[i], a[i], aref[i, 0], aerr[i]) for i in bad[:8]]
    # z * exp(a) = exp(psi(x)) where that is a normal number: relative error <= the bound on a plus the roundings of z,
    # of the product and of numpy's exp (4 ulp)
    ok = expsi[:, 0] > TINY
    prod = z[ok] * np.exp(a[ok])
    rel = np.abs((prod - expsi[ok, 0]) - expsi[ok, 1]) / expsi[ok, 0]
    rbound = bound[ok] + 4.0 * 2.0 ** -52
    report("exp_digamma_split z*exp(a) max ulp", ulp_err(prod, expsi[ok]).max())
    report("exp_digamma_split z*exp(a) max rel / bound", (rel / rbound).max())
    worst = np.argmax(rel / rbound)
    assert (rel / rbound).max() <= 1.0, (x[ok][worst], prod[worst], expsi[ok][worst, 0], rel[worst])
    small = np.abs(aref[ok, 0]) < 1.0     # x >= ~3: |a| < 1, and the product is within 4 ulp
    assert ulp_err(prod[small], expsi[ok][small]).max() <= 4.0


def test_device_math_exp_nonpos(probe, refs):
    d, ref = refs["exp_d"], refs["exp_ref"]
    dev = probe.run(mp.EXP_NONPOS, d)
    normal = ref[:, 0] >= TINY
    e = ulp_err(dev[normal], ref[normal])
    report("exp_nonpos max ulp (normal results)", e.max())
    assert e.max() <= 2.0, (d[normal][np.argmax(e)], e.max())
    # the subnormal band: within one spacing of the subnormal grid (dev * 2^1074 is exact)
    sub = ~normal & (d >= -746.0)
    spac = np.abs(np.ldexp(dev[sub], 1074) - ref[sub, 2])
    report("exp_nonpos max spacings (subnormal results)", spac.max())
    assert spac.max() <= 1.0, (d[sub][np.argmax(spac)], spac.max())
    assert int(sub.sum()) > 1000
    # exp(0) is exactly 1; the far tail is exactly 0 and never large (the 32-bit exponent taken from the shifted sum)
    assert np.all(dev[np.abs(d) == 0.0] == 1.0)
    far = d < -746.0
    assert far.sum() >= 200 and np.all(dev[far] == 0.0), dev[far].max()
    assert np.all(dev >= 0.0) and np.all(dev <= 1.0)


def test_device_math_exp_nonpos_monotone(probe):
    """non-increasing as d falls, across every change of n = round(d / ln 2) between 0 and the subnormal band"""
    ln2 = np.log(2.0)
    mids = -(np.arange(0, 1076) + 0.5) * ln2
    steps = np.arange(-6, 7)
    d = (mids[:, None] + steps[None, :] * np.spacing(np.abs(mids))[:, None]).ravel()
    d = np.concatenate([d, np.linspace(-746.0, 0.0, 200001)])
    d = np.sort(d[d <= 0.0])
    dev = probe.run(mp.EXP_NONPOS, d)
    drops = np.where(np.diff(dev) < 0.0)[0]
    assert drops.size == 0, [(d[i], dev[i], d[i + 1], dev[i + 1]) for i in drops[:8]]


def test_device_math_fast_rcp(probe, refs):
    x, ref = refs["rcp_x"], refs["rcp_ref"]
    dev = probe.run(mp.FAST_RCP, x)
    e = ulp_err(dev, ref)
    report("fast_rcp max ulp", e.max())
    assert e.max() <= 1.0, (x[np.argmax(e)], e.max())


def test_device_math_fast_rsqrt(probe, refs):
    x, ref = refs["rsqrt_x"], refs["rsqrt_ref"]
    dev = probe.run(mp.FAST_RSQRT, x)
    e = ulp_err(dev, ref)
    report("fast_rsqrt max ulp", e.max())
    assert e.max() <= 1.0, (x[np.argmax(e)], e.max())


def test_device_math_ebeta(probe, refs):
    """epilogue_values_reg's exp(Elogbeta): (z1 * rcp(z2)) * exp_nonpos(a1 - a2), the pair sum taken from the partner lane.
    The absolute error of a1 - a2 (up to 8 ulps of r, |r| ~ 2 at l of order 1: see the split above) is the relative error
    of the result, so the bound is 12 ulp, not the 8 a chain of correctly rounded steps would give."""
    ll, ref = refs["ebeta_l"], refs["ebeta_ref"]
    dev = probe.run(mp.EBETA, ll).reshape(-1, 2)
    e = ulp_err(dev, ref)
    report("Ebeta max ulp", e.max())
    i = np.unravel_index(np.argmax(e), e.shape)
    assert e.max() <= 12.0, (ll[i[0]], i[1], dev[i], ref[i][0], e.max())


@pytest.mark.parametrize("k", [3, 8, 20, 32])
def test_device_math_gamma_to_w(probe, refs, k):
    """w_k / w_max = exp(D_k), D_k = psi(g_k) - psi(g_max): its relative error is the absolute error of D_k, a few ulps
    of |D_k| (up to 700 here), so the bound is 1e-14 * max(1, |D_k|).  gamma_to_w_lean must agree bit for bit."""
    g, ratio, dk = refs[f"gamma{k}_g"], refs[f"gamma{k}_ratio"], refs[f"gamma{k}_d"]
    w = probe.run(mp.GAMMA_TO_W, g, 1.0, k).reshape(g.shape)
    lean = probe.run(mp.GAMMA_TO_W_LEAN, g, 1.0, k).reshape(g.shape)
    assert np.array_equal(w.view(np.uint64), lean.view(np.uint64)), "gamma_to_w_lean differs from gamma_to_w"
    m = np.argmax(g, axis=1)
    wr = w / w[np.arange(len(g)), m][:, None]
    normal = ratio >= TINY
    rel = np.abs(wr[normal] - ratio[normal]) / ratio[normal]
    scaled = rel / np.maximum(1.0, np.abs(dk[normal]))
    report(f"gamma_to_w<{k}> max rel (normal ratios)", rel.max())
    report(f"gamma_to_w<{k}> max rel / max(1, |D|)", scaled.max())
    report(f"gamma_to_w<{k}> max rel where |D| <= 1", rel[np.abs(dk[normal]) <= 1.0].max())
    # exponents 20 and more below the maximum are in the table (a clamp of a_k - a_max would show there)
    assert (ratio[normal] < np.exp(-20.0)).sum() >= 2 and (~normal).sum() >= 8
    assert scaled.max() <= 1e-14, (scaled.max(), np.argmax(scaled))
    # ratios that underflow stay negligible (no clamp lifts them)
    assert np.all(wr[~normal] <= 1e-300), wr[~normal].max()


@pytest.mark.parametrize("nv", list(range(1, 65)))
def test_device_math_wave_fold(probe, nv):
    """the lowest lane of every slot holds the exact wave total of that slot (small integers: every sum is exact)"""
    rng = np.random.default_rng(1000 + nv)
    waves = 3
    v = rng.integers(-1000, 1001, size=(waves, nv, 64)).astype(np.float64)
    out = probe.run(mp.WAVE_FOLD, v, 2.0 / nv, nv).reshape(waves, 64, 2)
    slot = out[0, :, 1].astype(int)
    assert set(range(nv)) <= set(slot.tolist()), sorted(set(slot.tolist()))
    for w in range(waves):
        assert np.array_equal(out[w, :, 1], out[0, :, 1])
        for s in range(nv):
            lane = int(np.where(slot == s)[0][0])
            assert out[w, lane, 0] == v[w, s].sum(), (w, s, lane, out[w, lane, 0], v[w, s].sum())


def test_device_math_codes(probe):
    """PLINK 2-bit codes -> (mom, dad, ok) and code_nibble: 00 -> y = 0, 01 -> missing, 10 -> y = 1, 11 -> y = 2"""
    out = probe.run(mp.CODES, np.array([0, 1, 2, 3], dtype=np.float64), 4.0).reshape(4, 4)
    want = np.array([[0, 2, 1, 0 | (2 << 2)], [0, 0, 0, 0], [1, 1, 1, 1 | (1 << 2)], [2, 0, 1, 2 | (0 << 2)]], dtype=np.float64)
    assert np.array_equal(out, want), out
