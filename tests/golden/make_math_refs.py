"""Generates tests/golden/device_math_refs.npz: inputs of the engine's device math primitives (csrc/tsamd_device.h,
gamma_to_w in csrc/tsamd_kernels.h) and their exact values from mpmath at 50 significant digits.

Every reference is stored as a double-double (hi, lo): hi is the correctly rounded double, lo = exact - hi rounded to a
double, so an error of a fraction of an ulp is measured against the exact value, not against another rounding.  For
exp_nonpos results in the subnormal band the table holds exp(d) * 2^1074 as well (spacings of the subnormal grid).

    python tests/golden/make_math_refs.py          # rewrites the fixture (deterministic: fixed seed)

tests/test_device_math_cpu.py re-derives a random sample of every table with the functions below, so the fixture
cannot drift from them silently; tests/test_gpu_device_math.py compares the device with it.
"""
import os

import mpmath
import numpy as np

DPS = 50
SEED = 20261016
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_math_refs.npz")
GAMMA_KS = (3, 8, 20, 32)
PSI_ROOT = 1.4616321449683622  # the positive zero of psi, rounded to double

mpmath.mp.dps = DPS
mpf = mpmath.mpf


def dd(v):
    """exact mpf -> (hi, lo): hi the correctly rounded double (mpmath rounds to nearest on conversion), lo the rest"""
    hi = float(v)
    lo = float(v - mpf(hi))
    return hi, lo


def ref_digamma(x):
    return dd(mpmath.digamma(mpf(float(x))))


def ref_exp_digamma_split(x):
    """(exp(psi(x)) as (hi, lo), a = psi(x) - log(z) as (hi, lo)) with z = x + 10 rounded to double, as the device forms it"""
    x = float(x)
    psi = mpmath.digamma(mpf(x))
    z = x + 10.0
    return dd(mpmath.exp(psi)), dd(psi - mpmath.log(mpf(z)))


def ref_exp(d):
    """(hi, lo, exp(d) * 2^1074): the last one counts spacings of the subnormal grid"""
    v = mpmath.exp(mpf(float(d)))
    hi, lo = dd(v)
    return hi, lo, float(v * mpmath.power(2, 1074))


def ref_rcp(x):
    return dd(1 / mpf(float(x)))


def ref_rsqrt(x):
    return dd(1 / mpmath.sqrt(mpf(float(x))))


def ref_ebeta(l0, l1):
    """(Ebeta_0, Ebeta_1) = exp(psi(l_t) - psi(l0 + l1)), the pair sum rounded to double as the epilogue forms it"""
    l0, l1 = float(l0), float(l1)
    ps = mpmath.digamma(mpf(l0 + l1))
    return dd(mpmath.exp(mpmath.digamma(mpf(l0)) - ps)), dd(mpmath.exp(mpmath.digamma(mpf(l1)) - ps))


def ref_gamma_row(g):
    """per component: D_k = psi(g_k) - psi(g_max) and exp(D_k) = w_k / w_max (the weights gamma_to_w forms up to a factor)"""
    psi = [mpmath.digamma(mpf(float(v))) for v in g]
    m = int(np.argmax(g))
    dk = [p - psi[m] for p in psi]
    return np.array([float(v) for v in dk]), np.array([float(mpmath.exp(v)) for v in dk])


def loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    tiny = np.nextafter(1e8, 0.0), 1e8, np.nextafter(1e8, np.inf)
    root = [PSI_ROOT + k * np.spacing(PSI_ROOT) for k in range(-8, 9)] + [PSI_ROOT + s for s in (-1e-6, -1e-9, 1e-9, 1e-6)]
    out = {}
    out["digamma_x"] = np.concatenate([loguniform(rng, 1e-8, 1e12, 2000), [1e-8, 1.0, 10.0, 2e6, 1e12], tiny, root])
    out["split_x"] = np.concatenate([loguniform(rng, 1e-8, 1e7, 1500), [1e-8, 1e-3, 0.05, 1.0, PSI_ROOT, 10.0, 2e6, 1e7]])
    far = -loguniform(rng, 746.0, 1.4e9, 200)
    out["exp_d"] = np.concatenate([
        rng.uniform(-746.0, 0.0, 2000),
        rng.uniform(-745.2, -708.4, 1000),  # results in the subnormal band
        -loguniform(rng, 1e-300, 1.0, 200),  # |d| small: n = 0, r = d
        [0.0, -0.0, -708.3964185322641, -708.3964185322642, -745.1332191019411, -745.1332191019412, -745.2, -746.0,
         -0.34657359027997264, -0.3465735902799727, -0.6931471805599453, -1.4e9],
        far])
    m = rng.uniform(1.0, 2.0, 2000)
    e = rng.integers(-1000, 1001, 2000)
    out["rcp_x"] = np.concatenate([np.ldexp(m, e), [1.0, 2.0, 3.0, np.nextafter(2.0, 0.0), 2.0 ** -1000, 2.0 ** 1000]])
    out["rsqrt_x"] = np.concatenate([
        loguniform(rng, 2.0, 1e10, 1500),
        np.ldexp(rng.uniform(1.0, 2.0, 500), rng.integers(-1000, 1001, 500)),
        [2.0, 3.0, 4.0, 1e6 + 2.0, 1e10, np.nextafter(4.0, 0.0)]])
    ll = loguniform(rng, 1.0, 4e6, 2 * 1200).reshape(1200, 2)
    out["ebeta_l"] = np.concatenate([ll, [[1.0, 4e6], [4e6, 1.0], [1.0, 1.0], [4e6, 4e6], [1.0, 2.0]]])
    for k in GAMMA_KS:
        rows = []
        for i in range(48):
            kind = i % 4
            if kind == 0:  # components log-uniform over the whole range
                g = loguniform(rng, 1e-8, 2e6, k)
            else:  # late-training rows: alpha + (K alpha + 2 L) theta, theta ~ Dirichlet(0.05)
                alpha = 1.0 / k
                theta = rng.dirichlet(np.full(k, 0.05))
                g = alpha + (k * alpha + 2.0 * rng.choice([5e5, 1e6])) * theta
                if kind == 2:  # a few components at the floor
                    g[rng.choice(k, size=max(1, k // 4), replace=False)] = 1e-8
                if kind == 3:  # mid-range: exponents 20 to 40 below the maximum stay representable
                    g = np.maximum(g, loguniform(rng, 0.02, 3.0, k))
            rows.append(g)
        out[f"gamma{k}_g"] = np.array(rows)
    return out


def references(inp):
    out = dict(inp)
    hi_lo = lambda f, xs: np.array([f(x) for x in xs], dtype=np.float64)  # noqa: E731
    out["digamma_ref"] = hi_lo(ref_digamma, inp["digamma_x"])
    sp = [ref_exp_digamma_split(x) for x in inp["split_x"]]
    out["split_expsi"] = np.array([s[0] for s in sp])
    out["split_a"] = np.array([s[1] for s in sp])
    out["exp_ref"] = hi_lo(ref_exp, inp["exp_d"])
    out["rcp_ref"] = hi_lo(ref_rcp, inp["rcp_x"])
    out["rsqrt_ref"] = hi_lo(ref_rsqrt, inp["rsqrt_x"])
    eb = [ref_ebeta(a, b) for a, b in inp["ebeta_l"]]
    out["ebeta_ref"] = np.array([[e[0], e[1]] for e in eb])  # [pair][side][hi, lo]
    for k in GAMMA_KS:
        r = [ref_gamma_row(g) for g in inp[f"gamma{k}_g"]]
        out[f"gamma{k}_d"] = np.array([x[0] for x in r])
        out[f"gamma{k}_ratio"] = np.array([x[1] for x in r])
    return out


def main():
    refs = references(inputs())
    np.savez_compressed(OUT, **refs)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(refs)} arrays)")


if __name__ == "__main__":
    main()
