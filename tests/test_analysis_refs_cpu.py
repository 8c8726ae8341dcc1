"""tests/analysis_refs.py on its own: the references against a brute-force loop, and the derived bounds against a plain fp64
numpy evaluation in the engine's order -- every value within HALF of its bound (the bounds are not too tight for a correct
fp64 evaluation), and each of four subtle mutations of that evaluation outside a bound (they are not too loose to see one).
tsamd_ld (ld_ref, compare_ld) goes through the same three sections, with one mutation of its own: the band read one column off."""
import hashlib
import math

import numpy as np
import pytest
from scipy.special import digamma

import analysis_refs as ar
import late_state
from helpers import pack_bed

LD = np.longdouble


# -- a plain fp64 evaluation in the engine's order: gamma / gamma.sum, lam0 / (lam0 + lam1), theta @ eb.T --------------------------

class Fp64:
    """theta [count][k], eb [l][k], ys [l][count] (stored genotypes of the shard): the three inputs a mutation touches"""

    def __init__(self, c, shard=None):
        b, n = (0, c.n) if shard is None else shard
        self.b = b
        g = c.gamma[b:b + n]
        self.theta = g / g.sum(axis=1, keepdims=True)
        self.lam = c.lam.copy()
        self.ys = ar.stored_genotypes(c.y, c.held, shard)
        self.gamma, self.alpha = g, c.alpha

    @property
    def eb(self):
        return self.lam[:, :, 0] / (self.lam[:, :, 0] + self.lam[:, :, 1])

    def q(self, locs):
        return self.theta @ self.eb[locs].T, self.ys[locs].T  # [count][J]

    def loglik(self, locs):
        q, y = self.q(locs)
        ok = y != 3
        prod = np.where(y == 0, (1.0 - q) * (1.0 - q), np.where(y == 1, 2.0 * q * (1.0 - q), q * q))
        t = np.where(ok, np.log(np.maximum(prod, 1e-30)), 0.0)
        out = dict(loc_sums=t.sum(axis=0), loc_counts=ok.sum(axis=0), indiv_sums=t.sum(axis=1), indiv_counts=ok.sum(axis=1))
        out["sum"], out["count"] = out["loc_sums"].sum(), int(ok.sum())
        return out

    def scan(self, locs, trait=None):
        q, y = self.q(locs)
        ok = y != 3
        h, r = 2.0 * q * (1.0 - q), np.where(ok, y, 0) - 2.0 * q
        out = dict(fit_sums=np.stack([np.where(ok, t, 0.0).sum(axis=0) for t in ((1.0 - q) ** 2, h, q * q, h * (1.0 - h))], axis=1),
                   fit_counts=np.stack([(y == v).sum(axis=0) for v in (0, 1, 2)], axis=1).astype(np.uint32))
        if trait is not None:
            has = ~np.isnan(trait)
            t = np.where(has, trait, 0.0)[:, None]
            m = ok & has[:, None]
            terms = (t + 0.0 * q, t * r, t * t * h, t * h, r, h)
            out.update(trait_sums=np.stack([np.where(m, x, 0.0).sum(axis=0) for x in terms], axis=1),
                       trait_counts=m.sum(axis=0).astype(np.uint32))
        return out

    def kin(self, ids, locs):
        rows = np.asarray(ids, dtype=np.int64) - self.b
        q, y = self.q(locs)
        q, y = q[rows], y[rows]
        ok = y != 3
        r = np.where(ok, y - 2.0 * q, 0.0)
        s = np.where(ok, np.sqrt(q * (1.0 - q)), 0.0)
        num, den = r @ r.T, s @ s.T
        with np.errstate(divide="ignore", invalid="ignore"):
            kin = np.where(den != 0.0, num / (4.0 * den), 0.0)
        return kin, num, den

    def ld(self, locs, window):
        """dict(num, cnt), bands [J][window + 1], in ld_terms' order: 2 q (1 - q), y - (q + q), one sqrt, one division"""
        q, y = self.q(np.arange(len(self.ys)) if locs is None else locs)
        h = 2.0 * q * (1.0 - q)
        ok = (y != 3) & (h > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(ok, (np.where(ok, y, 0) - (q + q)) / np.sqrt(h), 0.0)
        m = ok.astype(np.float64)
        J = z.shape[1]
        num, cnt = np.zeros((J, window + 1)), np.zeros((J, window + 1))
        for d in range(min(window, J - 1) + 1):
            num[:J - d, d] = (z[:, :J - d] * z[:, d:]).sum(axis=0)
            cnt[:J - d, d] = (m[:, :J - d] * m[:, d:]).sum(axis=0)
        return dict(num=num, cnt=cnt.astype(np.uint32))

    def foldin(self, locs, iters):
        y = self.ys[locs].T
        mom, dad = np.where(y == 3, 0.0, y), np.where(y == 3, 0.0, 2.0 - y)
        lam = self.lam[locs]
        eb = np.exp(digamma(lam) - digamma(lam.sum(axis=2, keepdims=True)))
        e0, e1 = eb[:, :, 0], eb[:, :, 1]
        g = self.gamma.copy()
        for _ in range(iters):
            w = np.exp(digamma(g) - digamma(g.sum(axis=1, keepdims=True)))
            gn = self.alpha + w * ((mom / (w @ e0.T)) @ e0 + (dad / (w @ e1.T)) @ e1)
            change = np.abs(gn - g).sum(axis=1) / gn.sum(axis=1)
            g = gn
        return g, dict(iters=np.full(len(g), iters, dtype=np.uint32), change=change)


def all_refs(c, shard=None, iters=(1, 3)):
    tr = c.trait if shard is None else c.trait[shard[0]:shard[0] + shard[1]]
    args = (c.y, c.gamma, c.lam)
    return dict(loglik=ar.loglik_ref(*args, c.held, c.locs, shard), scan=ar.scan_ref(*args, c.held, c.locs, shard, tr),
                kin=ar.kin_ref(*args, c.ids, c.held, c.locs, shard), foldin=ar.foldin_ref(*args, c.alpha, iters, c.held, c.locs, shard))


def compare_all(f, c, refs, shard=None, limit=0.5, iters=(1, 3)):
    """{family: worst |fp64 - ref| / bound}; asserts every value within limit x its bound"""
    tr = c.trait if shard is None else c.trait[shard[0]:shard[0] + shard[1]]
    worst = dict(loglik=ar.compare_loglik(f.loglik(c.locs), *refs["loglik"], limit=limit), scan=ar.compare_scan(f.scan(c.locs, tr), *refs["scan"], limit=limit),
                 kin=ar.compare_kin(f.kin(c.ids, c.locs), *refs["kin"], limit=limit))
    worst["foldin"] = max(ar.compare_foldin(*f.foldin(c.locs, i), refs["foldin"][i], limit=limit) for i in iters)
    return worst


def ld_refs(c, window, shard=None):
    """{list: (ref, bound)} of the full list (None) and of c.locs, from one Entries"""
    every = ar.Entries(c.y, c.gamma, c.lam, c.held, None, shard)
    return {key: ar.ld_ref(c.y, c.gamma, c.lam, window, c.held, which, shard, entries=every) for key, which in (("all", None), ("list", c.locs))}


def compare_ld_lists(f, c, refs, window, limit=0.5):
    return max(ar.compare_ld(f.ld(which, window), *refs[key], limit=limit) for key, which in (("all", None), ("list", c.locs)))


# -- 1. brute force ----------------------------------------------------------------------------------------------------------------

def test_the_references_equal_a_brute_force_loop():
    n, l, k = 37, 9, 3
    rng = np.random.default_rng(1)
    y = rng.integers(0, 4, size=(l, n)).astype(np.uint8)
    gamma = rng.gamma(2.0, 3.0, size=(n, k))
    lam = rng.gamma(2.0, 5.0, size=(l, k, 2)) + 0.1
    held = {0: np.array([0, 7, n - 1]), 4: np.array([3]), l - 1: np.array([n - 1])}
    locs = np.array([8, 0, 3, 3, 4], dtype=np.int64)
    ids = np.array([5, 36, 0, 11, 5], dtype=np.int64)
    trait = ar.make_trait(n, 2, nan_rate=0.2)
    alpha = 1.0 / k
    heldset = {(int(loc), int(i)) for loc, v in held.items() for i in v}
    J, m = len(locs), len(ids)

    def qof(i, loc):
        gs = sum(LD(gamma[i, a]) for a in range(k))
        return sum(LD(lam[loc, a, 0]) / (LD(lam[loc, a, 0]) + LD(lam[loc, a, 1])) * (LD(gamma[i, a]) / gs) for a in range(k))

    def stored(i, loc):
        return y[loc, i] != 3 and (loc, i) not in heldset

    zero = LD(0)
    ll = dict(loc_sums=[zero] * J, loc_counts=[0] * J, indiv_sums=[zero] * n, indiv_counts=[0] * n)
    fit, fitc = [[zero] * 4 for _ in range(J)], [[0] * 3 for _ in range(J)]
    trs, trc = [[zero] * 6 for _ in range(J)], [0] * J
    r = [[zero] * J for _ in range(n)]
    s = [[zero] * J for _ in range(n)]
    for jj, loc in enumerate(locs):
        for i in range(n):
            if not stored(i, loc):
                continue
            q, yv = qof(i, loc), int(y[loc, i])
            p = (1 - q) ** 2 if yv == 0 else 2 * q * (1 - q) if yv == 1 else q * q
            t = np.log(max(p, LD("1e-30")))
            ll["loc_sums"][jj] += t
            ll["indiv_sums"][i] += t
            ll["loc_counts"][jj] += 1
            ll["indiv_counts"][i] += 1
            h = 2 * q * (1 - q)
            for col, v in enumerate(((1 - q) ** 2, h, q * q, h * (1 - h))):
                fit[jj][col] += v
            fitc[jj][yv] += 1
            r[i][jj], s[i][jj] = yv - 2 * q, np.sqrt(q * (1 - q))
            if not math.isnan(trait[i]):
                tv = LD(trait[i])
                for col, v in enumerate((tv, tv * r[i][jj], tv * tv * h, tv * h, r[i][jj], h)):
                    trs[jj][col] += v
                trc[jj] += 1
    tiny = 1e-2  # of the bound: the two long-double evaluations differ in their order only
    ref, bound = ar.loglik_ref(y, gamma, lam, held, locs)
    for key in ("loc_sums", "indiv_sums"):
        assert ar.ratio(np.array(ll[key], dtype=LD), ref[key], bound[key]) <= tiny
    assert list(ref["loc_counts"]) == ll["loc_counts"] and list(ref["indiv_counts"]) == ll["indiv_counts"]
    assert ref["count"] == sum(ll["loc_counts"]) and ar.ratio(sum(ll["loc_sums"]), ref["sum"], bound["sum"]) <= tiny
    ref, bound = ar.scan_ref(y, gamma, lam, held, locs, trait=trait)
    assert ar.ratio(np.array(fit, dtype=LD), ref["fit_sums"], bound["fit_sums"]) <= tiny
    assert ar.ratio(np.array(trs, dtype=LD), ref["trait_sums"], bound["trait_sums"]) <= tiny
    assert ref["fit_counts"].tolist() == fitc and ref["trait_counts"].tolist() == trc
    assert set(ar.scan_ref(y, gamma, lam, held, locs)[0]) == {"fit_sums", "fit_counts"}
    ref, bound = ar.kin_ref(y, gamma, lam, ids, held, locs)
    num = np.array([[sum(r[a][j] * r[b][j] for j in range(J)) for b in ids] for a in ids], dtype=LD)
    den = np.array([[sum(s[a][j] * s[b][j] for j in range(J)) for b in ids] for a in ids], dtype=LD)
    kin = np.array([[num[a, b] / (4 * den[a, b]) if den[a, b] > 0 else zero for b in range(m)] for a in range(m)], dtype=LD)
    for key, v in (("num", num), ("den", den), ("kin", kin)):
        assert ar.ratio(v, ref[key], bound[key]) <= tiny, key
    # LD at window 3: individual after individual, pair after pair of list positions; the list's repeat (positions 2 and 3)
    # is a pair of its own
    w = 3
    ldnum, ldabs, ldcnt = [[zero] * (w + 1) for _ in range(J)], [[zero] * (w + 1) for _ in range(J)], [[0] * (w + 1) for _ in range(J)]
    for i in range(n):
        zi = [(r[i][jj] / np.sqrt(2 * qof(i, loc) * (1 - qof(i, loc))) if stored(i, loc) else None) for jj, loc in enumerate(locs)]
        for a in range(J):
            for d in range(w + 1):
                if a + d < J and zi[a] is not None and zi[a + d] is not None:
                    ldnum[a][d] += zi[a] * zi[a + d]
                    ldabs[a][d] += abs(zi[a] * zi[a + d])
                    ldcnt[a][d] += 1
    ref, bound = ar.ld_ref(y, gamma, lam, w, held, locs)
    assert ref["num"].shape == (J, w + 1) and ref["cnt"].dtype == np.uint32 and ref["cnt"].tolist() == ldcnt
    assert ar.ratio(np.array(ldnum, dtype=LD), ref["num"], bound["num"]) <= tiny
    assert ar.ratio(np.array(ldabs, dtype=LD), ref["absn"], bound["num"]) <= tiny
    assert ldcnt[2][1] == ldcnt[2][0] == ldcnt[3][0] and ldcnt[3][2] == 0 and ref["num"][4, 1] == 0  # the repeat; past the end
    wide = ar.ld_ref(y, gamma, lam, 7, held, locs)[0]  # (wider than the list: the band from the full product)
    assert np.array_equal(wide["cnt"][:, :w + 1], ref["cnt"]) and np.all(wide["cnt"][:, J:] == 0) and np.all(wide["num"][:, J:] == 0)
    assert ar.ratio(wide["num"][:, :w + 1], ref["num"], bound["num"]) <= tiny
    narrow, nbound = ar.ld_ref(y, gamma, lam, 1, held, locs)  # (a narrow band: the shifted products)
    assert np.array_equal(narrow["cnt"], ref["cnt"][:, :2]) and ar.ratio(narrow["num"], ref["num"][:, :2], bound["num"][:, :2]) <= tiny
    assert ar.ratio(nbound["num"], bound["num"][:, :2], bound["num"][:, :2]) <= tiny
    # fold-in, two updates
    g = [[LD(gamma[i, a]) for a in range(k)] for i in range(n)]
    for it in (1, 2):
        new, change = [], []
        for i in range(n):
            g64 = [float(v) for v in g[i]]
            w = [np.exp(LD(digamma(v)) - LD(digamma(math.fsum(g64)))) for v in g64]
            acc = [zero] * k
            for loc in locs:
                if not stored(i, loc):
                    continue
                e = [[np.exp(LD(digamma(lam[loc, a, t])) - LD(digamma(lam[loc, a, 0] + lam[loc, a, 1]))) for t in (0, 1)] for a in range(k)]
                s0, s1 = sum(w[a] * e[a][0] for a in range(k)), sum(w[a] * e[a][1] for a in range(k))
                for a in range(k):
                    acc[a] += int(y[loc, i]) * e[a][0] / s0 + (2 - int(y[loc, i])) * e[a][1] / s1
            row = [LD(alpha) + w[a] * acc[a] for a in range(k)]
            change.append(sum(abs(row[a] - g[i][a]) for a in range(k)) / sum(row))
            new.append(row)
        g = new
        snap = ar.foldin_ref(y, gamma, lam, alpha, (1, 2), held, locs)[it]
        assert np.max(np.abs(np.array(g, dtype=LD) - snap["gamma"]) / snap["gamma"]) <= 1e-15
        assert np.max(np.abs(np.array(change, dtype=LD) - snap["change"])) <= 1e-15 and np.all(snap["iters"] == it)
    assert ar.foldin_sum_error(snap["gamma"], k, alpha, ll["indiv_counts"]) <= 1e-15
    ys = ar.stored_genotypes(y, held)
    assert np.array_equal(ar.bed_bytes(ys)[:, :-1], pack_bed(ys)[:, :-1])
    assert np.all(ar.bed_bytes(ys)[:, -1] >> 2 == 0b010101)  # n = 37: three padding entries, 01


# -- 2. the bounds hold for a correct fp64 evaluation, with a factor two to spare -----------------------------------------------------

@pytest.mark.parametrize("k", [1, 4, 9, 17, 32, 33])
def test_fp64_numpy_lies_within_half_of_every_bound_every_k(k):
    c = ar.plant_every_k(k)
    print(k, compare_all(Fp64(c), c, all_refs(c)))
    c = ar.plant_every_k(k, n=602, l=150)  # the GPU test's shape of tsamd_ld
    print(k, "ld", compare_ld_lists(Fp64(c), c, ld_refs(c, 65), 65))


LATE_LD_WINDOW = 39  # l - 1 of the widest late shape: every pair of either list


@pytest.fixture(scope="module")
def late_refs():
    """{shape: (case, references)}, computed once"""
    out = {}
    for shape in ar.LATE_SHAPES:
        c, _ = ar.plant_late(*shape)
        out[shape] = (c, all_refs(c, c.shard, iters=(1, 5)))
        out[shape][1]["ld_lists"] = ld_refs(c, LATE_LD_WINDOW, c.shard)
        out[shape][1]["ld"] = out[shape][1]["ld_lists"]["list"]
    return out


@pytest.mark.parametrize("shape", ar.LATE_SHAPES)
def test_fp64_numpy_lies_within_half_of_every_bound_late_state(late_refs, shape):
    c, refs = late_refs[shape]
    e = ar.Entries(c.y, c.gamma, c.lam, c.held, None, c.shard)
    print(shape, "min q %.2e min 1-q %.2e" % (float(e.q.min()), float(e.omq.min())), compare_all(Fp64(c, c.shard), c, refs, c.shard, iters=(1, 5)))
    z = np.where(e.ok, e.r / np.sqrt(e.h), 0)
    print(shape, "max |z| %.0f" % float(np.abs(z).max()), "ld", compare_ld_lists(Fp64(c, c.shard), c, refs["ld_lists"], LATE_LD_WINDOW),
          "worst bound / sum |z z| %.2e" % float(np.max(refs["ld_lists"]["all"][1]["num"] / np.maximum(refs["ld_lists"]["all"][0]["absn"], LD("1e-300")))))
    eb = ar.ebeta_ref(c.lam)
    assert eb.min() < 1e-4 and 1 - eb.max() < 1e-4 and c.gamma.min() == 1e-8 and c.gamma.max() > 1e5  # late indeed
    # a floor row's w underflows: one update puts its floor components at alpha exactly
    g1 = refs["foldin"][1]["gamma"]
    rows = c.floor_rows[(c.floor_rows >= c.shard[0]) & (c.floor_rows < c.shard[0] + c.shard[1])]
    assert len(rows) > 0
    for i in rows:
        at_floor = c.gamma[i] == 1e-8
        assert at_floor.any() and np.all(g1[i - c.shard[0]][at_floor] == LD(c.alpha))


# -- 3. the bounds can tell a wrong kernel -------------------------------------------------------------------------------------------

def outside(f, c, refs, shard, families):
    """the families in which the (mutated) evaluation f leaves a bound or a count"""
    tr = c.trait[shard[0]:shard[0] + shard[1]]
    calls = dict(loglik=lambda: ar.compare_loglik(f.loglik(c.locs), *refs["loglik"]), scan=lambda: ar.compare_scan(f.scan(c.locs, tr), *refs["scan"]),
                 kin=lambda: ar.compare_kin(f.kin(c.ids, c.locs), *refs["kin"]),
                 foldin=lambda: ar.compare_foldin(*f.foldin(c.locs, 1), refs["foldin"][1]),
                 ld=lambda: ar.compare_ld(f.ld(c.locs, LATE_LD_WINDOW), *refs["ld"]))
    out = set()
    for name in families:
        try:
            calls[name]()
        except AssertionError:
            out.add(name)
    return out


def test_each_mutation_leaves_a_bound(late_refs):
    shape = ar.LATE_SHAPES[0]
    c, refs = late_refs[shape]
    shard, every = c.shard, {"loglik", "scan", "kin", "foldin", "ld"}
    assert outside(Fp64(c, shard), c, refs, shard, every) == set()
    ll, llb = refs["loglik"]
    e = ar.Entries(c.y, c.gamma, c.lam, c.held, c.locs, shard)
    listed = [int(i) for i in c.ids]
    has = ~np.isnan(c.trait)

    # one theta component scaled by 1 + 1e-9: the listed, phenotyped individual with the tightest per-individual bound, its
    # largest component.  The exact change of its sum is sum_j dterm/dq 1e-9 Ebeta_k theta_k: at least ten times the bound.
    cand = [i for i in listed if has[i]]
    n0 = min(cand, key=lambda i: float(llb["indiv_sums"][i]))
    k0 = int(np.argmax(c.gamma[n0]))
    dq = LD(1e-9) * ar.ebeta_ref(c.lam[e.locs])[:, k0] * ar.theta_ref(c.gamma[n0:n0 + 1])[0, k0]  # [J]
    q, om, ys = e.q[:, n0], e.omq[:, n0], e.ys[:, n0]
    dterm = np.where(ys == 0, -2 / om, np.where(ys == 1, 1 / q - 1 / om, 2 / q)) * dq
    change = abs(np.where(ys != 3, dterm, 0).sum())
    assert change >= 10 * llb["indiv_sums"][n0], (float(change), float(llb["indiv_sums"][n0]))
    f = Fp64(c, shard)
    f.theta[n0, k0] *= 1.0 + 1e-9
    assert outside(f, c, refs, shard, {"loglik", "scan", "kin"}) == {"loglik", "scan", "kin"}
    # tsamd_ld sums over every individual of the shard: the largest GAMMA component of individual 17 scaled by 1 + 1e-9 and
    # the row normalised again, a far smaller step (theta_k moves by 1e-9 theta_k (1 - theta_k), q by 1e-9 theta_k
    # (Ebeta_k - q)).  With dz/dq = -2 / sqrt(h) - z (1 - 2q) / h the exact change of the individual's own term of a pair,
    # z_i dz_j + z_j dz_i, is more than 1.5 times the bound in one entry of the band
    n0 = 17
    k0 = int(np.argmax(c.gamma[n0]))
    q, h = e.q[:, n0], e.h[:, n0]
    dq = LD(1e-9) * ar.theta_ref(c.gamma[n0:n0 + 1])[0, k0] * (ar.ebeta_ref(c.lam[e.locs])[:, k0] - q)
    z = e.r[:, n0] / np.sqrt(h)
    z = np.where(e.ok[:, n0], z, 0)
    dz = np.where(e.ok[:, n0], (-2 / np.sqrt(h) - z * (1 - 2 * q) / h) * dq, 0)
    change = np.abs(ar._band(np.outer(z, dz) + np.outer(dz, z), LATE_LD_WINDOW))
    bound = refs["ld"][1]["num"]
    over = float(np.max(np.where(change > 0, change / np.where(bound > 0, bound, 1), 0)))
    print("ld, gamma[17][%d] scaled by 1 + 1e-9: exact change / bound = %.2f" % (k0, over))
    assert over >= 1.5  # (section 2: the fp64 evaluation's own error takes at most 0.5 of the bound back)
    f = Fp64(c, shard)
    g = f.gamma[n0].copy()
    g[k0] *= 1.0 + 1e-9
    f.theta[n0] = g / g.sum()
    assert outside(f, c, refs, shard, {"ld"}) == {"ld"}

    # two neighbouring individuals' genotypes swapped at one listed location: both listed ids' neighbours would do; take the
    # first listed location and the first pair (n, n + 1) with n listed, both stored and phenotyped, different genotypes and
    # different trait values.  Each one's term changes by a whole genotype step: r by 1 or 2 against a bound of order 1e-13.
    loc = int(c.locs[0])
    ys0 = ar.stored_genotypes(c.y, c.held)[loc]
    pair = next(i for i in listed if i + 1 < c.n and ys0[i] != 3 and ys0[i + 1] != 3 and ys0[i] != ys0[i + 1] and has[i] and has[i + 1])
    assert abs(c.trait[pair] - c.trait[pair + 1]) > 1e-3
    ya, yb = int(ys0[pair]), int(ys0[pair + 1])

    def term(q, yv):
        return np.log(max((1 - q) ** 2 if yv == 0 else 2 * q * (1 - q) if yv == 1 else q * q, ar.CLAMP))

    assert list(c.locs).count(loc) == 1  # (row 0 of the listed entries, and no other)
    assert abs(term(e.q[0, pair], yb) - term(e.q[0, pair], ya)) >= 10 * llb["indiv_sums"][pair]
    assert abs((c.trait[pair] - c.trait[pair + 1]) * (yb - ya)) >= 10 * refs["scan"][1]["trait_sums"][0, 1]  # sum t r of that location
    a = listed.index(pair)  # num[a][a] = sum_j r^2
    assert abs((e.r[0, pair] + (yb - ya)) ** 2 - e.r[0, pair] ** 2) >= 10 * refs["kin"][1]["num"][a, a]
    f = Fp64(c, shard)
    f.ys[loc, [pair, pair + 1]] = f.ys[loc, [pair + 1, pair]]
    assert outside(f, c, refs, shard, every) == every

    # one held-out entry counted as stored: a listed individual of a listed held-out location
    loc = next(int(x) for x in c.locs if int(x) in c.held)
    n1 = int(c.held[loc][0])
    f = Fp64(c, shard)
    assert f.ys[loc, n1] == 3 and c.y[loc, n1] != 3
    f.ys[loc, n1] = c.y[loc, n1]
    assert outside(f, c, refs, shard, {"loglik", "scan", "foldin", "ld"}) == {"loglik", "scan", "foldin", "ld"}
    got = f.ld(c.locs, LATE_LD_WINDOW)
    row = list(c.locs).index(loc)
    assert got["cnt"][row, 0] == refs["ld"][0]["cnt"][row, 0] + 1  # (the count it is: ratio() alone would not see it)
    ids = c.ids.copy()
    ids[1] = n1  # (the kinship list need not hold that individual: put it there)
    kin_refs = dict(kin=ar.kin_ref(c.y, c.gamma, c.lam, ids, c.held, c.locs, shard))
    kept, c.ids = c.ids, ids
    try:
        assert outside(Fp64(c, shard), c, kin_refs, shard, {"kin"}) == set()
        assert outside(f, c, kin_refs, shard, {"kin"}) == {"kin"}
    finally:
        c.ids = kept

    # lambda's two sides swapped at one listed location: Ebeta becomes 1 - Ebeta there
    loc = int(c.locs[2])
    f = Fp64(c, shard)
    f.lam[loc] = f.lam[loc][:, ::-1]
    assert outside(f, c, refs, shard, every) == every


def test_a_band_read_one_column_off_leaves_the_bound(late_refs):
    """tsamd_ld's own wrong read-out: column d + 1 of the band where d belongs (the last column 0), the counts as they are"""
    c, refs = late_refs[ar.LATE_SHAPES[0]]
    ref, bound = refs["ld"]
    got = Fp64(c, c.shard).ld(c.locs, LATE_LD_WINDOW)
    assert ar.compare_ld(got, ref, bound) <= 0.5
    off = dict(num=np.concatenate([got["num"][:, 1:], np.zeros((len(c.locs), 1))], axis=1), cnt=got["cnt"])
    with pytest.raises(AssertionError):
        ar.compare_ld(off, ref, bound)
    # and the counts one column off on their own
    off = dict(num=got["num"], cnt=np.concatenate([got["cnt"][:, 1:], np.zeros((len(c.locs), 1), dtype=np.uint32)], axis=1))
    with pytest.raises(AssertionError):
        ar.compare_ld(off, ref, bound)


def test_fp64_numpy_ld_lies_within_half_of_the_bound_at_the_wide_late_shape():
    """(1030, 150, 8), window 65: the late shape the GPU test runs under the test hooks (three location tiles, two overlap tiles)"""
    c, _ = ar.plant_late(1030, 150, 8)
    print("late (1030, 150, 8) ld", compare_ld_lists(Fp64(c, c.shard), c, ld_refs(c, 65, c.shard), 65))


# -- 4. plant() without n_eff is what it was -------------------------------------------------------------------------------------------

def digest(s):
    h = hashlib.sha256()
    for a in (s.y, s.payload, s.gamma, s.counts, s.lam, s.floor_rows):
        h.update(np.ascontiguousarray(a).tobytes())
    for loc in sorted(s.held):
        h.update(np.uint32(loc).tobytes())
        h.update(s.held[loc].tobytes())
    return h.hexdigest()


def test_plant_without_n_eff_is_bit_for_bit_what_it_was():
    """the digest was taken on the commit before plant() got n_eff"""
    assert digest(late_state.plant(1030, 24, 8, 5)) == "49fad84ced020dd32b69068e82b50e186e222a7dba2fd6fec1ee632da5ad3985"
    a, b = late_state.plant(1030, 24, 8, 5, n_eff=1e6), late_state.plant(1030, 24, 8, 5)
    assert np.array_equal(a.gamma, b.gamma) and np.array_equal(a.y, b.y) and a.lam.max() > 100 * b.lam.max()


def test_shard_of_is_the_librarys_rule():
    assert ar.shard_of(1030, 1, 3) == (344, 344) and ar.shard_of(1030, 2, 3) == (688, 342) and ar.shard_of(1030, 0, 1) == (0, 1030)
    assert ar.shard_of(1030, 1, 3)[0] % 16 != 0
