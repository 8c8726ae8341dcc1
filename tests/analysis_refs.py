"""Extended-precision references, with derived error bounds, of five analysis calls: tsamd_train_loglik, tsamd_snp_scan,
tsamd_kinship, tsamd_fold_in and tsamd_ld.

Every function takes PLANTED inputs only -- the genotypes y [l][n] in {0, 1, 2, 3 = missing}, gamma [n][k], lambda [l][k][2],
the held-out lists {location: global ids}, the trait, the id list -- and never a value read back from an engine, so a getter
that is consistently wrong, a held-out fold on the wrong individuals, a wrong shard offset or a stale copy of w / eb cannot
leave kernel and reference in agreement.  `shard` = (begin, count) cuts the planted arrays to an engine's shard.

All arithmetic is numpy long double (x87 80 bit: eps 1.1e-19, a thousand times below fp64's), sums are long-double
reductions.  Only psi comes from scipy.special.digamma in fp64 (fold-in, whose tolerance is the project's relative 1e-9).

Bounds.  Each reference comes with a bound of the same shape on |fp64 evaluation - reference|, derived to first order with
u = 2^-53, not measured:
  * q = sum_k Ebeta_k theta_k has relative error c_q = (2K + 4) u: theta = gamma / sum (K - 1 additions and a division: K u),
    Ebeta = lambda0 / (lambda0 + lambda1) (an addition and a division: 2 u), K multiply-adds of positive terms ((K + 1) u);
  * 1 - q has relative error d1 = q c_q / (1 - q) + u (the cancellation), r = y - 2q absolute error 2 q c_q + u |r|,
    h = 2 q (1 - q) relative error c_q + d1, s = sqrt(q (1 - q)) relative error (c_q + d1) / 2 + 2 u;
  * the log and the products of an entry's term add 4 u (1 + |term|);
  * a sum of M terms adds M u sum |term|, whatever its order;
  * the per-location and per-individual sums of train_loglik and snp_scan carry a factor 4 on top, for the kernels' own
    summation order and multiply-add contraction; the kinship bound is the worst-order bound as it stands:
    sum_j (|r_a| dr_b + |r_b| dr_a) + (J + 2) u sum_j |r_a r_b| for num, the same with s for den, the quotient rule for kin;
  * tsamd_ld's z = r / sqrt(h) (0 where the entry is not stored or h <= 0) has absolute error
    dz = dr / sqrt(h) + |z| ((c_q + d1) / 2 + 3 u): the error of r, half the relative error of h, then one rounding each for
    the product 2 q (1 - q) behind the root, the root and the division; num of the pair of list positions (i, i + d) gets
    the worst-order bound as it stands, like kinship's and without the factor 4:
    sum_n (|z_i| dz_{i+d} + |z_{i+d}| dz_i) + (M + 2) u sum_n |z_i z_{i+d}|, M the shard's individuals; cnt is exact.
An entry whose exact product C(2,y) q^y (1-q)^(2-y) lies in [1e-31, 1e-29] is refused: at the 1e-30 clamp of the
log-likelihood term a rounding decides between two different terms and no bound holds.
"""
import numpy as np
from scipy.special import digamma

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the references need x87 extended precision (x86)"

U = LD(2.0) ** -53
CLAMP = LD("1e-30")
CLAMP_LO, CLAMP_HI = LD("1e-31"), LD("1e-29")


def stored_genotypes(y, held=None, shard=None):
    """y [l][count] of a shard with the held-out entries (global ids; those outside the shard ignored) as 3"""
    l, n = y.shape
    b, c = (0, n) if shard is None else shard
    ys = np.array(y[:, b:b + c], dtype=np.uint8)
    for loc, ids in (held or {}).items():
        ids = np.asarray(ids, dtype=np.int64)
        ids = ids[(ids >= b) & (ids < b + c)]
        ys[int(loc), ids - b] = 3
    return ys


def bed_bytes(ys):
    """PLINK bytes [l][ceil(count / 4)] of stored genotypes, the padding entries of the last byte as 01 (missing)"""
    l, n = ys.shape
    nb = (n + 3) // 4
    code = np.array([0b00, 0b10, 0b11, 0b01], dtype=np.uint8)
    c = np.full((l, nb * 4), 0b01, dtype=np.uint8)
    c[:, :n] = code[ys]
    c = c.reshape(l, nb, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def theta_ref(gamma):
    g = np.asarray(gamma, dtype=LD)
    return g / g.sum(axis=1, keepdims=True)


def ebeta_ref(lam):
    lam = np.asarray(lam, dtype=LD)
    return lam[:, :, 0] / (lam[:, :, 0] + lam[:, :, 1])


class Entries:
    """the listed entries of a shard: q, 1 - q, y [J][count] (long double), ok [J][count] and the first-order errors"""

    def __init__(self, y, gamma, lam, held=None, locs=None, shard=None):
        l, n = y.shape
        b, c = (0, n) if shard is None else shard
        self.k = k = np.asarray(gamma).shape[1]
        self.locs = np.arange(l)
        self.ys = ys = stored_genotypes(y, held, shard)
        theta = theta_ref(np.asarray(gamma)[b:b + c])
        q = ebeta_ref(lam) @ theta.T                                    # [l][count]
        self.ok = ys != 3
        self.y = np.where(self.ok, ys, 0).astype(LD)
        self.q, self.omq = q, LD(1.0) - q
        assert np.all((q > 0) & (self.omq > 0))
        self.c_q = (2 * k + 4) * U
        self.d1 = q * self.c_q / self.omq + U
        self.r = self.y - 2 * q
        self.dr = 2 * q * self.c_q + U * np.abs(self.r)
        self.h = 2 * q * self.omq
        self.dh = self.h * (self.c_q + self.d1)
        # the exact product of the log-likelihood term and its relative error
        self.p = np.where(ys == 0, self.omq * self.omq, np.where(ys == 1, self.h, q * q))
        self.dp = np.where(ys == 0, 2 * self.d1, np.where(ys == 1, self.c_q + self.d1, 2 * self.c_q))
        near = self.ok & (self.p >= CLAMP_LO) & (self.p <= CLAMP_HI)
        assert not near.any(), "an entry's product lies within a factor 10 of the 1e-30 clamp: choose another seed"
        if locs is not None:
            self.__dict__.update(self.take(locs).__dict__)

    def take(self, locs):
        """the entries of a list of locations (any order, repeats allowed) out of those of every location"""
        if locs is None:
            return self
        assert len(self.locs) == self.ys.shape[0] and np.array_equal(self.locs, np.arange(len(self.locs)))
        rows = np.asarray(locs, dtype=np.int64)
        e = Entries.__new__(Entries)
        for key, v in self.__dict__.items():
            setattr(e, key, v[rows] if isinstance(v, np.ndarray) and v.ndim == 2 else v)
        e.locs = rows
        return e


def _entries(y, gamma, lam, held, locs, shard, entries):
    """entries: an Entries of EVERY location of the same planted inputs and shard, computed once and shared"""
    return Entries(y, gamma, lam, held, locs, shard) if entries is None else entries.take(locs)


def _sum_bound(err, mag, mask, axis):
    """4 (sum of the entries' errors + M u sum |term|) over the entries of mask"""
    m = mask.sum(axis=axis).astype(LD)
    return 4 * (np.where(mask, err, 0).sum(axis=axis) + m * U * np.where(mask, np.abs(mag), 0).sum(axis=axis))


def _term_err(first_order, term):
    return first_order + 4 * U * (1 + np.abs(term))


def loglik_ref(y, gamma, lam, held=None, locs=None, shard=None, entries=None):
    """(ref, bound): loc_sums / loc_counts [J], indiv_sums / indiv_counts [count], sum, count; bound has the three sums"""
    e = _entries(y, gamma, lam, held, locs, shard, entries)
    clamped = e.p < CLAMP
    t = np.where(e.ok, np.log(np.where(clamped, CLAMP, e.p)), 0)
    err = _term_err(np.where(clamped, 0, e.dp), t)
    ref = dict(loc_sums=t.sum(axis=1), loc_counts=e.ok.sum(axis=1).astype(np.uint64), indiv_sums=t.sum(axis=0),
               indiv_counts=e.ok.sum(axis=0).astype(np.uint64))
    ref["sum"], ref["count"] = ref["loc_sums"].sum(), int(ref["loc_counts"].sum())
    bound = dict(loc_sums=_sum_bound(err, t, e.ok, 1), indiv_sums=_sum_bound(err, t, e.ok, 0))
    bound["sum"] = bound["loc_sums"].sum() + 4 * len(e.locs) * U * np.abs(ref["loc_sums"]).sum()
    return ref, bound


def scan_ref(y, gamma, lam, held=None, locs=None, shard=None, trait=None, entries=None):
    """(ref, bound): fit_sums [J][4], fit_counts [J][3] and, with a trait [count] (NaN = not phenotyped), trait_sums [J][6]
    and trait_counts [J]; bound has fit_sums and trait_sums"""
    e = _entries(y, gamma, lam, held, locs, shard, entries)
    q, omq, h = e.q, e.omq, e.h
    terms = [omq * omq, h, q * q, h * (1 - h)]
    first = [2 * e.d1 * omq * omq, e.dh, 2 * e.c_q * q * q, np.abs(1 - 2 * h) * e.dh]
    ref = dict(fit_sums=np.stack([np.where(e.ok, t, 0).sum(axis=1) for t in terms], axis=1),
               fit_counts=np.stack([(e.ys == v).sum(axis=1) for v in (0, 1, 2)], axis=1).astype(np.uint32))
    bound = dict(fit_sums=np.stack([_sum_bound(_term_err(f, t), t, e.ok, 1) for f, t in zip(first, terms)], axis=1))
    if trait is not None:
        trait = np.asarray(trait, dtype=np.float64)
        has = ~np.isnan(trait)
        tv = np.where(has, trait, 0.0).astype(LD)[None, :]
        m = e.ok & has[None, :]
        zero = np.zeros_like(q)
        terms = [tv + zero, tv * e.r, tv * tv * h, tv * h, e.r, h]
        first = [zero, np.abs(tv) * e.dr, tv * tv * e.dh, np.abs(tv) * e.dh, e.dr, e.dh]
        ref.update(trait_sums=np.stack([np.where(m, t, 0).sum(axis=1) for t in terms], axis=1), trait_counts=m.sum(axis=1).astype(np.uint32))
        bound.update(trait_sums=np.stack([_sum_bound(_term_err(f, t), t, m, 1) for f, t in zip(first, terms)], axis=1))
    return ref, bound


def kin_ref(y, gamma, lam, ids, held=None, locs=None, shard=None, entries=None):
    """(ref, bound): num, den, kin [m][m] of the listed GLOBAL ids (all inside the shard); kin is 0 where den is"""
    l, n = y.shape
    b, c = (0, n) if shard is None else shard
    rows = np.asarray(ids, dtype=np.int64) - b
    assert np.all((rows >= 0) & (rows < c))
    e = _entries(y, gamma, lam, held, locs, shard, entries)
    ok = e.ok[:, rows]
    r, dr = np.where(ok, e.r[:, rows], 0).T, np.where(ok, e.dr[:, rows], 0).T         # [m][J]
    s = np.sqrt(e.q * e.omq)
    ds = s * ((e.c_q + e.d1) / 2 + 2 * U)
    s, ds = np.where(ok, s[:, rows], 0).T, np.where(ok, ds[:, rows], 0).T
    acc = (len(e.locs) + 2) * U
    num, den = r @ r.T, s @ s.T
    bnum = np.abs(r) @ dr.T + dr @ np.abs(r).T + acc * (np.abs(r) @ np.abs(r).T)
    bden = s @ ds.T + ds @ s.T + acc * den
    pos = den > 0
    safe = np.where(pos, den, 1)
    kin = np.where(pos, num / (4 * safe), 0)
    bkin = np.where(pos, bnum / (4 * safe) + np.abs(num) * bden / (4 * safe * safe) + 2 * U * np.abs(kin), 0)
    return dict(num=num, den=den, kin=kin), dict(num=bnum, den=bden, kin=bkin)


def _band(full, window):
    """[J][window + 1] of a [J][J] matrix: column d of row i is entry (i, i + d), 0 where i + d >= J"""
    J = full.shape[0]
    i = np.arange(J)[:, None]
    j = i + np.arange(window + 1)[None, :]
    return np.where(j < J, full[i, np.minimum(j, J - 1)], 0)


def _band_of_products(a, b, window):
    """[J][window + 1]: sum_n a(i, n) b(i + d, n) of a, b [J][M]; from the full product a b^T where the band covers most of it"""
    J = a.shape[0]
    reach = min(window, J - 1)
    if 2 * (reach + 1) > J:
        return _band(a @ b.T, window)
    out = np.zeros((J, window + 1), dtype=np.result_type(a, b))
    for d in range(reach + 1):
        out[:J - d, d] = (a[:J - d] * b[d:]).sum(axis=1)
    return out


def ld_ref(y, gamma, lam, window, held=None, locs=None, shard=None, entries=None):
    """(ref, bound): num, cnt (uint32), absn, bands [J][window + 1] whose column d of row i is the pair of list positions
    (i, i + d), 0 where i + d >= J; bound has num"""
    e = _entries(y, gamma, lam, held, locs, shard, entries)
    ok = e.ok & (e.h > 0)
    root = np.sqrt(np.where(ok, e.h, 1))
    z = np.where(ok, e.r / root, 0)                                                   # [J][count]
    dz = np.where(ok, e.dr / root + np.abs(z) * ((e.c_q + e.d1) / 2 + 3 * U), 0)
    az = np.abs(z)
    m = ok.astype(np.float64)                                                         # (0 / 1: the fp64 product is exact)
    num, absn = _band_of_products(z, z, window), _band_of_products(az, az, window)
    cnt = _band(m @ m.T, window).astype(np.uint32)
    bnum = _band_of_products(az, dz, window) + _band_of_products(dz, az, window) + (z.shape[1] + 2) * U * absn
    return dict(num=num, cnt=cnt, absn=absn), dict(num=bnum)


def foldin_ref(y, gamma, lam, alpha, snapshots, held=None, locs=None, shard=None):
    """{i: dict(gamma [count][k], iters [count], change [count])} after i = each of `snapshots` updates at tol = 0, from
        w_k = exp(psi(gamma_k) - psi(sum_k gamma_k)),  eb = exp(psi(lambda) - psi(lambda0 + lambda1))
        gamma'_k = alpha + w_k sum_{j listed, stored} (y eb[j][k][0] / S0_j + (2 - y) eb[j][k][1] / S1_j),  S = sum_k w_k eb[j][k]
        change = mean_k |gamma' - gamma| / mean_k gamma'"""
    l, n = y.shape
    b, c = (0, n) if shard is None else shard
    locs = np.arange(l) if locs is None else np.asarray(locs, dtype=np.int64)
    ys = stored_genotypes(y, held, shard)[locs].T                                     # [count][J]
    ok = ys != 3
    mom = np.where(ok, ys, 0).astype(LD)
    dad = np.where(ok, 2 - ys.astype(np.int64), 0).astype(LD)
    lam = np.asarray(lam, dtype=np.float64)[locs]
    eb = np.exp(digamma(lam).astype(LD) - digamma(lam.sum(axis=2)).astype(LD)[:, :, None])
    e0, e1 = eb[:, :, 0], eb[:, :, 1]                                                 # [J][k]
    g = np.asarray(gamma, dtype=np.float64)[b:b + c].astype(LD)
    alpha = LD(alpha)
    out = {}
    for it in range(1, max(snapshots) + 1):
        g64 = g.astype(np.float64)
        w = np.exp(digamma(g64).astype(LD) - digamma(g64.sum(axis=1)).astype(LD)[:, None])
        c0, c1 = mom / (w @ e0.T), dad / (w @ e1.T)
        gn = alpha + w * (c0 @ e0 + c1 @ e1)
        change = np.abs(gn - g).sum(axis=1) / gn.sum(axis=1)
        # gamma and gamma' each within relative FOLDIN_TOL: the numerator moves by at most that of sum (gamma' + gamma)
        change_bound = FOLDIN_TOL * ((gn + g).sum(axis=1) / gn.sum(axis=1) + change)
        g = gn
        if it in snapshots:
            out[it] = dict(gamma=g.copy(), iters=np.full(c, it, dtype=np.uint32), change=change, change_bound=change_bound)
    return out


# -- comparisons: a result (a kernel's, or a plain fp64 evaluation's) against a reference and its bound ---------------------------

def ratio(got, ref, bound):
    """max |got - ref| / bound (0 where both differences and bounds vanish, inf where only the bound does)"""
    d = np.abs(np.asarray(got).astype(LD) - ref)
    b = np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0, d / b)
    return float(np.max(r))


def compare_loglik(got, ref, bound, limit=1.0):
    for key in ("loc_counts", "indiv_counts"):
        assert np.array_equal(np.asarray(got[key]).astype(np.uint64), ref[key]), key
    assert int(got["count"]) == ref["count"]
    worst = max(ratio(got[key], ref[key], bound[key]) for key in ("loc_sums", "indiv_sums", "sum"))
    assert worst <= limit, ("train_loglik", worst)
    return worst


def compare_scan(got, ref, bound, limit=1.0):
    assert set(got) == set(ref)
    worst = 0.0
    for key in ref:
        if key.endswith("counts"):
            assert np.array_equal(got[key], ref[key]), key
        else:
            worst = max(worst, ratio(got[key], ref[key], bound[key]))
    assert worst <= limit, ("snp_scan", worst)
    return worst


def compare_kin(got, ref, bound, limit=1.0):
    """got = (kin, num, den)"""
    kin, num, den = got
    assert np.all(np.asarray(kin)[ref["den"] == 0] == 0.0)
    worst = max(ratio(num, ref["num"], bound["num"]), ratio(den, ref["den"], bound["den"]), ratio(kin, ref["kin"], bound["kin"]))
    assert worst <= limit, ("kinship", worst)
    return worst


def compare_ld(got, ref, bound, limit=1.0):
    """got = dict(num, cnt): cnt byte for byte, the entries past the list's end exactly 0, every value finite"""
    num, cnt = np.asarray(got["num"]), np.asarray(got["cnt"])
    assert num.shape == ref["num"].shape and cnt.shape == ref["cnt"].shape and cnt.dtype == np.uint32
    assert np.all(np.isfinite(num))
    assert cnt.tobytes() == ref["cnt"].tobytes(), "cnt"
    J, w1 = num.shape
    past = np.add.outer(np.arange(J), np.arange(w1)) >= J
    for a in (num, cnt, ref["num"], ref["cnt"]):
        assert np.all(a[past] == 0), "an entry past the list's end"
    worst = ratio(num, ref["num"], bound["num"])
    assert worst <= limit, ("ld", worst)
    return worst


FOLDIN_TOL = 1e-9        # gamma, relative: the project's parity tolerance
FOLDIN_SUM_TOL = 1e-11   # sum_k gamma = K alpha + 2 M, relative


def compare_foldin(gamma, out, ref, limit=1.0):
    """gamma [count][k] and dict(iters, change) after as many updates as ref (one snapshot of foldin_ref) holds; returns
    max relative |gamma - ref| / 1e-9"""
    assert np.array_equal(out["iters"], ref["iters"])
    worst = float(np.max(np.abs(np.asarray(gamma).astype(LD) - ref["gamma"]) / ref["gamma"])) / FOLDIN_TOL
    assert worst <= limit, ("fold_in", worst)
    ch = ratio(out["change"], ref["change"], ref["change_bound"])
    assert ch <= limit, ("fold_in change", ch)
    return worst


def foldin_sum_error(gamma, k, alpha, indiv_counts):
    """max relative |sum_k gamma - (K alpha + 2 M)|, M the individual's listed stored entries"""
    want = k * LD(alpha) + 2 * np.asarray(indiv_counts).astype(LD)
    return float(np.max(np.abs(np.asarray(gamma).astype(LD).sum(axis=1) - want) / want))


# -- the planted cases the CPU and GPU tests share ------------------------------------------------------------------------------

class Case:
    """n, l, k, y [l][n], gamma [n][k], lam [l][k][2], held {loc: global ids}, alpha, trait [n], locs, ids"""


EVERY_K = list(range(1, 33)) + [33, 64, 128]
EVERY_K_L = 150   # in one segment five LDS batches of 32 (the last of 22), ten of 16 on the wide fold-in path; three fold-in segments
KIN_M = 130       # three tiles of 64 listed individuals, the last one ragged


def every_k_n(k):
    """the largest tile of the four families (256 x 16 / 8 / 4 / 2 individuals) and a second, ragged one"""
    return 4611 if k <= 4 else 2563 if k <= 8 else 1539 if k <= 16 else 1027


def make_trait(n, seed, nan_rate=0.05):
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 1.0, size=n)
    t[rng.random(n) < nan_rate] = np.nan
    return t


def pick_lists(c, seed, begin=0, count=None):
    """locs: unsorted, with a repeat, ends included; ids: KIN_M global ids of [begin, begin + count), unsorted, both ends
    included, the last one a repeat of the first"""
    rng = np.random.default_rng(seed)
    count = c.n - begin if count is None else count
    locs = rng.permutation(np.arange(1, c.l - 1))[:c.l // 2]
    c.locs = np.concatenate([locs, [c.l - 1], locs[1:2], [0]]).astype(np.uint32)
    inner = begin + 1 + rng.choice(count - 2, size=KIN_M - 3, replace=False)
    ids = np.concatenate([inner[:1], [begin + count - 1], inner[1:], [begin]])
    c.ids = np.concatenate([ids, ids[:1]]).astype(np.uint32)
    assert c.ids.size == KIN_M


def plant_every_k(k, n=None, l=EVERY_K_L):
    """(n, l: every_k_n(k) and EVERY_K_L unless given)  PSD genotypes with 10 % missing, the initial gamma, a "trained" lambda = 1 + c (beta, 1 - beta) with a per-location
    c in (0, 200), and held-out lists at locations 0, l / 2 and l - 1 that include individuals 0 and n - 1"""
    from helpers import init_gamma, psd_genotypes

    c = Case()
    n = every_k_n(k) if n is None else n
    c.n, c.l, c.k = n, l, k
    c.y, _, beta = psd_genotypes(n, l, k, 7000 + k, missing_rate=0.1)
    rng = np.random.default_rng(7200 + k)
    scale = rng.uniform(0.0, 200.0, size=(l, 1))
    c.lam = np.stack([1.0 + scale * beta, 1.0 + scale * (1.0 - beta)], axis=2)
    c.gamma = init_gamma(n, k, 7400 + k)
    c.held = {0: np.array([0, 5, 64, n - 1], dtype=np.uint32), l // 2: np.arange(3, n, 7, dtype=np.uint32),
              l - 1: np.array([0, 1, n - 2, n - 1], dtype=np.uint32)}
    c.alpha = 1.0 / k
    c.trait = make_trait(n, 7600 + k)
    pick_lists(c, 7800 + k)
    return c


LATE_SHAPES = [(1030, 40, 8, 1, 0), (2050, 40, 20, 1, 0), (4200, 36, 3, 1, 0), (700, 40, 33, 1, 0), (1030, 40, 8, 3, 1)]  # n, l, k, world, rank


def shard_of(n, rank, world):
    """tsamd_shard_range: contiguous shards of ceil(n / world) rounded up to a multiple of 4"""
    per = (-(-n // world) + 3) // 4 * 4
    begin = min(n, rank * per)
    return begin, min(n, begin + per) - begin


def plant_late(n, l, k, world=1, rank=0, seed=5):
    """late_state.plant with lambda scaled to an effective sample of 1e6: Ebeta within 1e-6 of 0 and 1, gamma from the 1e-8
    floor to 1e6; returns (Case, the Late state that late_state.load_engine takes)"""
    import late_state

    s = late_state.plant(n, l, k, seed, n_eff=1e6)
    c = Case()
    c.n, c.l, c.k, c.y, c.gamma, c.lam, c.held, c.alpha = n, l, k, s.y, s.gamma, s.lam, s.held, 1.0 / k
    c.shard = shard_of(n, rank, world)
    c.trait = make_trait(n, 100 + seed)
    pick_lists(c, 200 + seed, *c.shard)
    c.floor_rows = s.floor_rows
    return c, s
