"""Extended-precision references, with derived error bounds, of tsamd_theta_info and tsamd_theta_se, in the style of
analysis_refs.py and built on its Entries: PLANTED inputs only, numpy long double, bounds derived to first order with
u = 2^-53 and never measured.

tsamd_theta_info.  H[n][p] = sum_j c(n, j) Ebeta[j][a] Ebeta[j][b], p = (a <= b) packed, every term non-negative, so the bounds
are relative to the sum itself.  With c_q and d1 as analysis_refs defines them (relative errors of q and of 1 - q):
  * y / q^2 carries 2 c_q + 3 u (q twice; a square, a quotient and the term's addition round once each);
  * (2 - y) / (1 - q)^2 carries 2 d1 + 3 u;
  * 2 / (q (1 - q)) carries c_q + d1 + 3 u;
  * Ebeta_a Ebeta_b carries 5 u (two Ebeta of 2 u each and the product);
  * a sum of M terms gets the project's 4 (sum of the terms' errors + M u sum of terms).

tsamd_theta_se.  The reference is pinv(P H P), P = I - 1 1^T / K, in long double: (P H P + s J)^-1 - J / s with J = 1 1^T / K (the
two act on orthogonal subspaces; s = trace(P H P) / K keeps the sum as well conditioned as P H P is on its own subspace), by
Gauss-Jordan elimination -- another route than the library's Cholesky of Z^T H Z.  The bound on
cov_ab is 8 K^2 u cond_2(M) sqrt(cov_aa cov_bb), M = Z^T H Z: the classical relative error of a Cholesky solve, c K^2 u cond_2
with c = 8 for forming M (4 terms per entry), the factor, the two triangular solves and Z M^-1 Z^T's sums, measured against
the entry's scale sqrt(cov_aa cov_bb) >= |cov_ab|; on the diagonal that is 8 K^2 u cond_2(M) |cov_kk|, and se = sqrt(cov_kk)
gets half of it relatively.

The calibration fixture (calibration_case, numpy_fold_in) is the claim the standard errors make, on numpy alone.
"""
import numpy as np
from scipy.special import digamma

import analysis_refs as ar
from analysis_refs import LD, U


def packed(k):
    return k * (k + 1) // 2


def info_ref(y, gamma, lam, ids, held=None, locs=None, shard=None, entries=None):
    """(ref, bound): dict(obs, exp), each [m][P], of the listed GLOBAL ids (all inside the shard) over locs"""
    l, n = y.shape
    b, c = (0, n) if shard is None else shard
    rows = np.asarray(ids, dtype=np.int64) - b
    assert np.all((rows >= 0) & (rows < c))
    e = ar._entries(y, gamma, lam, held, locs, shard, entries)
    k = e.k
    ok = e.ok[:, rows]
    q, omq, yv, d1 = e.q[:, rows], e.omq[:, rows], e.y[:, rows], e.d1[:, rows]
    t0, t1 = yv / (q * q), (2 - yv) / (omq * omq)
    cobs = np.where(ok, t0 + t1, 0)
    dcobs = np.where(ok, t0 * (2 * e.c_q + 3 * U) + t1 * (2 * d1 + 3 * U), 0)
    cexp = np.where(ok, 2 / (q * omq), 0)
    dcexp = cexp * (e.c_q + d1 + 3 * U)
    eb = ar.ebeta_ref(lam)[np.asarray(e.locs, dtype=np.int64)]                      # [J][k]
    a, bb_ = np.triu_indices(k)
    bb = eb[:, a] * eb[:, bb_]                                                      # [J][P]
    m_terms = ok.sum(axis=0).astype(LD)[:, None]                                   # [m][1]
    ref, bound = {}, {}
    for key, cc, dc in (("obs", cobs, dcobs), ("exp", cexp, dcexp)):
        h = cc.T @ bb                                                               # [m][P]
        ref[key] = h
        bound[key] = 4 * (dc.T @ bb + 5 * U * h + m_terms * U * h)
    return ref, bound


def info_numpy(y, gamma, lam, ids, held=None, locs=None, shard=None):
    """the device terms restated in plain fp64 numpy: dict(obs, exp)"""
    l, n = y.shape
    b, c = (0, n) if shard is None else shard
    rows = np.asarray(ids, dtype=np.int64) - b
    locs = np.arange(l) if locs is None else np.asarray(locs, dtype=np.int64)
    ys = ar.stored_genotypes(y, held, shard)[locs][:, rows].T                       # [m][J]
    g = np.asarray(gamma, dtype=np.float64)[b:b + c][rows]
    lam = np.asarray(lam, dtype=np.float64)[locs]
    return info_fp64(g / g.sum(axis=1, keepdims=True), lam[:, :, 0] / (lam[:, :, 0] + lam[:, :, 1]), ys)


def info_fp64(theta, eb, ys):
    """dict(obs, exp) [m][P] from theta [m][k], Ebeta [J][k] and genotypes ys [m][J] in {0, 1, 2, 3 = no term}, in fp64 as
    info_terms (csrc/tsamd_info_plan.h) forms them"""
    k = theta.shape[1]
    q = theta @ eb.T
    p = 1.0 - q
    ok = ys != 3
    yv = np.where(ok, ys, 0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        co = np.where(yv > 0, yv / (q * q), 0.0) + np.where(yv < 2, (2.0 - yv) / (p * p), 0.0)
        ce = 2.0 / (q * p)
    ok = ok & (q > 0) & (p > 0) & np.isfinite(co) & np.isfinite(ce)
    a, b = np.triu_indices(k)
    bb = eb[:, a] * eb[:, b]
    return dict(obs=np.where(ok, co, 0.0) @ bb, exp=np.where(ok, ce, 0.0) @ bb)


def unpack(pk, k, dtype=LD):
    pk = np.asarray(pk, dtype=dtype)
    a, b = np.triu_indices(k)
    out = np.zeros((pk.shape[0], k, k), dtype=dtype)
    out[:, a, b] = pk
    out[:, b, a] = pk
    return out


def _inverse_ld(a):
    """batched inverse [m][r][r] of symmetric positive definite matrices by Gauss-Jordan elimination in long double"""
    m, r, _ = a.shape
    w = np.concatenate([a.astype(LD), np.broadcast_to(np.eye(r, dtype=LD), (m, r, r))], axis=2)
    for j in range(r):
        w[:, j, :] = w[:, j, :] / w[:, j, j][:, None]
        f = w[:, :, j].copy()
        f[:, j] = 0
        w -= f[:, :, None] * w[:, j, :][:, None, :]
    return w[:, :, r:]


def se_ref(info, k):
    """(ref, bound): dict(se [m][k], cov [m][P]) = pinv(P H P) in long double of packed fp64 information matrices that are
    identified; bound likewise"""
    h = unpack(info, k)
    m = h.shape[0]
    a, b = np.triu_indices(k)
    if k == 1:
        z = np.zeros((m, 1), dtype=LD)
        return dict(se=z, cov=z.copy()), dict(se=z.copy(), cov=z.copy())
    j = np.full((k, k), LD(1) / k, dtype=LD)
    p = np.eye(k, dtype=LD) - j
    php = p[None] @ h @ p[None]
    s = (np.trace(php, axis1=1, axis2=2) / k)[:, None, None]  # J scaled to P H P's own size: the sum is as well conditioned as M
    cov = _inverse_ld(php + s * j[None]) - j[None] / s
    mm = h[:, :k - 1, :k - 1] - h[:, :k - 1, k - 1:] - h[:, k - 1:, :k - 1] + h[:, k - 1:, k - 1:]
    cond = np.array([np.linalg.cond(x) for x in mm.astype(np.float64)]).astype(LD)
    rel = 8 * k * k * U * cond                                                      # [m]
    d = np.diagonal(cov, axis1=1, axis2=2)
    scale = np.sqrt(d[:, a] * d[:, b])
    ref = dict(se=np.sqrt(d), cov=cov[:, a, b])
    bound = dict(se=np.sqrt(d) * rel[:, None] / 2, cov=scale * rel[:, None])
    return ref, bound


def se_numpy(info, k):
    """the library's algorithm restated in plain fp64 numpy: M = Z^T H Z, Cholesky without pivoting, cov = Z M^-1 Z^T;
    dict(se, cov, status)"""
    h = unpack(info, k, np.float64)
    m = h.shape[0]
    a, b = np.triu_indices(k)
    se, cov, status = np.zeros((m, k)), np.zeros((m, packed(k))), np.zeros(m, dtype=np.uint8)
    if k == 1:
        return dict(se=se, cov=cov, status=status)
    r = k - 1
    z = np.concatenate([np.eye(r), -np.ones((1, r))], axis=0)
    mm = h[:, :r, :r] - h[:, :r, r:] - h[:, r:, :r] + h[:, r:, r:]
    low = np.zeros((m, r, r))
    ok = np.ones(m, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(r):  # column by column, no pivoting; a pivot must exceed 1e-12 of its own original diagonal entry
            d = mm[:, j, j] - (low[:, j, :j] ** 2).sum(axis=1)
            ok &= (d > 1e-12 * mm[:, j, j]) & (d > 0) & np.isfinite(d)
            ljj = np.sqrt(np.where(ok, d, 1.0))
            low[:, j, j] = ljj
            low[:, j + 1:, j] = (mm[:, j + 1:, j] - (low[:, j + 1:, :j] * low[:, j:j + 1, :j]).sum(axis=2)) / ljj[:, None]
    low[~ok] = np.eye(r)
    li = np.linalg.solve(low, np.broadcast_to(np.eye(r), (m, r, r)))
    full = z[None] @ (li.transpose(0, 2, 1) @ li) @ z.T[None]
    se, cov = np.sqrt(np.diagonal(full, axis1=1, axis2=2)), full[:, a, b]
    se[~ok], cov[~ok], status[~ok] = np.nan, np.nan, 1
    return dict(se=se, cov=cov, status=status)


def compare_info(got, ref, bound, limit=1.0):
    worst = max(ar.ratio(got[key], ref[key], bound[key]) for key in ("obs", "exp"))
    assert worst <= limit, ("theta_info", worst)
    return worst


def compare_se(got, ref, bound, limit=1.0):
    assert np.all(np.asarray(got["status"]) == 0)
    worst = max(ar.ratio(got[key], ref[key], bound[key]) for key in ("se", "cov"))
    assert worst <= limit, ("theta_se", worst)
    return worst


# -- the calibration claim ------------------------------------------------------------------------------------------------------

CAL_SEEDS = list(range(6, 14))
CAL_N, CAL_L, CAL_K = 256, 4096, 3
CAL_THETA = np.array([0.5, 0.3, 0.2])
CAL_RATIO_BAND = (0.80, 1.25)      # sd over individuals of theta_k / mean se_k
CAL_COVER_BAND = (0.89, 0.995)     # share of |theta_k - planted| < 1.96 se_k, all k together


def calibration_case(seed):
    """dict(y [l][n] in {0, 1, 2, 3 = missing}, theta [n][k], beta [l][k], lam [l][k][2]): n replicates of one interior theta,
    beta uniform in [0.05, 0.95], lambda = 1e6 (beta, 1 - beta) so that exp(Elogbeta) and Ebeta agree with beta to about 1e-6,
    10 % missing"""
    rng = np.random.default_rng(seed)
    theta = np.tile(CAL_THETA, (CAL_N, 1))
    beta = rng.uniform(0.05, 0.95, size=(CAL_L, CAL_K))
    p = beta @ theta.T
    y = (rng.random((CAL_L, CAL_N)) < p).astype(np.uint8) + (rng.random((CAL_L, CAL_N)) < p).astype(np.uint8)
    y[rng.random(y.shape) < 0.1] = 3
    lam = 1e6 * np.stack([beta, 1.0 - beta], axis=2)
    return dict(y=y, theta=theta, beta=beta, lam=lam)


def numpy_fold_in(y, lam, k, iters=200):
    """gamma [n][k] after `iters` fold-in updates from gamma = 1 (analysis_refs.foldin_ref's update in fp64), alpha = 1 / k"""
    ys = y.T
    ok = ys != 3
    mom = np.where(ok, ys, 0).astype(np.float64)
    dad = np.where(ok, 2.0 - ys.astype(np.float64), 0.0)
    eb = np.exp(digamma(lam) - digamma(lam.sum(axis=2))[:, :, None])
    e0, e1 = eb[:, :, 0], eb[:, :, 1]
    g = np.ones((ys.shape[0], k))
    for _ in range(iters):
        w = np.exp(digamma(g) - digamma(g.sum(axis=1))[:, None])
        g = 1.0 / k + w * ((mom / (w @ e0.T)) @ e0 + (dad / (w @ e1.T)) @ e1)
    return g


def calibration_figures(theta_hat, se, planted=CAL_THETA):
    """(ratios [k], coverage): sd over individuals of theta_k / mean se_k, and the share of |theta_k - planted| < 1.96 se_k"""
    ratios = theta_hat.std(axis=0, ddof=1) / se.mean(axis=0)
    cover = float(np.mean(np.abs(theta_hat - planted[None, :]) < 1.96 * se))
    return ratios, cover


def assert_calibrated(theta_hat, se, what=""):
    ratios, cover = calibration_figures(theta_hat, se)
    print(f"{what}sd / mean se = {np.array2string(ratios, precision=3)}, coverage = {cover:.4f}")
    assert np.all((ratios >= CAL_RATIO_BAND[0]) & (ratios <= CAL_RATIO_BAND[1])), ratios
    assert CAL_COVER_BAND[0] <= cover <= CAL_COVER_BAND[1], cover
    return ratios, cover
