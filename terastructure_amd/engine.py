"""Engine: one tsamd_ctx (one GPU, one shard of individuals).

Method names follow include/tsamd.h; array shapes follow the reference
(gamma/theta [n][k], lambda [l][k][2], Ebeta [l][k]), all float64 row-major.
"""
import ctypes as C

import numpy as np

from . import _lib


def shard_range(n, rank, world):
    """(begin, count) of rank's individuals -- tsamd_shard_range."""
    h = _lib.load()
    b, c = C.c_uint32(0), C.c_uint32(0)
    h.tsamd_shard_range(n, rank, world, C.byref(b), C.byref(c))
    return b.value, c.value


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def host_alloc(nbytes):
    """numpy uint8 view of pinned host memory (tsamd_host_alloc); free it with host_free(arr)"""
    h = _lib.load()
    ptr = C.c_void_p()
    rc = h.tsamd_host_alloc(C.byref(ptr), nbytes)
    if rc != 0:
        raise _lib.TsamdError(rc, h.tsamd_last_error(None).decode())
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
    return arr


def host_free(arr):
    _lib.load().tsamd_host_free(C.c_void_p(arr.ctypes.data))


def scan_statistics(fit_sums, fit_counts, trait_sums=None, trait_counts=None):
    """[n_locs][6] = z_het, p_het, z_freq, p_freq, z_trait, p_trait from the sufficient statistics of Engine.snp_scan (added
    across shards by the caller) -- tsamd_scan_statistics.  No device work: runs without a GPU."""
    h = _lib.load()
    fs = np.ascontiguousarray(fit_sums, dtype=np.float64).reshape(-1, _lib.SCAN_FIT_SUMS)
    fc = np.ascontiguousarray(fit_counts, dtype=np.uint32).reshape(-1, _lib.SCAN_FIT_COUNTS)
    n_locs = fs.shape[0]
    if fc.shape[0] != n_locs:
        raise ValueError("fit_sums and fit_counts differ in length")
    ts = tc = None
    if trait_sums is not None and trait_counts is not None:
        ts = np.ascontiguousarray(trait_sums, dtype=np.float64).reshape(-1, _lib.SCAN_TRAIT_SUMS)
        tc = np.ascontiguousarray(trait_counts, dtype=np.uint32).reshape(-1)
        if ts.shape[0] != n_locs or tc.shape[0] != n_locs:
            raise ValueError("trait_sums / trait_counts differ in length from fit_sums")
    out = np.zeros((n_locs, _lib.SCAN_STATS), dtype=np.float64)
    rc = h.tsamd_scan_statistics(_dp(fs), _up(fc), None if ts is None else _dp(ts), None if tc is None else _up(tc), n_locs, _dp(out))
    if rc != 0:
        raise _lib.TsamdError(rc, h.tsamd_last_error(None).decode())
    return out


def ld_statistics(num, cnt):
    """(r, p), both [n_locs][window + 1], from the bands of Engine.ld (added across shards by the caller): r = num / cnt (0 where
    cnt < 2), p = erfc(|r| sqrt(cnt) / sqrt(2)) -- tsamd_ld_statistics.  No device work: runs without a GPU."""
    h = _lib.load()
    nu = np.ascontiguousarray(num, dtype=np.float64)
    cn = np.ascontiguousarray(cnt, dtype=np.uint32)
    if nu.ndim != 2 or nu.shape != cn.shape or nu.shape[1] < 1:
        raise ValueError("num and cnt must be bands of one shape [n_locs][window + 1]")
    r, p = np.zeros(nu.shape, dtype=np.float64), np.zeros(nu.shape, dtype=np.float64)
    rc = h.tsamd_ld_statistics(_dp(nu), _up(cn), nu.shape[0], nu.shape[1] - 1, _dp(r), _dp(p))
    if rc != 0:
        raise _lib.TsamdError(rc, h.tsamd_last_error(None).decode())
    return r, p


def ld_prune(r, r2_max):
    """bool [n_locs]: the positions an LD pruning of the band r [n_locs][window + 1] keeps -- in ascending order, a position is
    dropped if and only if a KEPT position at most window before it has r^2 > r2_max with it -- tsamd_ld_prune.  No device work."""
    h = _lib.load()
    ra = np.ascontiguousarray(r, dtype=np.float64)
    if ra.ndim != 2 or ra.shape[1] < 1:
        raise ValueError("r must be a band [n_locs][window + 1]")
    keep = np.zeros(ra.shape[0], dtype=np.uint8)
    rc = h.tsamd_ld_prune(_dp(ra), ra.shape[0], ra.shape[1] - 1, float(r2_max), keep.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise _lib.TsamdError(rc, h.tsamd_last_error(None).decode())
    return keep.astype(bool)


def info_packed(k):
    """P = k (k + 1) / 2: the packed length of a symmetric k x k matrix -- TSAMD_INFO_PACKED"""
    return k * (k + 1) // 2


def info_unpack(packed, k):
    """[m][k][k], symmetric, from packed rows [m][P] of Engine.theta_info or theta_se's cov: entry (a <= b) of a row is at
    a k - a (a - 1) / 2 + (b - a)."""
    pa = np.asarray(packed, dtype=np.float64)
    if pa.ndim != 2 or pa.shape[1] != info_packed(k):
        raise ValueError(f"packed must be [m][{info_packed(k)}]")
    a, b = np.triu_indices(k)  # (row by row: the packed order)
    out = np.zeros((pa.shape[0], k, k), dtype=np.float64)
    out[:, a, b] = pa
    out[:, b, a] = pa
    return out


def theta_se(info, k):
    """dict(se [m][k], cov [m][P] packed, status [m]) from information matrices [m][P] of Engine.theta_info (either kind; rows
    over disjoint location lists added by the caller) -- tsamd_theta_se: the asymptotic plug-in standard errors of theta on
    the simplex with lambda taken as known.  status 1 marks a row that is not identified: its se and cov are NaN.  No device
    work: runs without a GPU."""
    h = _lib.load()
    k = int(k)
    ia = np.ascontiguousarray(info, dtype=np.float64)
    if ia.ndim != 2 or not 1 <= k <= 128 or ia.shape[1] != info_packed(k):
        raise ValueError("info must be [m][k (k + 1) / 2] with 1 <= k <= 128")
    m = ia.shape[0]
    se = np.zeros((m, k), dtype=np.float64)
    cov = np.zeros(ia.shape, dtype=np.float64)
    status = np.zeros(m, dtype=np.uint8)
    rc = h.tsamd_theta_se(_dp(ia), m, k, _dp(se), _dp(cov), status.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise _lib.TsamdError(rc, h.tsamd_last_error(None).decode())
    return dict(se=se, cov=cov, status=status)


class Engine:
    def __init__(self, n, l, k, device=0, rank=0, world=1, flags=0, **overrides):
        self.h = _lib.load()
        cfg = _lib.Config()
        self.h.tsamd_default_config(C.byref(cfg), n, l, k)
        cfg.device, cfg.rank, cfg.world, cfg.flags = device, rank, world, flags
        for key, val in overrides.items():
            if not hasattr(cfg, key):
                raise AttributeError(f"tsamd_config has no field {key}")
            setattr(cfg, key, val)
        self.cfg = cfg
        self.n, self.l, self.k = n, l, k
        self.rank, self.world = rank, world
        self.shard_begin, self.shard_count = shard_range(n, rank, world)
        ctx = C.c_void_p()
        rc = self.h.tsamd_create(C.byref(cfg), C.byref(ctx))
        if rc != 0:
            raise _lib.TsamdError(rc, self.h.tsamd_last_error(None).decode())
        self.ctx = ctx

    # -- plumbing -----------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise _lib.TsamdError(rc, self.h.tsamd_last_error(self.ctx).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.h.tsamd_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- genotypes ----------------------------------------------------------
    def upload_bed(self, payload, first_loc=0):
        """payload: uint8 [n_locs][ceil(n/4)] raw PLINK SNP-major bytes (global n)."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be [n_locs][bytes_per_snp]")
        self._check(self.h.tsamd_upload_bed(self.ctx, payload.ctypes.data, payload.shape[1], first_loc,
                                            payload.shape[0]))

    def upload_bed_async(self, ptr, bytes_per_snp, first_loc, n_locs):
        """payload at address ptr in pinned memory (host_alloc); valid until the next synchronize()"""
        self._check(self.h.tsamd_upload_bed_async(self.ctx, ptr, bytes_per_snp, first_loc, n_locs))

    def upload_bed_indiv_major(self, payload, first_indiv=0):
        """payload: uint8 [n_indivs][ceil(l/4)] PLINK individual-major rows (global individuals from first_indiv)"""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be [n_indivs][bytes_per_indiv]")
        self._check(self.h.tsamd_upload_bed_indiv_major(self.ctx, payload.ctypes.data, payload.shape[1], first_indiv,
                                                        payload.shape[0]))

    def genotype_counts(self, first_loc=0, n_locs=None):
        """counts of the PLINK codes (00, 01 = missing, 10, 11) over the shard's individuals"""
        n_locs = self.l - first_loc if n_locs is None else n_locs
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.h.tsamd_genotype_counts(self.ctx, first_loc, n_locs, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def download_bed(self, loc):
        out = np.zeros((self.shard_count + 3) // 4, dtype=np.uint8)
        self._check(self.h.tsamd_download_bed(self.ctx, loc, out.ctypes.data, out.size))
        return out

    def set_heldout(self, loc, indivs):
        a = np.ascontiguousarray(indivs, dtype=np.uint32)
        self._check(self.h.tsamd_set_heldout(self.ctx, loc, _up(a), a.size))

    def synth_genotypes(self, theta, beta, first_loc=0, seed=1, missing_rate=0.0):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        assert theta.shape == (self.shard_count, self.k) and beta.shape[1] == self.k
        self._check(self.h.tsamd_synth_genotypes(self.ctx, _dp(theta), _dp(beta), first_loc, beta.shape[0],
                                                 seed, missing_rate))

    # -- per-individual state -------------------------------------------------
    def set_gamma(self, gamma):
        g = np.ascontiguousarray(gamma, dtype=np.float64)
        if g.shape != (self.shard_count, self.k):
            raise ValueError(f"gamma must be [{self.shard_count}][{self.k}]")
        self._check(self.h.tsamd_set_gamma(self.ctx, _dp(g)))

    def _get_nk(self, fn):
        out = np.empty((self.shard_count, self.k), dtype=np.float64)
        self._check(fn(self.ctx, _dp(out)))
        return out

    def get_gamma(self):
        return self._get_nk(self.h.tsamd_get_gamma)

    def get_theta(self):
        return self._get_nk(self.h.tsamd_get_theta)

    def get_elogtheta(self):
        return self._get_nk(self.h.tsamd_get_elogtheta)

    def set_counts(self, c):
        a = np.ascontiguousarray(c, dtype=np.uint32)
        assert a.shape == (self.shard_count,)
        self._check(self.h.tsamd_set_counts(self.ctx, _up(a)))

    def get_counts(self):
        out = np.empty(self.shard_count, dtype=np.uint32)
        self._check(self.h.tsamd_get_counts(self.ctx, _up(out)))
        return out

    # -- per-location state ---------------------------------------------------
    def set_lambda(self, loc, lam):
        a = np.ascontiguousarray(lam, dtype=np.float64)
        if a.shape != (self.k, 2):
            raise ValueError("lambda must be [k][2]")
        self._check(self.h.tsamd_set_lambda(self.ctx, loc, _dp(a)))

    def set_lambda_range(self, lam, first_loc=0):
        """lambda of locations first_loc .. first_loc + len(lam) - 1 in one call -- tsamd_set_lambda_range; lam is [n_locs][k][2]"""
        a = np.ascontiguousarray(lam, dtype=np.float64)
        if a.ndim != 3 or a.shape[1:] != (self.k, 2):
            raise ValueError("lambda must be [n_locs][k][2]")
        self._check(self.h.tsamd_set_lambda_range(self.ctx, first_loc, a.shape[0], _dp(a)))

    def get_lambda(self, first_loc=0, n_locs=None):
        n_locs = self.l - first_loc if n_locs is None else n_locs
        out = np.empty((n_locs, self.k, 2), dtype=np.float64)
        self._check(self.h.tsamd_get_lambda(self.ctx, first_loc, n_locs, _dp(out)))
        return out

    def get_ebeta(self, first_loc=0, n_locs=None):
        n_locs = self.l - first_loc if n_locs is None else n_locs
        out = np.empty((n_locs, self.k), dtype=np.float64)
        self._check(self.h.tsamd_get_ebeta(self.ctx, first_loc, n_locs, _dp(out)))
        return out

    def get_elogbeta(self, first_loc=0, n_locs=None):
        n_locs = self.l - first_loc if n_locs is None else n_locs
        out = np.empty((n_locs, self.k, 2), dtype=np.float64)
        self._check(self.h.tsamd_get_elogbeta(self.ctx, first_loc, n_locs, _dp(out)))
        return out

    # -- the hot path -----------------------------------------------------------
    def snp_update(self, loc, hol_mode=0):
        it = C.c_uint32(0)
        self._check(self.h.tsamd_snp_update(self.ctx, loc, int(hol_mode), C.byref(it)))
        return it.value

    def run_schedule(self, locs, hol_mode=0):
        a = np.ascontiguousarray(locs, dtype=np.uint32)
        self._check(self.h.tsamd_run_schedule(self.ctx, _up(a), a.size, int(hol_mode)))

    def synchronize(self):
        self._check(self.h.tsamd_synchronize(self.ctx))

    def prepare(self):
        """capture + instantiate the replayed hipGraphs now (otherwise the first run_schedule does)"""
        self._check(self.h.tsamd_prepare(self.ctx))

    def total_passes(self):
        v = C.c_uint64(0)
        self._check(self.h.tsamd_total_passes(self.ctx, C.byref(v)))
        return v.value

    def pass_histogram(self):
        """completed SNP updates by inner passes run (index = passes; last bin = that many or more)"""
        h = np.zeros(_lib.PASS_HIST_BINS, dtype=np.uint64)
        self._check(self.h.tsamd_pass_histogram(self.ctx, h.ctypes.data_as(C.POINTER(C.c_uint64))))
        return h

    def clear_pending(self):
        self._check(self.h.tsamd_clear_pending(self.ctx))

    def heldout_loglik(self, loc):
        s, c = C.c_double(0), C.c_uint32(0)
        self._check(self.h.tsamd_heldout_loglik(self.ctx, loc, C.byref(s), C.byref(c)))
        return s.value, c.value

    def heldout_eval(self, locs, run_updates=True):
        """(sum, count, per-location sums, per-location counts) of the held-out log-likelihood over
        locs -- tsamd_heldout_eval: the validation block of compute_likelihood in one call."""
        a = np.ascontiguousarray(locs, dtype=np.uint32)
        sums = np.zeros(a.size, dtype=np.float64)
        cnts = np.zeros(a.size, dtype=np.uint32)
        s, c = C.c_double(0), C.c_uint32(0)
        self._check(self.h.tsamd_heldout_eval(self.ctx, _up(a), a.size, int(run_updates), _dp(sums), _up(cnts),
                                              C.byref(s), C.byref(c)))
        return s.value, c.value, sums, cnts

    def train_loglik(self, locs=None, per_loc=True, per_indiv=True):
        """training-data log-likelihood of the current state over locs (None: every location) -- tsamd_train_loglik:
        dict(sum, count[, loc_sums, loc_counts][, indiv_sums, indiv_counts]); the per-individual arrays cover this
        engine's shard.  Changes no state."""
        if locs is None:
            a, n_locs = None, self.l
        else:
            a = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = a.size
        ls = np.zeros(n_locs, dtype=np.float64) if per_loc else None
        lc = np.zeros(n_locs, dtype=np.uint32) if per_loc else None
        ns = np.zeros(self.shard_count, dtype=np.float64) if per_indiv else None
        nc = np.zeros(self.shard_count, dtype=np.uint32) if per_indiv else None
        s, c = C.c_double(0), C.c_uint64(0)
        self._check(self.h.tsamd_train_loglik(self.ctx, None if a is None else _up(a), n_locs,
                                              None if ls is None else _dp(ls), None if lc is None else _up(lc),
                                              None if ns is None else _dp(ns), None if nc is None else _up(nc),
                                              C.byref(s), C.byref(c)))
        out = dict(sum=s.value, count=c.value)
        if per_loc:
            out.update(loc_sums=ls, loc_counts=lc)
        if per_indiv:
            out.update(indiv_sums=ns, indiv_counts=nc)
        return out

    def fold_in(self, locs=None, max_iters=100, tol=0.0):
        """fit this shard's gamma against the engine's lambda, held fixed, over locs (None: every location) --
        tsamd_fold_in: dict(iters [shard_count], change [shard_count], n_converged, iters_run).  Starts from the current
        gamma; an individual whose change falls below tol is frozen; tol = 0 runs exactly max_iters updates."""
        if locs is None:
            a, n_locs = None, self.l
        else:
            a = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = a.size
        it = np.zeros(self.shard_count, dtype=np.uint32)
        ch = np.zeros(self.shard_count, dtype=np.float64)
        nc, ran = C.c_uint32(0), C.c_uint32(0)
        self._check(self.h.tsamd_fold_in(self.ctx, None if a is None else _up(a), n_locs, int(max_iters), float(tol),
                                         _up(it), _dp(ch), C.byref(nc), C.byref(ran)))
        return dict(iters=it, change=ch, n_converged=nc.value, iters_run=ran.value)

    def kinship(self, indivs=None, locs=None, parts=False):
        """admixture-adjusted relatedness (REAP) of the listed individuals (GLOBAL ids inside this engine's shard; None: the
        whole shard) over locs (None: every location) -- tsamd_kinship: kin [m][m], or (kin, num, den) when parts is true.
        The diagonal is (1 + F) / 2.  Changes no state."""
        if indivs is None:
            ia, m = None, self.shard_count
        else:
            ia = np.ascontiguousarray(indivs, dtype=np.uint32)
            m = ia.size
        if locs is None:
            la, n_locs = None, self.l
        else:
            la = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = la.size
        kin = np.zeros((m, m), dtype=np.float64)
        num = np.zeros((m, m), dtype=np.float64) if parts else None
        den = np.zeros((m, m), dtype=np.float64) if parts else None
        self._check(self.h.tsamd_kinship(self.ctx, None if ia is None else _up(ia), m, None if la is None else _up(la), n_locs,
                                         _dp(kin), None if num is None else _dp(num), None if den is None else _dp(den)))
        return (kin, num, den) if parts else kin

    def snp_scan(self, locs=None, trait=None):
        """per-location sufficient statistics of the structure-adjusted fit and association tests over locs (None: every
        location) -- tsamd_snp_scan: dict(fit_sums [n_locs][4], fit_counts [n_locs][3][, trait_sums [n_locs][6], trait_counts
        [n_locs]]); trait is [shard_count] with NaN for an individual that is not phenotyped.  Every value is a plain sum over
        this engine's shard: add the shards' arrays, then scan_statistics gives z and p.  Changes no state."""
        if locs is None:
            a, n_locs = None, self.l
        else:
            a = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = a.size
        t = None
        if trait is not None:
            t = np.ascontiguousarray(trait, dtype=np.float64)
            if t.shape != (self.shard_count,):
                raise ValueError(f"trait must be [{self.shard_count}]")
        fs = np.zeros((n_locs, _lib.SCAN_FIT_SUMS), dtype=np.float64)
        fc = np.zeros((n_locs, _lib.SCAN_FIT_COUNTS), dtype=np.uint32)
        ts = np.zeros((n_locs, _lib.SCAN_TRAIT_SUMS), dtype=np.float64) if t is not None else None
        tc = np.zeros(n_locs, dtype=np.uint32) if t is not None else None
        self._check(self.h.tsamd_snp_scan(self.ctx, None if a is None else _up(a), n_locs, None if t is None else _dp(t), _dp(fs), _up(fc),
                                          None if ts is None else _dp(ts), None if tc is None else _up(tc)))
        out = dict(fit_sums=fs, fit_counts=fc)
        if t is not None:
            out.update(trait_sums=ts, trait_counts=tc)
        return out

    def ld(self, locs=None, window=64):
        """structure-adjusted LD of the listed locations (None: every location) at most `window` list positions apart, over
        this engine's shard -- tsamd_ld: dict(num, cnt), bands [n_locs][window + 1] whose column d of row i is the pair
        (i, i + d).  Both are plain sums: add the shards' bands, then ld_statistics gives r and p and ld_prune the positions
        to keep.  Changes no state."""
        if locs is None:
            a, n_locs = None, self.l
        else:
            a = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = a.size
        window = int(window)
        cols = window + 1 if 0 <= window <= _lib.LD_MAX_WINDOW else 1  # (a bad window is the library's to refuse)
        num = np.zeros((n_locs, cols), dtype=np.float64)
        cnt = np.zeros((n_locs, cols), dtype=np.uint32)
        self._check(self.h.tsamd_ld(self.ctx, None if a is None else _up(a), n_locs, window & 0xffffffff, _dp(num), _up(cnt)))
        return dict(num=num, cnt=cnt)

    def theta_info(self, indivs=None, locs=None):
        """information matrices of theta of the listed individuals (GLOBAL ids inside this engine's shard; None: the whole
        shard) over locs (None: every location) -- tsamd_theta_info: dict(obs, exp), each [m][P] packed (info_unpack), the
        observed and the expected information with lambda held fixed.  Both are plain sums over the locations; theta_se turns
        either into standard errors.  Changes no state."""
        if indivs is None:
            ia, m = None, self.shard_count
        else:
            ia = np.ascontiguousarray(indivs, dtype=np.uint32)
            m = ia.size
        if locs is None:
            la, n_locs = None, self.l
        else:
            la = np.ascontiguousarray(locs, dtype=np.uint32)
            n_locs = la.size
        obs = np.zeros((m, info_packed(self.k)), dtype=np.float64)
        exp = np.zeros((m, info_packed(self.k)), dtype=np.float64)
        self._check(self.h.tsamd_theta_info(self.ctx, None if ia is None else _up(ia), m, None if la is None else _up(la), n_locs,
                                            _dp(obs), _dp(exp)))
        return dict(obs=obs, exp=exp)

    # -- the full state: save / restore ------------------------------------------
    def state_sizes(self):
        """(indiv_bytes, loc_bytes) of the two state blobs -- tsamd_state_sizes"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.h.tsamd_state_sizes(self.ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def state_export(self, indiv=True, loc=True):
        """(indiv, loc): the shard's own part (gamma, the stored w, c_n) and the location part (lambda, the stored
        exp(Elogbeta), the pending gamma step, the pass counters) as uint8 arrays -- tsamd_state_export; a part that is
        not asked for comes back as None"""
        ni, nl = self.state_sizes()
        a = np.empty(ni, dtype=np.uint8) if indiv else None
        b = np.empty(nl, dtype=np.uint8) if loc else None
        self._check(self.h.tsamd_state_export(self.ctx, a.ctypes.data if indiv else None, ni if indiv else 0,
                                              b.ctypes.data if loc else None, nl if loc else 0))
        return a, b

    def state_import(self, indiv=None, loc=None):
        """restore either part or both (uint8 arrays / bytes from state_export); validated before anything is touched --
        tsamd_state_import"""
        a = None if indiv is None else np.ascontiguousarray(np.frombuffer(indiv, dtype=np.uint8))
        b = None if loc is None else np.ascontiguousarray(np.frombuffer(loc, dtype=np.uint8))
        self._check(self.h.tsamd_state_import(self.ctx, None if a is None else a.ctypes.data, 0 if a is None else a.size,
                                              None if b is None else b.ctypes.data, 0 if b is None else b.size))

    # -- multi-GPU --------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
        rc = self.h.tsamd_comm_unique_id(buf)
        if rc != 0:
            raise _lib.TsamdError(rc, self.h.tsamd_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, uid):
        assert len(uid) == _lib.COMM_ID_BYTES
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        self._check(self.h.tsamd_comm_init(self.ctx, buf))

    def p2p_export(self):
        buf = (C.c_uint8 * _lib.P2P_HANDLE_BYTES)()
        self._check(self.h.tsamd_p2p_export(self.ctx, buf))
        return bytes(buf)

    def p2p_connect(self, handles):
        """handles: list of world byte strings in rank order (tsamd_p2p_export of every rank)."""
        blob = b"".join(handles)
        assert len(blob) == self.world * _lib.P2P_HANDLE_BYTES
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        self._check(self.h.tsamd_p2p_connect(self.ctx, buf))

    @staticmethod
    def p2p_connect_local(engines):
        """Peer-to-peer exchange between engines of THIS process (ranks 0..world-1, one each).
        Afterwards enqueue the same run_schedule on every engine, then synchronize each;
        snp_update would wait for peers that have not been enqueued."""
        arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
        rc = engines[0].h.tsamd_p2p_connect_local(arr, len(engines))
        engines[0]._check(rc)

    @staticmethod
    def run_schedule_all(engines, locs, hol_mode=0):
        """run_schedule on every engine of a p2p_connect_local group (bounded interleaving)."""
        a = np.ascontiguousarray(locs, dtype=np.uint32)
        arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
        engines[0]._check(engines[0].h.tsamd_run_schedule_all(arr, len(engines), _up(a), a.size, int(hol_mode)))

    # -- measurement ------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.h.tsamd_profile_enable(self.ctx, int(on)))

    def profile_read(self):
        pn, fn = C.c_uint64(0), C.c_uint64(0)
        pm, fm = C.c_double(0), C.c_double(0)
        self._check(self.h.tsamd_profile_read(self.ctx, C.byref(pn), C.byref(pm), C.byref(fn), C.byref(fm)))
        return dict(pass_launches=pn.value, pass_ms=pm.value, first_launches=fn.value, first_ms=fm.value)

    def probe_stream(self, reps=50):
        """(read_us, rmw_us): bare streaming read of w / read-modify-write of w and gamma per launch"""
        a, b = C.c_double(0), C.c_double(0)
        self._check(self.h.tsamd_probe_stream(self.ctx, reps, C.byref(a), C.byref(b)))
        return a.value, b.value

    def launch_info(self):
        """dict(kernels_per_snp, plain_grid, first_grid) -- tsamd_launch_info"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self.h.tsamd_launch_info(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(kernels_per_snp=a.value, plain_grid=b.value, first_grid=c.value)

    def schedule_geometry(self, mode=_lib.LAUNCH_PER_SCHEDULE):
        """dict(workgroups, indivs_per_thread, exchange_levels, on_chip_per_thread) of the resident kernel of `mode` --
        tsamd_schedule_geometry (on_chip_per_thread < indivs_per_thread: ts_hybrid, part of the weights streamed)"""
        a, b, c, d = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self.h.tsamd_schedule_geometry(self.ctx, int(mode), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(workgroups=a.value, indivs_per_thread=b.value, exchange_levels=c.value, on_chip_per_thread=d.value)

    def holblock_info(self):
        """dict(batch, launches, locations) of the batched validation block -- tsamd_holblock_info"""
        a, b, c = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.h.tsamd_holblock_info(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return dict(batch=a.value, launches=b.value, locations=c.value)

    def set_launch_mode(self, mode):
        """LAUNCH_PER_PASS / LAUNCH_PER_SNP / LAUNCH_PER_SCHEDULE -- tsamd_set_launch_mode"""
        self._check(self.h.tsamd_set_launch_mode(self.ctx, int(mode)))

    def recoveries(self):
        """times a resident launch found its workgroups not all resident and the schedule was replayed launch per pass"""
        v = C.c_uint32(0)
        self._check(self.h.tsamd_recoveries(self.ctx, C.byref(v)))
        return v.value

    def debug_occupy(self, workgroups, milliseconds):
        """test aid: hold `workgroups` compute units for `milliseconds` with a kernel on a second stream"""
        self._check(self.h.tsamd_debug_occupy(self.ctx, int(workgroups), int(milliseconds)))

    def last_error(self):
        return self.h.tsamd_last_error(self.ctx).decode()

    def mem_info(self):
        f, t = C.c_uint64(0), C.c_uint64(0)
        self._check(self.h.tsamd_mem_info(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value
