"""A planted late-training state (seeded, deterministic) for parity tests far from the fresh start.

A production run (L = 5e5 ... 1e6 SNPs) spends nearly all of its updates with gamma rows summing to K alpha + 2 L_eff
(most components near alpha, one or two near 2 L_eff), c_n in the thousands (rho ~ 0.01 ... 0.03), lambda of order N
(Ebeta from ~1e-7 to 1 - 1e-7) and softmax exponents 20 and more apart.  plant() builds such a state for a small l:
gamma_scale = L_eff in both the engine and the oracle, so every gamma step moves the rows on that scale.
"""
import numpy as np

from helpers import pack_bed


class Late:
    """n, l, k, l_eff, y [l][n] (3 = missing), payload, gamma [n][k], counts [n], lam [l][k][2], held {loc: indivs}"""


def plant(n, l, k, seed, l_eff=5e5, held_locs=(1, 4, 6), missing_rate=0.02, n_eff=None):
    """n_eff: the sample size lambda is scaled to (None: n itself); 1e6 puts Ebeta within 1e-6 of 0 and 1 at a small n"""
    rng = np.random.default_rng(seed)
    alpha, eta = 1.0 / k, 1.0
    theta = rng.dirichlet(np.full(k, 0.05), size=n)                  # [n][k]
    beta = rng.uniform(0.0, 1.0, size=(l, k))
    # loci where one population's allele frequency is exactly 0 or 1: that side of lambda stays at eta
    for loc in range(0, l, 3):
        beta[loc, rng.integers(k)] = float(rng.integers(2))
    p = np.clip(theta @ beta.T, 0.0, 1.0).T                          # [l][n]
    y = (rng.random((l, n)) < p).astype(np.uint8) + (rng.random((l, n)) < p).astype(np.uint8)
    y[rng.random((l, n)) < missing_rate] = 3
    # gamma: alpha + (K alpha + 2 L_eff) theta, perturbed; a few rows with components at the 1e-8 floor
    gamma = alpha + (k * alpha + 2.0 * l_eff) * theta * np.exp(0.05 * rng.standard_normal((n, k)))
    floor_rows = rng.choice(n, size=max(4, n // 500), replace=False)
    for i in floor_rows:
        gamma[i, rng.choice(k, size=max(1, k // 3), replace=False)] = 1e-8
    # c_n: thousands; a few fresh individuals and a few near 1e6
    counts = rng.integers(0, 20_001, size=n).astype(np.uint32)
    counts[rng.choice(n, size=8, replace=False)] = 0
    counts[rng.choice(n, size=8, replace=False)] = (1_000_000 - rng.integers(0, 1000, size=8)).astype(np.uint32)
    # lambda = eta + 2 N share_k (beta, 1 - beta), N = n_eff where given
    share = theta.mean(axis=0)
    pop = n if n_eff is None else n_eff
    lam = np.empty((l, k, 2))
    lam[:, :, 0] = eta + 2.0 * pop * share[None, :] * beta
    lam[:, :, 1] = eta + 2.0 * pop * share[None, :] * (1.0 - beta)
    held = {}
    for loc in held_locs:
        cand = np.nonzero(y[loc] != 3)[0]
        held[loc] = np.sort(rng.choice(cand, size=max(1, len(cand) // 50), replace=False)).astype(np.uint32)
    s = Late()
    s.n, s.l, s.k, s.l_eff = n, l, k, l_eff
    s.y, s.payload, s.gamma, s.counts, s.lam, s.held = y, pack_bed(y), gamma, counts, lam, held
    s.floor_rows = np.sort(floor_rows)
    return s


def load_engine(eng, s):
    """the planted state into an engine of ONE shard"""
    eng.upload_bed(s.payload)
    for loc, ind in s.held.items():
        eng.set_heldout(loc, ind)
    b, c = eng.shard_begin, eng.shard_count
    eng.set_gamma(s.gamma[b:b + c])
    eng.set_counts(s.counts[b:b + c])
    for loc in range(s.l):
        eng.set_lambda(loc, s.lam[loc])


def load_oracle(orc, s):
    orc.load_bed_payload(s.payload)
    for loc, ind in s.held.items():
        orc.set_heldout(loc, ind)
    orc.set_gamma(s.gamma)
    orc.set_counts(s.counts)
    for loc in range(s.l):
        orc.set_lambda(loc, s.lam[loc])
