"""numpy restatement of gml_log_partition_ais (include/gml.h): the quantised model of the term chains
(_term_chains_reference.quantise_spins), the start energy that counts every term once at its smallest spin, the weight update
logw -= (beta_t - beta_(t-1)) E in three roundings, the heat-bath sweeps at beta_t with the tracked energy E -= (s_new - s_old) h,
vectorised over chains.  Terms are (1-based key tuple, weight) pairs or a dict of them.  ais() returns (logw [chains], E [chains],
the final +-1 states [chains, n]); summary() the `result` triple; exact_log_z() log Z by enumeration; lattice() and sparse_model()
are the test models of the chain tests."""
import numpy as np

from _mcmc_chains_reference import u01
from _term_chains_reference import quantise_spins


def _grouped(q):
    groups = {}
    for qe, o in q:
        groups.setdefault(len(o), ([], []))
        groups[len(o)][0].append(qe)
        groups[len(o)][1].append(o)
    return [(np.array(qs, dtype=np.int64), np.array(os, dtype=np.int64)) for qs, os in groups.values()]


def _int_field(groups, S, nchains):
    tot = np.zeros(nchains, dtype=np.int64)
    for qs, os in groups:
        tot += qs @ S[os].prod(axis=1)  # exact: |sum| < 2^24 2^38
    return tot


def ais(terms, n, nchains, betas, sweeps_per_step, seed):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    betas = np.asarray(betas, dtype=np.float64)
    assert len(betas) >= 2 and betas[0] == 0.0
    spins = [(a, sig, _grouped(q), _grouped([(qe, o) for qe, o in q if min(o) > i])) for i, (a, sig, q) in enumerate(quantise_spins(terms, n))]
    c = np.arange(nchains, dtype=np.uint64)
    S = np.empty((n, nchains), dtype=np.int64)
    for i in range(n):
        S[i] = np.where(u01(seed, 0xFFFFFFFF, c * np.uint64(n) + np.uint64(i)) < 0.5, 1, -1)
    E = np.zeros(nchains)
    for i in range(n):
        a, sig, _, upper = spins[i]
        t = a + sig * _int_field(upper, S, nchains).astype(np.float64)
        E = E - S[i].astype(np.float64) * t
    logw = np.zeros(nchains)
    sw = 0
    for t in range(1, len(betas)):
        d = betas[t] - betas[t - 1]
        p = d * E
        logw = logw - p
        for _ in range(sweeps_per_step):
            for i in range(n):
                a, sig, groups, _ = spins[i]
                h = a + sig * _int_field(groups, S, nchains).astype(np.float64)
                pup = 1.0 / (1.0 + np.exp(-2.0 * (betas[t] * h)))
                new = np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1, -1)
                E = E - (new - S[i]).astype(np.float64) * h
                S[i] = new
            sw += 1
    return logw, E, S.T.astype(np.int8)


def summary(logw, n):
    """result[0..3) of the contract: log Z, its delta-method standard error, the effective sample size"""
    logw = np.asarray(logw, dtype=np.float64)
    chains = len(logw)
    m = logw.max()
    x = np.exp(logw - m)
    s1, s2 = 0.0, 0.0
    for v in x.tolist():  # in chain order, as the library adds them
        s1 += v
        s2 += v * v
    mean = s1 / chains
    se = float(np.sqrt(max(s2 / chains - mean * mean, 0.0) / (chains - 1)) / mean) if chains > 1 else 0.0
    return float(n * np.log(2.0) + m + np.log(mean)), se, s1 * s1 / s2


def energies(terms, states):
    """E(s) = - sum_t w_t prod s of every row of states [K, n] (+-1), from the unquantised weights"""
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    s = np.asarray(states, dtype=np.float64)
    en = np.zeros(len(s))
    for k, w in terms:
        en -= w * np.prod(s[:, [i - 1 for i in k]], axis=1)
    return en


def exact_log_z(terms, n):
    states = ((np.arange(2 ** n)[:, None] >> np.arange(n)) & 1) * 2 - 1
    en = -energies(terms, states)
    m = en.max()
    return float(m + np.log(np.exp(en - m).sum()))


# the helpers of tests/test_gpu_tempered.py
def lattice(L, J, h, seed):
    rng = np.random.default_rng(seed)
    idx = lambda x, y: (x % L) * L + (y % L) + 1  # noqa: E731
    terms = {}
    for x in range(L):
        for y in range(L):
            terms[(idx(x, y), idx(x + 1, y))] = J * rng.choice([-1.0, 1.0])
            terms[(idx(x, y), idx(x, y + 1))] = J * rng.choice([-1.0, 1.0])
    for i in range(L * L):
        terms[(i + 1,)] = rng.normal(scale=h)
    return terms


def sparse_model(n, n3, n2, scale, seed, order=3, fields=True):
    """about n3 order-`order` and n2 pairwise terms per spin, random spins, N(0, scale^2) weights"""
    rng = np.random.default_rng(seed)
    terms = {}
    for _ in range(n * n3 // order):
        terms[tuple(int(v) for v in rng.choice(n, order, replace=False) + 1)] = float(rng.normal(scale=scale))
    for _ in range(n * n2 // 2):
        terms[tuple(int(v) for v in rng.choice(n, 2, replace=False) + 1)] = float(rng.normal(scale=scale))
    if fields:
        for i in range(n):
            terms[(i + 1,)] = float(rng.normal(scale=0.2))
    return terms
