"""numpy restatement of the per-row masked conditional chains (include/gml.h: gml_problem_create_mcmc_terms_masked,
gml_conditional_means_masked): the rule of _conditional_reference.conditional with "hidden" read per evidence row.  Every sweep walks
i = 0 .. n - 1; at spin i every chain evaluates the full field (all incidences, the quantised model of the term chains) and the heat
bath, and a chain takes the new spin, and adds to its mean, iff its row hides i.  Vectorised over chains.
Terms are (1-based key tuple, weight) pairs or a dict of them; evidence int8 [K, n] of +-1 (its values at hidden entries play no
part); mask bool [K, n], True = hidden in that row.  Chain c = r K + k is replica r of row k.  Returns (states int8
[chains * samples_per_chain, n], row t chains + c; means float64 [chains, n]: the Rao-Blackwellised mean of a hidden entry, the
evidence value of an observed one)."""
import numpy as np

from _conditional_reference import _grouped, exact_conditional
from _mcmc_chains_reference import u01
from _term_chains_reference import quantise_spins


def masked(terms, n, evidence, mask, replicas, samples_per_chain, burn_in, thin, seed):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    evidence, mask = np.asarray(evidence), np.asarray(mask, dtype=bool)
    K = evidence.shape[0]
    assert evidence.shape == (K, n) and mask.shape == (K, n) and set(np.unique(evidence)) <= {-1, 1} and replicas >= 1
    spins = [(a, sig, _grouped(q)) for a, sig, q in quantise_spins(terms, n)]
    nchains = K * replicas
    c = np.arange(nchains, dtype=np.uint64)
    S = np.tile(evidence.T.astype(np.int64), (1, replicas))  # [n, chains]: column r K + k is row k
    hid = np.tile(mask.T, (1, replicas))  # [n, chains]
    for i in range(n):
        S[i] = np.where(hid[i], np.where(u01(seed, 0xFFFFFFFF, c * np.uint64(n) + np.uint64(i)) < 0.5, 1, -1), S[i])
    out = np.empty((nchains * samples_per_chain, n), dtype=np.int8)
    acc = np.zeros((n, nchains))
    for sw in range(burn_in + (samples_per_chain - 1) * thin):
        done = sw + 1
        recorded = done >= burn_in and (done - burn_in) % thin == 0
        for i in range(n):
            if not hid[i].any():  # (the stream is counter based: what is skipped changes no bit)
                continue
            a, sig, groups = spins[i]
            tot = np.zeros(nchains, dtype=np.int64)
            for qs, os in groups:
                tot += qs @ S[os].prod(axis=1)  # exact: |sum| < 2^24 2^38
            h = a + sig * tot.astype(np.float64)
            pup = 1.0 / (1.0 + np.exp(-2.0 * h))
            S[i] = np.where(hid[i], np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1, -1), S[i])
            if recorded:
                acc[i] = np.where(hid[i], acc[i] + (2.0 * pup - 1.0), acc[i])
        if recorded:
            t = (done - burn_in) // thin
            out[t * nchains:(t + 1) * nchains] = S.T.astype(np.int8)
    means = np.where(hid, acc * (1.0 / samples_per_chain), np.tile(evidence.T.astype(np.float64), (1, replicas)))
    return out, means.T.copy()


def random_mask(K, n, p, seed):
    """bool [K, n]: every entry hidden with probability p"""
    return np.random.default_rng(seed).random((K, n)) < p


def mask_rows(mask):
    """the mask as the int8 rows of its handle: -1 (sign bit set) = hidden, +1 = observed"""
    return np.where(np.asarray(mask, dtype=bool), -1, 1).astype(np.int8)


# the enumeration case of the host and the device tests: 8192 independent chains per evidence row, recorded once after 40 sweeps; every
# row hides its own random set of 2 to 5 spins
ENUM = dict(n=10, K=6, replicas=8192, burn_in=40, seed=3, mask_seed=5)


def enum_model():
    """(terms, evidence int8 [6, 10], mask bool [6, 10])"""
    from _ais_reference import sparse_model
    from _conditional_reference import random_rows
    n, K = ENUM["n"], ENUM["K"]
    rng = np.random.default_rng(ENUM["mask_seed"])
    mask = np.zeros((K, n), dtype=bool)
    for k in range(K):
        mask[k, rng.choice(n, size=int(rng.integers(2, 6)), replace=False)] = True
    return sparse_model(10, 6, 3, 0.5, 7), random_rows(K, n, 1), mask


def check_enumeration(terms, ev, mask, states, means):
    """states int8 [R K, n] (the one recorded sweep), means [R K, n], chain r K + k.  For every row: each configuration of its hidden
    spins has a count within 6 binomial standard deviations of R p, p its exact conditional probability; the replica-averaged mean of
    every hidden spin lies within 6 of its own standard errors (sample std over replicas / sqrt R) of the exact conditional
    magnetisation.  The chains are independent and recorded once, so both are plain 6 sigma bounds.  Returns the worst z-scores
    (cells, means)."""
    n, K, R = ENUM["n"], ENUM["K"], ENUM["replicas"]
    st = np.asarray(states).reshape(R, K, n)
    mn = np.asarray(means).reshape(R, K, n)
    worst_cell = worst_mean = 0.0
    for k in range(K):
        hid = np.flatnonzero(mask[k])
        p, mag = exact_conditional(terms, n, ev[k], hid)
        code = ((st[:, k][:, hid] < 0) << np.arange(len(hid))).sum(axis=1)
        z = np.abs(np.bincount(code, minlength=1 << len(hid)) - R * p) / np.sqrt(R * p * (1 - p))
        zm = np.abs(mn[:, k][:, hid].mean(axis=0) - mag) / (mn[:, k][:, hid].std(axis=0, ddof=1) / np.sqrt(R))
        worst_cell, worst_mean = max(worst_cell, z.max()), max(worst_mean, zm.max())
        assert z.max() < 6, (k, z)
        assert zm.max() < 6, (k, zm)
    return worst_cell, worst_mean
