"""numpy restatement of gml_problem_create_mcmc_terms_tempered (include/gml.h): the quantised model of the term chains
(_term_chains_reference.quantise_spins), R rungs per ladder that start from the state of chain l R, the heat-bath update at beta_r
with the rung's own stream, the tracked relative energy E -= (s_new - s_old) h (one rounding per flip) and the swap rounds of
alternating parity, vectorised over ladders.  Terms are (1-based key tuple, weight) pairs or a dict of them.  Returns (the +-1 states
of rung 0, row t * ladders + l; swap_counts [2][R-1] = attempts, accepts)."""
import numpy as np

from _mcmc_chains_reference import u01
from _term_chains_reference import quantise_spins


def tempered(terms, n, ladders, samples_per_chain, burn_in, thin, betas, swap_every, seed):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    betas = np.asarray(betas, dtype=np.float64)
    R = len(betas)
    spins = []
    for a, sig, q in quantise_spins(terms, n):
        groups = {}
        for qe, o in q:
            groups.setdefault(len(o), ([], []))
            groups[len(o)][0].append(qe)
            groups[len(o)][1].append(o)
        spins.append((a, sig, [(np.array(qs, dtype=np.int64), np.array(os, dtype=np.int64)) for qs, os in groups.values()]))
    ell = np.arange(ladders, dtype=np.uint64)
    c = ell[:, None] * np.uint64(R) + np.arange(R, dtype=np.uint64)[None, :]  # [ladders, R]: the chain index of a rung
    S = np.empty((n, ladders, R), dtype=np.int64)
    for i in range(n):
        S[i] = np.where(u01(seed, 0xFFFFFFFF, ell * np.uint64(R) * np.uint64(n) + np.uint64(i)) < 0.5, 1, -1)[:, None]
    E = np.zeros((ladders, R))
    counts = np.zeros((2, max(R - 1, 0)), dtype=np.int64)
    out = np.empty((ladders * samples_per_chain, n), dtype=np.int8)
    for sw in range(burn_in + (samples_per_chain - 1) * thin):
        for i in range(n):
            a, sig, groups = spins[i]
            tot = np.zeros((ladders, R), dtype=np.int64)
            for qs, os in groups:
                tot += np.tensordot(qs, S[os].prod(axis=1), axes=1)  # exact: |sum| < 2^24 2^38
            h = a + sig * tot.astype(np.float64)
            pup = 1.0 / (1.0 + np.exp(-2.0 * (betas[None, :] * h)))
            new = np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1, -1)
            E = E - (new - S[i]).astype(np.float64) * h
            S[i] = new
        done = sw + 1
        if done % swap_every == 0:
            m = done // swap_every
            for r in range((m - 1) % 2, R - 1, 2):
                d = (betas[r] - betas[r + 1]) * (E[:, r] - E[:, r + 1])
                acc = u01(seed, 2 ** 32 + sw, c[:, r]) < np.exp(np.minimum(d, 0.0))
                S[:, acc, r], S[:, acc, r + 1] = S[:, acc, r + 1].copy(), S[:, acc, r].copy()
                E[acc, r], E[acc, r + 1] = E[acc, r + 1].copy(), E[acc, r].copy()
                counts[0, r] += ladders
                counts[1, r] += int(acc.sum())
        if done >= burn_in and (done - burn_in) % thin == 0:
            t = (done - burn_in) // thin
            out[t * ladders:(t + 1) * ladders] = S[:, :, 0].T.astype(np.int8)
    return out, counts


def bimodal_16():
    """16 spins: every pair 0.35, 12 random triples, small fields -- two wells, P(m > 0) = 0.893 and every <s_i> = 0.786 or so"""
    terms = {(i + 1, j + 1): 0.35 for i in range(16) for j in range(i + 1, 16)}
    rng = np.random.default_rng(6)
    for _ in range(12):  # (a later triple with the same key overwrites the earlier one)
        terms[tuple(int(v) for v in np.sort(rng.choice(16, 3, replace=False)) + 1)] = float(rng.normal(scale=0.2))
    for i in range(16):
        terms[(i + 1,)] = float(rng.normal(scale=0.03) + 0.02)
    return terms


def exact_moments(terms, n):
    """(P(m > 0), <s_i> [n], <s_i s_j> [n, n]) by enumeration, E = - sum_t w_t prod s"""
    states = ((np.arange(2 ** n)[:, None] >> np.arange(n)) & 1) * 2 - 1
    en = np.zeros(2 ** n)
    for k, w in terms.items():
        en += w * np.prod(states[:, [i - 1 for i in k]], axis=1)
    p = np.exp(en - en.max())
    p /= p.sum()
    return p[states.sum(axis=1) > 0].sum(), p @ states, (states * p[:, None]).T @ states
