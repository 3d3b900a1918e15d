"""numpy restatement of the conditional chains (include/gml.h: gml_problem_create_mcmc_terms_conditional, gml_conditional_means),
always as the FULL WALK: every update sums all incidences of the hidden spin.  Built on the quantised model of the term chains
(_term_chains_reference.quantise_spins) and the samplers' u01 (_mcmc_chains_reference.u01), vectorised over chains.
Terms are (1-based key tuple, weight) pairs or a dict of them; evidence is int8 [K, n] of +-1; hidden the 0-based hidden spins.
Chain c = r K + k is replica r of evidence row k.  Returns (states int8 [chains * samples_per_chain, n], row t chains + c;
means float64 [chains, H], the hidden spins ascending)."""
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


def conditional(terms, n, evidence, hidden, replicas, samples_per_chain, burn_in, thin, seed):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    evidence = np.asarray(evidence)
    K = evidence.shape[0]
    assert evidence.shape == (K, n) and set(np.unique(evidence)) <= {-1, 1}
    hid = sorted(int(i) for i in hidden)
    assert hid and len(set(hid)) == len(hid) and 0 <= hid[0] and hid[-1] < n and replicas >= 1
    spins = [(a, sig, _grouped(q)) for a, sig, q in quantise_spins(terms, n)]
    nchains = K * replicas
    c = np.arange(nchains, dtype=np.uint64)
    S = np.tile(evidence.T.astype(np.int64), (1, replicas))  # [n, chains]: column r K + k is row k
    for i in hid:
        S[i] = np.where(u01(seed, 0xFFFFFFFF, c * np.uint64(n) + np.uint64(i)) < 0.5, 1, -1)
    out = np.empty((nchains * samples_per_chain, n), dtype=np.int8)
    acc = np.zeros((len(hid), nchains))
    for sw in range(burn_in + (samples_per_chain - 1) * thin):
        done = sw + 1
        recorded = done >= burn_in and (done - burn_in) % thin == 0
        for a_, i in enumerate(hid):
            a, sig, groups = spins[i]
            tot = np.zeros(nchains, dtype=np.int64)
            for qs, os in groups:
                tot += qs @ S[os].prod(axis=1)  # exact: |sum| < 2^24 2^38
            h = a + sig * tot.astype(np.float64)
            pup = 1.0 / (1.0 + np.exp(-2.0 * h))
            S[i] = np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1, -1)
            if recorded:
                acc[a_] = acc[a_] + (2.0 * pup - 1.0)
        if recorded:
            t = (done - burn_in) // thin
            out[t * nchains:(t + 1) * nchains] = S.T.astype(np.int8)
    return out, (acc * (1.0 / samples_per_chain)).T.copy()


def exact_conditional(terms, n, row, hidden):
    """By enumeration over the 2^H hidden configurations of one evidence row (unquantised weights): (p [2^H], configuration j has
    hidden spin a = -1 where bit a of j is set; magnetisation [H])"""
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    hid = sorted(int(i) for i in hidden)
    H = len(hid)
    states = np.tile(np.asarray(row, dtype=np.float64), (1 << H, 1))
    conf = np.where((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1, -1.0, 1.0)
    states[:, hid] = conf
    E = np.zeros(1 << H)
    for k, w in terms:
        E += w * np.prod(states[:, [i - 1 for i in k]], axis=1)
    p = np.exp(E - E.max())
    p /= p.sum()
    return p, p @ conf


def random_rows(K, n, seed):
    """int8 [K, n] of +-1: evidence rows"""
    return np.where(np.random.default_rng(seed).random((K, n)) < 0.5, -1, 1).astype(np.int8)


def closed_form_bound(terms, n, i):
    """deg_i sigma_i / 2 + 1e-15 for the mean of a single hidden spin i (0-based) against tanh of its brute-force field: the 2^-38
    quantisation of at most deg_i couplings (each off by at most sigma_i / 2); tanh has slope <= 1"""
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    _, sig, q = quantise_spins(terms, n)[i]
    return len(q) * sig / 2 + 1e-15


# the enumeration case of the host and the device tests: 8192 independent chains per evidence row, recorded once
ENUM = dict(n=10, hidden=[1, 4, 6, 9], K=6, replicas=8192, burn_in=40, seed=3)


def enum_model():
    from _ais_reference import sparse_model
    return sparse_model(10, 6, 3, 0.5, 7), random_rows(ENUM["K"], ENUM["n"], 1)


def check_enumeration(terms, ev, states, means):
    """states int8 [R K, n] (the one recorded sweep), means [R K, H], chain r K + k.  For every row: each of the 16 hidden
    configurations has a count within 6 binomial standard deviations of R p, p its exact conditional probability; the
    replica-averaged mean of every hidden spin lies within 6 of its own standard errors (sample std over replicas / sqrt R) of the
    exact conditional magnetisation.  The chains are independent and recorded once, so both are plain 6 sigma bounds.  Returns the
    worst z-scores (cells, means)."""
    n, hid, K, R = ENUM["n"], ENUM["hidden"], ENUM["K"], ENUM["replicas"]
    st = np.asarray(states).reshape(R, K, n)
    mn = np.asarray(means).reshape(R, K, len(hid))
    worst_cell = worst_mean = 0.0
    for k in range(K):
        p, mag = exact_conditional(terms, n, ev[k], hid)
        code = ((st[:, k][:, hid] < 0) << np.arange(len(hid))).sum(axis=1)
        z = np.abs(np.bincount(code, minlength=16) - R * p) / np.sqrt(R * p * (1 - p))
        zm = np.abs(mn[:, k].mean(axis=0) - mag) / (mn[:, k].std(axis=0, ddof=1) / np.sqrt(R))
        worst_cell, worst_mean = max(worst_cell, z.max()), max(worst_mean, zm.max())
        assert z.max() < 6, (k, z)
        assert zm.max() < 6, (k, zm)
    return worst_cell, worst_mean


def exact_field(terms, n, row, i):
    """the brute-force FP64 field of spin i (0-based) at the state `row`, from the unquantised weights"""
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    s = np.asarray(row, dtype=np.float64)
    h = 0.0
    for k, w in terms:
        sp = []
        for v in k:  # a spin named twice cancels
            v = int(v) - 1
            sp.remove(v) if v in sp else sp.append(v)
        if i in sp:
            h += w * float(np.prod([s[j] for j in sp if j != i]))
    return h
