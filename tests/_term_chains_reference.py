"""numpy restatement of gml_problem_create_mcmc_terms_chains (include/gml.h): the incidences of a term list, the per-spin field
sum a_i (left to right in term order), sigma_i and q_e, the exact int64 fields and the heat-bath update, vectorised over chains.
Terms are (1-based key tuple, weight) pairs (a dict's items()); non-positive entries of a key are unused slots.  Returns the +-1
states the handle holds, row t * chains + c."""
import numpy as np

from _mcmc_chains_reference import u01


def incidences(terms, n):
    """per spin: [(weight, other spins (0-based))] in term order; a spin named twice cancels, zero weights are skipped"""
    inc = [[] for _ in range(n)]
    for key, w in terms:
        sp = []
        for v in key:
            v = int(v) - 1
            if v < 0:
                continue
            if v in sp:
                sp.remove(v)
            else:
                sp.append(v)
        if w == 0.0:
            continue
        for a, s in enumerate(sp):
            inc[s].append((float(w), tuple(sp[:a] + sp[a + 1:])))
    return inc


def quantise_spins(terms, n):
    """per spin: (a_i, sigma_i, [(q_e, others)]) with a_i a left-to-right Python sum, q_e Python ints"""
    out = []
    for inc in incidences(terms, n):
        a = 0.0
        for w, o in inc:
            if not o:
                a += w
        coup = [(w, o) for w, o in inc if o]
        mx = max((abs(w) for w, _ in coup), default=0.0)
        ex = int(np.frexp(mx)[1]) if mx > 0 else 0
        q = [(int(np.rint(np.ldexp(w, 38 - ex))), o) for w, o in coup]
        out.append((a, float(np.ldexp(1.0, ex - 38)), q))
    return out


def chains(terms, n, nchains, samples_per_chain, burn_in, thin, seed):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    spins = []
    for a, sig, q in quantise_spins(terms, n):
        groups = {}
        for qe, o in q:
            groups.setdefault(len(o), ([], []))
            groups[len(o)][0].append(qe)
            groups[len(o)][1].append(o)
        spins.append((a, sig, [(np.array(qs, dtype=np.int64), np.array(os, dtype=np.int64)) for qs, os in groups.values()]))
    c = np.arange(nchains, dtype=np.uint64)
    S = np.empty((n, nchains), dtype=np.int64)
    for i in range(n):
        S[i] = np.where(u01(seed, 0xFFFFFFFF, c * np.uint64(n) + np.uint64(i)) < 0.5, 1, -1)
    out = np.empty((nchains * samples_per_chain, n), dtype=np.int8)
    for sw in range(burn_in + (samples_per_chain - 1) * thin):
        for i in range(n):
            a, sig, groups = spins[i]
            tot = np.zeros(nchains, dtype=np.int64)
            for qs, os in groups:
                tot += qs @ S[os].prod(axis=1)  # exact: |sum| < 2^24 2^38
            h = a + sig * tot.astype(np.float64)
            pup = 1.0 / (1.0 + np.exp(-2.0 * h))
            S[i] = np.where(u01(seed, sw, c * np.uint64(n) + np.uint64(i)) < pup, 1, -1)
        done = sw + 1
        if done >= burn_in and (done - burn_in) % thin == 0:
            t = (done - burn_in) // thin
            out[t * nchains:(t + 1) * nchains] = S.T.astype(np.int8)
    return out
