"""numpy restatement of gml_conditional_draw and gml_conditional_draw_masked (include/gml.h): exact draws of a row's hidden spins by
Gumbel-max over the row's enumeration.  The energies E_k(s) of the 2^h local states are those of _cond_exact_reference.py (all terms,
the row's constant included) summed by _best_reference._energies in np.longdouble; the perturbation is the rule of the header,
    u = u01(seed, c, s)  (the hash of gml_rng.h, _mcmc_chains_reference.u01: stream = chain c, counter = state s),
    g = -log(-log u) (u = 0: -inf),  key(c, s) = E_k(s) + g,
in long double, and the draw of chain c is the first state of largest key (numpy's argmax: the lower state of equal keys).  Chain
c = r K + k is replica r of row k.  Every function also returns each chain's GAP between its best and second-best key (inf for a row
without a hidden spin): where the gap exceeds the rounding of the device's energies and logarithms the device must give the same state.
Models are {1-based key tuple: weight} dicts; rows are +-1 vectors [n]; hidden holds 0-BASED spins; h <= 20."""
import numpy as np

from _best_reference import _energies
from _cond_exact_reference import row_coefficients
from _exact_reference import LD, reduce_key
from _mcmc_chains_reference import u01


def gumbel(seed, chain, nstates):
    """g(c, s) for s = 0 .. nstates - 1, long double"""
    u = u01(seed, chain, np.arange(nstates, dtype=np.uint64)).astype(LD)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def row_energies(terms, row, hidden):
    """(E long double [2^h], log_w) of one row"""
    hid = sorted(int(i) for i in hidden)
    E = _energies(len(hid), list(row_coefficients(terms, np.asarray(row), hid).items()))
    m = E.max()
    return E, m + np.log(np.exp(E - m).sum())


def draw_of(E, log_w, seed, chain):
    """(local state, its unperturbed energy, its log_p, the gap of the keys) of one chain on the energies of its row"""
    key = E + gumbel(seed, chain, len(E))
    best = int(np.argmax(key))
    rest = np.delete(key, best)
    gap = float(key[best] - rest.max()) if len(rest) else float("inf")
    return best, E[best], E[best] - log_w, gap


def cond_draw_masked(terms, n, rows, mask, replicas, seed, chains=None):
    """every row under its own hidden set mask[k] (bool [K, n]), `replicas` chains per row: (completed int8 [K replicas, n], energy,
    log_p, gap [K replicas]), chain r K + k at that place.  chains [K replicas] (optional): the chain numbers to use instead."""
    rows, mask = np.asarray(rows), np.asarray(mask, dtype=bool)
    K, R = len(rows), int(replicas)
    done = np.tile(rows.astype(np.int8), (R, 1))
    energy, log_p, gap = np.zeros(K * R, dtype=LD), np.zeros(K * R, dtype=LD), np.zeros(K * R)
    for k, row in enumerate(rows):
        hid = np.flatnonzero(mask[k])
        E, log_w = row_energies(terms, row, hid)
        for r in range(R):
            c = r * K + k
            best, energy[c], log_p[c], gap[c] = draw_of(E, log_w, seed, c if chains is None else int(chains[c]))
            done[c, hid] = [-1 if (best >> j) & 1 else 1 for j in range(len(hid))]
    return done, energy, log_p, gap


def cond_draw_masked_grouped(terms, n, rows, mask, replicas, seed):
    """cond_draw_masked (completed rows only) for many rows of few spins: the rows that share a hidden set are walked together -- every
    term's product over [rows, states] at once, long double, the same rule and the same chain numbers.  The host loop of learn_missing
    completes 20000 rows of 8 spins with it."""
    rows, mask = np.asarray(rows), np.asarray(mask, dtype=bool)
    K, R = len(rows), int(replicas)
    done = np.tile(rows.astype(np.int8), (R, 1))
    items = [(reduce_key(key), w) for key, w in (terms.items() if isinstance(terms, dict) else terms) if w != 0.0]
    packed = np.packbits(mask, axis=1)
    for pattern in np.unique(packed, axis=0):
        members = np.flatnonzero((packed == pattern).all(axis=1))
        hid = np.flatnonzero(mask[members[0]])
        h = len(hid)
        if h == 0:
            continue
        bits = ((np.arange(1 << h)[:, None] >> np.arange(h)) & 1).astype(bool)  # [states, h]
        X = np.repeat(rows[members][:, None, :].astype(np.int8), 1 << h, axis=1)  # [members, states, n]
        X[:, :, hid] = np.where(bits, -1, 1)[None]
        E = np.zeros(X.shape[:2], dtype=LD)
        for sp, w in items:
            E += LD(w) * np.prod(X[:, :, [v - 1 for v in sp]], axis=2)
        for r in range(R):
            chain = (r * K + members).astype(np.uint64)
            u = u01(seed, chain[:, None], np.arange(1 << h, dtype=np.uint64)[None, :]).astype(LD)
            with np.errstate(divide="ignore"):
                best = np.argmax(E - np.log(-np.log(u)), axis=1)
            done[(r * K + members)[:, None], hid[None, :]] = np.where(bits[best], -1, 1)
    return done


def cond_draw_rows(terms, n, rows, hidden, replicas, seed):
    """every row under one hidden set: (states int8 [K replicas, h], the hidden spins ascending; energy; log_p; gap)"""
    rows = np.asarray(rows)
    hid = sorted(int(i) for i in hidden)
    mask = np.zeros(rows.shape, dtype=bool)
    mask[:, hid] = True
    done, energy, log_p, gap = cond_draw_masked(terms, n, rows, mask, replicas, seed)
    return np.ascontiguousarray(done[:, hid]), energy, log_p, gap


def state_probabilities(terms, row, hidden):
    """P(local state | the row's visible spins), float64 [2^h]: the softmax of the row's energies"""
    E, log_w = row_energies(terms, row, hidden)
    return np.exp(E - log_w).astype(np.float64)


def codes_of(states):
    """the local states of int8 [C, h] draws: bit j set iff the j-th hidden spin is -1"""
    st = np.asarray(states)
    return ((st < 0).astype(np.int64) << np.arange(st.shape[1])).sum(axis=1)
