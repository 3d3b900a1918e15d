"""numpy restatement of the two oldest samplers (include/gml.h): the exact block sampler of gml_problem_create_sampled / _sampled_terms
(connected components of the term hypergraph, all 2^sb energies of a block, the normalised CDF, inversion at u01(seed, block, k)),
the FP64 Glauber chains of gml_problem_create_mcmc_terms, and the histogram of gml_problem_create_sampled_hist.  Written from the
header and from the comments of gml_sampler.hip and gml_chain.h; it shares no code with the kernels.  Energies and CDFs are
np.longdouble, so that the reference's own rounding stays far below the bounds the device is held to.
Terms are (1-based key tuple, weight) pairs (a dict's items()); non-positive entries of a key are unused slots."""
import numpy as np

from _mcmc_chains_reference import u01
from _term_chains_reference import incidences


def _items(terms):
    return list(terms.items()) if isinstance(terms, dict) else list(terms)


def _reduced(key):
    """the distinct 0-based spins of a key after cancellation (a spin named twice cancels: s^2 = 1), in the order they are named"""
    sp = []
    for v in key:
        v = int(v) - 1
        if v < 0:
            continue
        if v in sp:
            sp.remove(v)
        else:
            sp.append(v)
    return sp


def blocks(terms, n):
    """Connected components of the term hypergraph: [(spins ascending, masks uint32 [nt], weights float64 [nt])], numbered by
    their smallest spin.  A term joins the spins that remain after cancellation; zero-weight terms and the empty term are dropped.
    Bit t of a mask <=> the block's t-th spin is in the term; the terms of a block keep the order of the list."""
    kept = [(sp, float(w)) for sp, w in ((_reduced(k), w) for k, w in _items(terms)) if w != 0.0 and sp]
    comp = list(range(n))  # comp[i]: the smallest spin known to be connected to i
    changed = True
    while changed:  # label propagation to the fixed point: slow and plain
        changed = False
        for sp, _ in kept:
            m = min(comp[v] for v in sp)
            for v in sp:
                if comp[v] != m:
                    comp[v], changed = m, True
    out = []
    for root in sorted(set(comp)):
        spins = [i for i in range(n) if comp[i] == root]
        pos = {v: t for t, v in enumerate(spins)}
        mine = [(sp, w) for sp, w in kept if comp[sp[0]] == root]
        masks = np.array([sum(1 << pos[v] for v in sp) for sp, _ in mine], dtype=np.uint32)
        out.append((spins, masks, np.array([w for _, w in mine], dtype=np.float64)))
    return out


def block_energies(masks, wts, sb):
    """e(state) = sum_t w_t prod_{i in t} s_i for all 2^sb states (bit i set <=> spin i is +1), np.longdouble, summed in term order"""
    state = np.arange(1 << sb, dtype=np.uint32)
    en = np.zeros(1 << sb, dtype=np.longdouble)
    for m, w in zip(masks, wts):
        x = np.uint32(m) & ~state  # the term's spins that are -1
        for s in (16, 8, 4, 2, 1):
            x = x ^ (x >> np.uint32(s))
        en += np.where(x & np.uint32(1), -np.longdouble(w), np.longdouble(w))
    return en


def block_cdf(en):
    """the normalised inclusive CDF of exp(en - max), np.longdouble; the last entry is exactly 1"""
    p = np.exp(np.asarray(en, dtype=np.longdouble) - np.max(en))
    c = np.cumsum(p)
    c = c / c[-1]
    c[-1] = np.longdouble(1)
    return c


def draw_states(cdf, N, seed, block):
    """(state [N] int64, margin): sample k takes the first state whose cdf > u01(seed, block, k) (the last state at the latest);
    margin = the smallest distance of a u to either edge of its cell [cdf[state - 1], cdf[state]) (cdf[-1] = 0)"""
    u = u01(seed, block, np.arange(N, dtype=np.uint64)).astype(np.longdouble)
    st = np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1)
    lower = np.where(st > 0, cdf[np.maximum(st - 1, 0)], np.longdouble(0))
    margin = min(np.min(cdf[st] - u), np.min(u - lower))
    return st.astype(np.int64), float(margin)


def exact_draws(terms, n, N, seed):
    """(S [N, n] int8, margin) of gml_problem_create_sampled_terms: block b of blocks() draws from the stream u01(seed, b, .)"""
    S = np.zeros((N, n), dtype=np.int8)
    margin = np.inf
    for b, (spins, masks, wts) in enumerate(blocks(terms, n)):
        st, m = draw_states(block_cdf(block_energies(masks, wts, len(spins))), N, seed, b)
        margin = min(margin, m)
        for t, v in enumerate(spins):
            S[:, v] = np.where((st >> t) & 1, 1, -1)
    return S, margin


def glauber(terms, n, N, sweeps, seed):
    """(S [N, n] int8, margin) of gml_problem_create_mcmc_terms: N chains, one sample each after `sweeps` sequential sweeps.
    margin = the smallest |u - pup| of all heat-bath decisions"""
    inc = incidences(_items(terms), n)
    k = np.arange(N, dtype=np.uint64)
    S = np.empty((n, N), dtype=np.float64)
    for i in range(n):
        S[i] = np.where(u01(seed, 0xFFFFFFFF, k * np.uint64(n) + np.uint64(i)) < 0.5, 1.0, -1.0)
    margin = np.inf
    for sw in range(sweeps):
        for i in range(n):
            field = np.zeros(N, dtype=np.float64)
            for w, others in inc[i]:  # left to right in term order, every product +-1: one FP64 rounding per incidence
                pr = np.ones(N, dtype=np.float64)
                for j in others:
                    pr = pr * S[j]
                field = field + w * pr
            pup = 1.0 / (1.0 + np.exp(-2.0 * field))
            u = u01(seed, sw, k * np.uint64(n) + np.uint64(i))
            margin = min(margin, float(np.min(np.abs(u - pup))))
            S[i] = np.where(u < pup, 1.0, -1.0)
    return S.T.astype(np.int8), margin


def histogram(S):
    """(rows [K', n] int8, counts [K'] int64): the distinct rows of S ascending by key (bit i set <=> spin i is -1; n <= 64)"""
    S = np.asarray(S)
    n = S.shape[1]
    assert n <= 64
    keys = np.zeros(len(S), dtype=np.uint64)
    for i in range(n):
        keys |= (S[:, i] < 0).astype(np.uint64) << np.uint64(i)
    uniq, counts = np.unique(keys, return_counts=True)  # unsigned: a key with bit 63 sorts last
    rows = np.where((uniq[:, None] >> np.arange(n, dtype=np.uint64)) & np.uint64(1), -1, 1).astype(np.int8)
    return rows, counts.astype(np.int64)
