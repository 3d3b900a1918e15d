"""numpy restatement of gml_conditional_exact (include/gml.h) by brute force in np.longdouble: for one evidence row and one hidden set
every one of the 2^h hidden states is listed and its energy E_k(s_H) = sum_t w_t sigma_{t,k} prod_{i in hid(t)} s_i is summed over ALL
terms (those without a hidden spin and the empty key are the row's constant).  The rules of the contract are here too: a spin named
twice cancels, a zero weight joins nothing.  The states are walked in blocks of 2^18 so that h = 24 needs no table of 2^24 long doubles.
Models are {1-based key tuple: weight} dicts or lists of such pairs; rows are +-1 vectors [n]; hidden holds 0-BASED spins."""
import numpy as np

from _exact_reference import LD, reduce_key

BLOCK_BITS = 18


def _parity(x):
    x = x ^ (x >> 16)
    x = x ^ (x >> 8)
    x = x ^ (x >> 4)
    x = x ^ (x >> 2)
    x = x ^ (x >> 1)
    return (x & 1).astype(bool)


def row_coefficients(terms, row, hidden):
    """{hidden part as a mask over the local bits (bit j <-> the j-th hidden spin, ascending): sum of w_t sigma_t}, long double, in the
    caller's term order"""
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    loc = {s: j for j, s in enumerate(sorted(int(i) for i in hidden))}
    coef = {}
    for key, w in terms:
        if w == 0.0:
            continue
        m, sigma = 0, 1
        for v in reduce_key(key):
            if v - 1 in loc:
                m |= 1 << loc[v - 1]
            else:
                sigma *= int(row[v - 1])
        coef[m] = coef.get(m, LD(0)) + LD(w) * sigma
    return coef


def cond_exact(terms, n, row, hidden):
    """(means long double [h], the hidden spins ascending; log_w; log_p) of one row"""
    row = np.asarray(row)
    assert row.shape == (n,) and set(np.unique(row)) <= {-1, 1}
    hid = sorted(int(i) for i in hidden)
    h = len(hid)
    assert len(set(hid)) == h and (h == 0 or (0 <= hid[0] and hid[-1] < n))
    coef = row_coefficients(terms, row, hid)
    lb = min(h, BLOCK_BITS)
    low = (1 << lb) - 1
    states = np.arange(1 << lb, dtype=np.uint32)
    neg = {}  # low mask -> where the product of its spins is -1
    for m in coef:
        if m & low not in neg:
            neg[m & low] = _parity(states & np.uint32(m & low))
    down = [((states >> j) & 1).astype(bool) for j in range(lb)]
    held = sum(1 << j for j, s in enumerate(hid) if row[s] < 0)
    blocks, e_held = [], None
    for hb in range(1 << (h - lb)):
        E = np.zeros(1 << lb, dtype=LD)
        for m, c in coef.items():
            if bin((m >> lb) & hb).count("1") & 1:
                c = -c
            E += np.where(neg[m & low], -c, c)
        if hb == held >> lb:
            e_held = E[held & low]
        mb = E.max()
        p = np.exp(E - mb)
        Z = p.sum()
        S = [Z - 2 * p[down[j]].sum() for j in range(lb)] + [-Z if (hb >> (j - lb)) & 1 else Z for j in range(lb, h)]
        blocks.append((mb, Z, S))
    M = max(b[0] for b in blocks)
    Z = sum(b[1] * np.exp(b[0] - M) for b in blocks)
    means = np.array([sum(b[2][j] * np.exp(b[0] - M) for b in blocks) / Z for j in range(h)], dtype=LD)
    log_w = M + np.log(Z)
    return means, log_w, e_held - log_w


def cond_exact_rows(terms, n, rows, hidden):
    """every row of `rows` [K, n] under one hidden set: (means [K, h], log_w [K], log_p [K]), long double"""
    out = [cond_exact(terms, n, r, hidden) for r in np.asarray(rows)]
    h = len(list(hidden))
    return (np.array([o[0] for o in out], dtype=LD).reshape(len(out), h), np.array([o[1] for o in out], dtype=LD),
            np.array([o[2] for o in out], dtype=LD))


def cond_exact_masked(terms, n, rows, mask):
    """every row under its own hidden set mask[k] (bool [K, n]): (means [K, n], an observed entry holding its evidence value; log_w [K];
    log_p [K]), long double"""
    rows, mask = np.asarray(rows), np.asarray(mask, dtype=bool)
    means = rows.astype(LD)
    log_w, log_p = np.zeros(len(rows), dtype=LD), np.zeros(len(rows), dtype=LD)
    for k, r in enumerate(rows):
        hid = np.flatnonzero(mask[k])
        m, log_w[k], log_p[k] = cond_exact(terms, n, r, hid)
        means[k, hid] = m
    return means, log_w, log_p


def energy(terms, row):
    """E(row) = sum_t w_t prod s, long double, with the contract's reductions"""
    return cond_exact(terms, len(row), row, [])[1]


def abs_weight(terms):
    terms = list(terms.items()) if isinstance(terms, dict) else list(terms)
    return float(sum(abs(w) for _, w in terms))


def tol(terms):
    """the project's tolerance of the exact enumerations (tests/test_gpu_exact.py): 1e-12 max(1, sum_t |w_t|), absolute"""
    return 1e-12 * max(1.0, abs_weight(terms))
