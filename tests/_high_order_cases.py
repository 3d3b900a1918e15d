"""Sample sets for the tests of interaction orders 5 to 8 (tests/test_gpu_high_order.py) and for the samplers: histograms over ALL 2^n states of a model
with true terms of every size up to the order, enumerated in numpy.  iid spins would leave an l1 optimum almost empty and test
nothing; here every size of key carries a coupling of about 0.3.

(n, order) are those of the shapes H5 .. H8, E7, E3 of tests/_f64_pass_reference.py; the samples are not (those are iid)."""
import numpy as np

import _f64_pass_reference as F

DRAWS = 1000000


def true_terms(n, order, seed):
    """{0-based sorted tuple: weight}: two terms of every size 1 .. min(order, n) where the size has two subsets (one otherwise),
    |weight| in [0.25, 0.35], signs mixed"""
    rng = np.random.default_rng(seed)
    terms = {}
    for q in range(1, min(order, n) + 1):
        for _ in range(2):
            key = tuple(sorted(int(i) for i in rng.choice(n, size=q, replace=False)))
            terms[key] = float(rng.uniform(0.25, 0.35) * rng.choice([-1.0, 1.0]))
    return terms


def all_states(n):
    """int8 [2^n][n]: state k has spin i = -1 where bit i of k is set"""
    k = np.arange(1 << n)[:, None]
    return np.where((k >> np.arange(n)[None, :]) & 1, -1, 1).astype(np.int8)


def histogram(name, seed=0, draws=DRAWS):
    """(spins int8 [K][n], counts float64 [K], terms): DRAWS multinomial draws from p(s) ~ exp(sum_t w_t prod_{i in t} s_i) over the
    2^n states; the states never drawn are left out"""
    n, order = F.SHAPES[name][:2]
    terms = true_terms(n, order, 1000 + seed + 7 * n + order)
    S = all_states(n)
    E = np.zeros(len(S))
    for key, w in terms.items():
        E += w * S[:, list(key)].astype(np.float64).prod(axis=1)
    pr = np.exp(E - E.max())
    pr /= pr.sum()
    c = np.random.default_rng(2000 + seed + n).multinomial(draws, pr).astype(np.float64)
    keep = c > 0
    return S[keep], c[keep], terms


def hist_array(spins, counts):
    """the reference's histogram layout: the count, then the spins"""
    return np.concatenate([counts[:, None], spins.astype(np.float64)], axis=1)


def wide_terms(n, seed, spins=None, scale=0.3, per_size=5, fields=True):
    """{1-based key: weight} for the samplers: per_size terms of each of 5, 6, 7 and 8 distinct spins among `spins` (default: all of
    1 .. n), keys not ascending, and keys that name a spin twice -- (i, i, a .. e) is the 5-spin term (a .. e), (i, a .. f, i) the
    6-spin term (a .. f), (i, j, i, j, a) the field of a -- so that cancellation happens next to the widest keys; a field on
    every second spin"""
    rng = np.random.default_rng(seed)
    live = np.arange(1, n + 1) if spins is None else np.asarray(spins)
    pick = lambda q: [int(v) for v in rng.choice(live, q, replace=False)]  # noqa: E731
    terms = {}
    for q in (5, 6, 7, 8):
        for _ in range(per_size):
            terms[tuple(pick(q))] = float(rng.normal(scale=scale))
    for _ in range(3):
        k = pick(6)
        terms[(k[0], k[0]) + tuple(k[1:])] = float(rng.normal(scale=scale))
        k = pick(7)
        terms[(k[0],) + tuple(k[1:]) + (k[0],)] = float(rng.normal(scale=scale))
        k = pick(3)
        terms[(k[0], k[1], k[0], k[1], k[2])] = float(rng.normal(scale=scale))
    if fields:
        for i in live[::2]:
            terms.setdefault((int(i),), float(rng.normal(scale=0.2)))
    return terms
