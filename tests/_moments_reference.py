"""numpy restatement of gml_problem_moments / gml_problem_term_moments (include/gml.h): the exact integer sums over a weighted
histogram, computed in float64 where every partial sum is an integer below 2^53 (asserted), returned as int64."""
import numpy as np

LIMIT = float(1 << 53)


def _check(c):
    c = np.asarray(c, dtype=np.float64)
    assert np.all(c == np.rint(c)) and np.all(c >= 0), "counts must be non-negative integers"
    # every entry of every product below is a sum of +-c_k: its partial sums are integers bounded by sum_k c_k
    assert float(c.sum()) < LIMIT, "sum of counts must stay below 2^53"
    return c


def moments(S, c):
    """S [K, n] of +-1, c [K] integer counts -> (sum1 [n], sum2 [n, n]) int64: c @ S and S' diag(c) S"""
    S = np.asarray(S, dtype=np.float64)
    c = _check(c)
    assert S.ndim == 2 and S.shape[0] == c.shape[0] and np.all(np.abs(S) == 1.0)
    sum1 = c @ S
    sum2 = S.T @ (c[:, None] * S)
    return sum1.astype(np.int64), sum2.astype(np.int64)


def term_sums(S, c, keys):
    """sums[t] = c @ prod(S[:, key t]) for 0-based keys (iterables of spins; -1 = unused slot; a repeated spin is multiplied
    twice, i.e. cancels; the empty key gives M)"""
    S = np.asarray(S, dtype=np.float64)
    c = _check(c)
    out = np.zeros(len(keys), dtype=np.int64)
    for t, key in enumerate(keys):
        prod = np.ones(S.shape[0])
        for i in key:
            if i >= 0:
                prod = prod * S[:, int(i)]
        out[t] = np.int64(c @ prod)
    return out


def split_histogram(samples):
    """(S, c) of a K x (1 + n) histogram matrix"""
    s = np.asarray(samples, dtype=np.float64)
    return s[:, 1:], s[:, 0]
