"""gml_model_exact on the device: exact log Z, means, pair correlations and query expectations by streaming enumeration, against brute
force in np.longdouble (tests/_exact_reference.py) and against closed forms.
Tolerance of log Z and of every expectation: 1e-12 max(1, sum_t |w_t|), absolute.  The a-priori error is about (c + log2 T) 2^-53 sum|w|
from the energy butterflies plus about 1e-13 from the sums: the project's standing 1e-12 scaled by the energy scale, more than 100
times that estimate."""
import itertools
import time

import numpy as np
import pytest

import gml_amd as gml
from _exact_reference import ExactModel, LD, abs_weight, chain_corr, chain_log_z, chain_model, dense_model

pytestmark = pytest.mark.gpu
_lib = gml._lib

_cache = {}


def tol(terms):
    return 1e-12 * max(1.0, abs_weight(terms))


def two_component_model(sb):
    """(terms, n): a dense component on spins 1 .. sb, a second one on the two spins after it"""
    terms = dense_model(range(1, sb + 1), seed=100 + sb, extra=8)
    terms.update({(sb + 1, sb + 2): 0.35, (sb + 1,): -0.2, (sb + 2,): 0.15})
    return terms, sb + 2


def queries_for(sb):
    """keys of orders 1 to 6 within the large component, one with a duplicated spin, the empty key, a fully cancelled one, and keys
    that span the two components"""
    rng = np.random.default_rng(sb)
    q = [(), (1, 1), (sb + 1, sb + 2, sb + 1), (1, sb + 1), (sb, sb + 2, sb + 1), (1,)]
    for k in range(2, 7):
        if k <= sb:
            key = tuple(int(v) for v in rng.choice(np.arange(1, sb + 1), size=k, replace=False))
            q += [key, key + (sb + 2,), key + key[:1]]
    return q


def reference(sb):
    """the brute-force model of two_component_model(sb) with its correlations, computed once"""
    if sb not in _cache:
        terms, n = two_component_model(sb)
        ref = ExactModel(terms, n)
        _cache[sb] = (terms, n, ref, ref.corr)
    return _cache[sb]


def check_model(sb, what):
    terms, n, ref, corr = reference(sb)
    q = queries_for(sb)
    log_z, m, C, e = _lib.model_exact(terms, n, queries=q, pairs=True)
    want = np.array([ref.expectation(k) for k in q], dtype=LD)
    errs = (abs(log_z - ref.log_z), np.abs(m - ref.mean).max(), np.abs(C - corr).max(), np.abs(e - want).max())
    print(f"{what}: sb = {sb}, sum|w| = {abs_weight(terms):.1f}, log Z = {log_z:.12f}; errors: log Z {float(errs[0]):.1e}, means "
          f"{float(errs[1]):.1e}, pairs {float(errs[2]):.1e}, queries {float(errs[3]):.1e}; tolerance {tol(terms):.1e}")
    assert all(np.isfinite(x).all() for x in (log_z, m, C, e))
    assert max(errs) <= tol(terms), errs
    assert np.array_equal(np.diag(C), np.ones(n)) and np.array_equal(C, C.T)
    assert e[0] == 1.0 and e[1] == 1.0  # the empty key and the fully cancelled one
    return log_z, m, C, e


class chunk_bits:
    """the test hook's chunk width for the body, the default again afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        assert _lib.lib().gml_test_exact_chunk_bits(self.c) >= 0

    def __exit__(self, *a):
        _lib.lib().gml_test_exact_chunk_bits(0)


# 1. against brute force: a partial chunk (1, 3, 11), exactly one chunk (12), two chunks (13), 64 chunks (18)
@pytest.mark.parametrize("sb", [1, 3, 11, 12, 13, 18])
def test_against_brute_force(sb):
    check_model(sb, "default chunk")


# 2. the chunk width changes the order of the sums, not the result beyond the tolerance
def test_chunk_width_invariance():
    got = {}
    for c in (4, 8, 0):
        with chunk_bits(c):
            got[c] = check_model(10, f"chunk bits {c or 'default'}")
    for c in (4, 8):
        assert abs(got[c][0] - got[0][0]) <= 2 * tol(reference(10)[0])


def test_many_chunks_per_group_against_brute_force():
    # 18 spins at 4 chunk bits: 2^14 chunks, 1024 groups of 16 chunks each; every low mask has more terms than one item holds
    with chunk_bits(4):
        check_model(18, "chunk bits 4")


def test_more_chunks_per_group_than_one_accumulator_takes():
    # a 24-spin chain at 2 chunk bits: 2^22 chunks, 4096 per group, four blocks of 1024 into the second accumulator
    terms, J = chain_model(list(range(1, 25)), seed=24)
    with chunk_bits(2):
        log_z, m, C, _ = _lib.model_exact(terms, 24, pairs=True)
    errs = (abs(log_z - chain_log_z(J)), np.abs(m).max(), np.abs(C - chain_corr(J)).max())
    print(f"24-spin chain, chunk bits 2: errors log Z {float(errs[0]):.1e}, means {float(errs[1]):.1e}, pairs {float(errs[2]):.1e}")
    assert max(errs) <= tol(terms), errs


def test_more_queries_than_one_window():
    # the 13-spin component: 13 + 78 moments and 1287 keys of order 5, two enumerations of at most 1023 expectations each
    terms, n, ref, _ = reference(13)
    q = list(itertools.combinations(range(1, 14), 5))
    log_z, m, C, e = _lib.model_exact(terms, n, queries=q, pairs=True)
    want = np.array([ref.expectation(k) for k in q], dtype=LD)
    assert len(q) == 1287 and np.abs(e - want).max() <= tol(terms) and abs(log_z - ref.log_z) <= tol(terms)
    assert log_z == _lib.model_exact(terms, n, pairs=False)[0]
    assert np.array_equal(gml.exact_moments(terms, terms=q), e)


# 3. components: log Z adds, expectations multiply
def test_components():
    n = 50
    terms = {(7,): 0.6}                                                  # a component of one spin
    terms.update(dense_model([2, 9, 30], seed=31, extra=1))              # of three
    terms.update(dense_model(range(10, 23), seed=32, extra=6))           # of thirteen
    chain, _ = chain_model(list(range(31, 51)), seed=33)                 # of twenty: a chain with fields and a few longer terms
    terms.update(chain)
    rng = np.random.default_rng(34)
    terms.update({(v,): float(rng.normal(scale=0.2)) for v in range(31, 51, 3)})
    terms.update({(31, 40, 50): 0.25, (33, 35, 44, 47): -0.3, (32, 36, 41, 45, 49): 0.2})
    terms[(7, 10)] = 0.0                                                 # a zero weight joins nothing
    terms[()] = -0.75                                                    # the empty key: a constant of log Z
    terms[(3, 3)] = 0.5                                                  # cancels to the empty key, and spin 3 stays free
    ref = ExactModel(terms, n)
    assert sorted(len(c.spins) for c in ref.comp) == [1] * 14 + [3, 13, 20]
    q = [(7, 2, 9), (10, 11, 31, 32), (7, 7), (1,), (1, 7), (2, 9, 30, 15, 16, 17, 40, 41), ()]
    log_z, m, C, e = _lib.model_exact(terms, n, queries=q, pairs=True)
    want = np.array([ref.expectation(k) for k in q], dtype=LD)
    errs = (abs(log_z - ref.log_z), np.abs(m - ref.mean).max(), np.abs(C - ref.corr).max(), np.abs(e - want).max())
    print(f"components: errors log Z {float(errs[0]):.1e}, means {float(errs[1]):.1e}, pairs {float(errs[2]):.1e}, queries "
          f"{float(errs[3]):.1e}; tolerance {tol(terms):.1e}")
    assert max(errs) <= tol(terms), errs
    # the product rules themselves: across components the product of the means, 1 on the diagonal, 0 for a free spin
    of = ref.of
    for i in range(n):
        for j in range(n):
            if of[i + 1] != of[j + 1]:
                assert C[i, j] == m[i] * m[j]
    free = [i for i in range(n) if len(ref.comp[of[i + 1]].spins) == 1 and i != 6]
    assert len(free) == 13 and np.all(m[free] == 0.0) and np.array_equal(np.diag(C), np.ones(n))
    assert e[2] == 1.0 and e[3] == 0.0 and e[4] == 0.0 and e[6] == 1.0
    assert abs(e[0] - m[6] * C[1, 8]) <= 1e-15


# 4. range: neither a shift by sum|w| nor an unshifted exp would do
@pytest.mark.parametrize("J", [-150.0, 150.0])
def test_range(J):
    terms = {k: J for k in itertools.combinations(range(1, 7), 2)}
    ref = ExactModel(terms, 6)
    if J < 0:
        assert abs(float(ref.log_z) - 452.9957322735) < 1e-9
    log_z, m, C, _ = _lib.model_exact(terms, 6, pairs=True)
    print(f"K6, J = {J}: log Z = {log_z!r}, reference {float(ref.log_z)!r}")
    assert np.isfinite(log_z) and np.isfinite(m).all() and np.isfinite(C).all()
    assert abs(log_z - ref.log_z) <= tol(terms) and np.abs(m - ref.mean).max() <= tol(terms) and np.abs(C - ref.corr).max() <= tol(terms)


# 5. beyond the sampler's table: one component of 30 spins
def test_open_chain_of_30_spins():
    terms, J = chain_model(list(range(1, 31)), seed=30)
    t0 = time.perf_counter()
    log_z, m, C, _ = _lib.model_exact(terms, 30, pairs=True)
    dt = time.perf_counter() - t0
    errs = (abs(log_z - chain_log_z(J)), np.abs(m).max(), np.abs(C - chain_corr(J)).max())
    print(f"30-spin chain: {dt:.3f} s; errors log Z {float(errs[0]):.1e}, means {float(errs[1]):.1e}, pairs {float(errs[2]):.1e}; "
          f"tolerance {tol(terms):.1e}")
    assert max(errs) <= tol(terms), errs
    with pytest.raises(gml.GMLError, match="limited to 22"):  # the sampler's own limit stays
        gml.Problem(terms=terms, n=30, num_samples=16)


# 6. the result is a function of the model: the same bits from every call
def test_reproducible_bits():
    terms, n = two_component_model(13)
    q = queries_for(13)
    a, b = _lib.model_exact(terms, n, queries=q), _lib.model_exact(terms, n, queries=q)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# 7. the exact sampler draws from the distribution whose moments these are
def test_tie_to_the_exact_sampler():
    rng = np.random.default_rng(12)
    A = np.triu(rng.normal(scale=0.25, size=(12, 12)), 1)
    A = A + A.T + np.diag(rng.normal(scale=0.2, size=12))
    N = 10 ** 6
    with gml.Problem(model=A, num_samples=N, seed=5) as p:
        sm, sC = p.moments()
    m, C = gml.exact_moments(A)
    print(f"sampler against exact moments: means {np.abs(sm - m).max():.2e}, pairs {np.abs(sC - C).max():.2e}, bound {6 / np.sqrt(N):.1e}")
    assert np.abs(sm - m).max() <= 6 / np.sqrt(N) and np.abs(sC - C).max() <= 6 / np.sqrt(N)  # Hoeffding: <= 2 e^-18 per moment
    only_m, none = gml.exact_moments(A, pairs=False)
    assert none is None and np.array_equal(only_m, m)


# 8. the front door
def test_front_door():
    terms, n, ref, _ = reference(11)
    lp = gml.log_partition(terms, gml.Exact())
    assert isinstance(lp, gml.LogPartition) and lp.stderr == 0.0 and np.isnan(lp.ess) and len(lp.log_weights) == 0
    assert abs(lp.log_z - ref.log_z) <= tol(terms)
    rng = np.random.default_rng(8)
    data = np.concatenate([rng.integers(1, 9, size=(40, 1)), rng.choice([-1, 1], size=(40, n))], axis=1).astype(np.float64)
    ll = gml.log_likelihood(data, terms, gml.Exact())
    with gml.Problem(data) as p:
        data_term = float(np.dot(list(terms.values()), p.term_moments(terms, raw=True).astype(np.float64))) / p.M
    assert ll.stderr == 0.0 and ll.data_term == data_term and ll.log_z == lp.log_z and ll.mean == data_term - lp.log_z
    assert abs(ll.mean - (LD(data_term) - ref.log_z)) <= tol(terms)
    assert gml.log_likelihood(data, terms, log_z=lp).mean == ll.mean
