"""gml_problem_moments / gml_problem_term_moments on the device: exact integer sums, compared with `==` against the numpy
restatement (tests/_moments_reference.py), independent of the handle's shape and creation route, tied to the RISE gradient at
Theta = 0 and to the enumerated expectations of a small model."""
import itertools

import numpy as np
import pytest

import gml_amd as gml
from _moments_reference import moments as ref_moments, split_histogram, term_sums as ref_term_sums
from conftest import load_csv

pytestmark = pytest.mark.gpu
_lib = gml._lib


def raw_moments(p):
    s1, s2 = p.moments(raw=True)
    assert s1.dtype == np.int64 and s2.dtype == np.int64 and s2.shape == (p.n, p.n)
    return s1, s2


def check_against_reference(p, S, c):
    r1, r2 = ref_moments(S, c)
    s1, s2 = raw_moments(p)
    assert np.array_equal(s1, r1)
    assert np.array_equal(s2, r2)
    only1, none = p.moments(pairs=False, raw=True)
    assert none is None and np.array_equal(only1, r1)


# 1. the golden sample files, both ingest routes
@pytest.mark.parametrize("ingest", ["host", "device"])
@pytest.mark.parametrize("name", ["a", "b", "c", "mvt"])
def test_golden_histograms(name, ingest):
    samples = load_csv(f"{name}_samples.csv")
    S, c = split_histogram(samples)
    n = S.shape[1]
    keys = [k for q in (1, 2, 3) for k in itertools.combinations(range(n), q)]
    with gml.Problem(samples=samples, ingest=ingest) as p:
        check_against_reference(p, S, c)
        got = p.term_moments([tuple(i + 1 for i in k) for k in keys], raw=True)
        m, C = p.moments()
        assert np.array_equal(m, ref_moments(S, c)[0] / c.sum()) and np.array_equal(C, ref_moments(S, c)[1] / c.sum())
    assert np.array_equal(got, ref_term_sums(S, c, keys))
    fm, fC = gml.moments(samples)  # the front door builds and closes a handle
    assert np.array_equal(fm, m) and np.array_equal(fC, C)
    assert np.array_equal(gml.moments(samples, terms=[(1, 2), ()], raw=True), ref_term_sums(S, c, [(0, 1), ()]))


# 2. random rows with random integer counts, every edge of the tiling
NS = [1, 2, 31, 33, 64, 65, 257, 1024]
KS = [1, 31, 1023, 1025, 50001]
COUNTS = ["ones", "sevens", "small", "to_2_30", "to_2_38"]


def random_counts(kind, K, rng):
    if kind == "ones":
        return np.ones(K)
    if kind == "sevens":
        return np.full(K, 7.0)
    hi = {"small": 6, "to_2_30": 1 << 30, "to_2_38": 1 << 38}[kind]
    c = rng.integers(0, hi, size=K, endpoint=True).astype(np.float64)
    c[rng.integers(K)] = float(hi)  # the top bit plane is in use
    return c


# counts up to 2^38 only for K <= 1025: at K = 50 001 their sum would pass the contract's 2^50
CASES = [(n, K, kind) for n in NS for K in KS for kind in COUNTS if kind != "to_2_38" or K <= 1025]


@pytest.mark.parametrize("n,K,kind", CASES)
def test_random_histograms(n, K, kind):
    rng = np.random.default_rng([n, K, COUNTS.index(kind)])
    S = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    c = random_counts(kind, K, rng)
    assert c.sum() < 2.0 ** (49 if kind == "to_2_38" else 46)
    with gml.Problem(spins=S, counts=None if kind == "ones" else c) as p:
        assert p.M == c.sum()
        check_against_reference(p, S, c)
        assert np.array_equal(p.counts(), c)  # integer counts come back exactly


def test_m_above_2_50_is_unsupported():
    S = np.array([[1, -1], [-1, -1], [1, 1]], dtype=np.int8)
    with gml.Problem(spins=S, counts=np.array([2.0 ** 50, 1.0, 1.0])) as p:
        with pytest.raises(gml.GMLError) as e:
            p.moments()
        assert e.value.code == _lib.GML_EUNSUPPORTED and "2^50" in str(e.value)
        with pytest.raises(gml.GMLError) as e:
            p.term_moments([(1, 2)])
        assert e.value.code == _lib.GML_EUNSUPPORTED
    with gml.Problem(spins=S, counts=np.array([2.0 ** 50 - 2, 1.0, 1.0])) as p:  # M = 2^50 itself is inside
        check_against_reference(p, S, np.array([2.0 ** 50 - 2, 1.0, 1.0]))


# 3. chain handles
def dense_model(n, seed):
    rng = np.random.default_rng(seed)
    J = np.triu(rng.normal(scale=0.7 / np.sqrt(n), size=(n, n)), 1)
    J = J + J.T
    J[np.diag_indices(n)] = rng.normal(scale=0.2, size=n)
    return J


def test_chain_handle_n_1024():
    J = dense_model(1024, 1)
    with gml.Problem(model=J, num_samples=4096, burn_in=3, thin=1, samples_per_chain=8, seed=2) as p:
        S = p.spins()
        check_against_reference(p, S, np.ones(p.K))


POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def test_chain_handle_n_16384():
    n = 16384
    J = dense_model(n, 3)
    with gml.Problem(model=J, num_samples=2048, burn_in=1, thin=1, samples_per_chain=8, seed=4) as p:
        del J
        s1, s2 = raw_moments(p)
        bits = p.sign_bits().view(np.uint8)  # [n][bytes]: bit set <=> -1; padding bits are zero
        M = int(p.M)

    def pair(i, j):
        return M - 2 * POP8[bits[i] ^ bits[j]].sum(axis=-1)

    rng = np.random.default_rng(5)
    ii, jj = rng.integers(n, size=4096), rng.integers(n, size=4096)
    assert np.array_equal(s2[ii, jj], pair(ii, jj))
    assert np.array_equal(np.diagonal(s2), np.full(n, M))
    assert np.array_equal(s2[0], pair(np.zeros(n, dtype=np.int64), np.arange(n)))
    assert np.array_equal(s2[:, 0], s2[0])
    assert np.array_equal(s1, M - 2 * POP8[bits].sum(axis=1))


# 4. independence of the handle's shape and of the call
def test_independent_of_order_node_range_and_histogramming():
    n, N = 12, 60000
    J = dense_model(n, 7)
    keys = [(1,), (2, 5), (1, 2, 3), (3, 7, 9, 12), ()]
    results = []
    for kw in (dict(), dict(node_range=(3, 7)), dict(order=3), dict(histogram=True)):
        with gml.Problem(model=J, num_samples=N, seed=9, **kw) as p:
            assert (p.K < N) == bool(kw.get("histogram"))
            a = raw_moments(p) + (p.term_moments(keys, raw=True),)
            b = raw_moments(p) + (p.term_moments(keys, raw=True),)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))  # two calls on one handle
            results.append(a)
            if not kw:
                S = p.spins()
    for r in results[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(results[0], r))
    r1, r2 = ref_moments(S, np.ones(N))
    assert np.array_equal(results[0][0], r1) and np.array_equal(results[0][1], r2)


# 5. term moments
@pytest.mark.parametrize("weighted", [False, True])
def test_term_moments(weighted):
    n, K = 40, 3000
    rng = np.random.default_rng(11 + weighted)
    S = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    c = rng.integers(1, 1000, size=K).astype(np.float64) if weighted else np.ones(K)
    keys3 = [tuple(rng.choice(n, size=3, replace=False)) for _ in range(200)]
    keys5 = [tuple(rng.choice(n, size=5, replace=False)) for _ in range(200)]
    odd = [(4, 4), (1, 7, 1), (2, 3, 2, 3), (5, 5, 5), (), (9,), (0, 39)]
    keys = keys3 + keys5 + odd
    want = ref_term_sums(S, c, keys)
    with gml.Problem(spins=S, counts=c if weighted else None) as p:
        s1, s2 = raw_moments(p)
        got = p.term_moments([tuple(int(i) + 1 for i in k) for k in keys], raw=True)
        assert np.array_equal(got, want)
        assert got[len(keys3) + len(keys5) + 4] == int(c.sum())  # the empty key
        assert np.array_equal(p.term_moments([()]), np.array([1.0]))
        # key_stride larger than the longest key, through the C call
        wide = np.full((len(keys), 9), -1, dtype=np.int32)
        for t, k in enumerate(keys):
            wide[t, 9 - len(k):] = k
        sums = np.zeros(len(keys), dtype=np.int64)
        _lib.check(_lib.lib().gml_problem_term_moments(p._h, _lib._ptr(wide), 9, len(keys), _lib._ptr(sums)))
        assert np.array_equal(sums, want)
        _lib.check(_lib.lib().gml_problem_term_moments(p._h, _lib._ptr(wide), 9, 0, _lib._ptr(sums)))  # nterms = 0: a no-op
        # length-1 and length-2 keys are sum1 and the entries of sum2
        assert np.array_equal(p.term_moments([(i + 1,) for i in range(n)], raw=True), s1)
        pairs = list(itertools.combinations(range(n), 2))
        got2 = p.term_moments([(i + 1, j + 1) for i, j in pairs], raw=True)
        assert np.array_equal(got2, np.array([s2[i, j] for i, j in pairs]))
        # a TermArray: every key of an order-3 model on the first spins, window by window
        ta = gml.factor_graph.TermArray(n, 3, True, np.zeros(_lib.terms_count(n, 3, True)))
        allkeys = [k for q in (1, 2, 3) for k in itertools.combinations(range(n), q)]
        assert np.array_equal(p.term_moments(ta, raw=True), ref_term_sums(S, c, allkeys))
        fg = gml.FactorGraph(3, n, "spin", {(1, 2, 3): 0.1, (4,): 0.2})
        assert np.array_equal(p.term_moments(fg, raw=True), ref_term_sums(S, c, [tuple(i - 1 for i in k) for k in fg.terms]))


# 6. the tie to the operator: the RISE gradient at Theta = 0 is minus the moments
def test_rise_gradient_at_zero():
    n, K = 48, 20000
    rng = np.random.default_rng(13)
    S = rng.choice(np.array([-1, 1], dtype=np.int8), size=(K, n))
    with gml.Problem(spins=S) as p:
        s1, s2 = raw_moments(p)
        f, g = p.objgrad("RISE", np.arange(n), np.zeros((n, n)), precision="i8w")
        M = p.M
    assert np.array_equal(f, np.ones(n))
    want = -s2 / M
    want[np.diag_indices(n)] = -s1 / M  # row u: entry u is the field, entry j != u the coupling (:191-208)
    err = np.abs(g - want).max()
    print("max |grad + moments| =", err)
    assert err <= 1e-12


# 7. statistical closure: 1e6 exact draws of a 9-spin model against the enumerated expectations
def test_moments_of_exact_samples_match_enumeration():
    n, N = 9, 1000000
    J = dense_model(n, 17) * 2.0
    states = ((np.arange(2 ** n)[:, None] >> np.arange(n)) & 1) * 2 - 1  # int_to_spin (sampling.jl:11-14)
    sf = states.astype(float)
    A = J - np.diag(np.diag(J))
    en = 0.5 * ((sf @ A) * sf).sum(1) + sf @ np.diag(J)  # weigh_proba (sampling.jl:26-30)
    pr = np.exp(en - en.max())
    pr /= pr.sum()
    with gml.Problem(model=J, num_samples=N, seed=21, histogram=True) as p:
        assert p.K <= 2 ** n and p.M == N
        m, C = p.moments()
    em, eC = pr @ sf, sf.T @ (pr[:, None] * sf)
    iu = np.triu_indices(n, 1)
    dev = np.concatenate([np.abs(m - em), np.abs(C[iu] - eC[iu])])
    assert dev.shape == (45,)
    print("largest deviation in units of 1/sqrt(N):", dev.max() * np.sqrt(N))
    assert dev.max() <= 6.0 / np.sqrt(N)  # each is a mean of N independent +-1 values: sd <= 1/sqrt(N)


# 8. errors and device memory
def test_errors():
    S = np.array([[1, -1, 1], [-1, -1, 1], [1, 1, -1]], dtype=np.int8)
    with gml.Problem(spins=S, counts=np.array([1.0, 2.5, 3.0])) as p:
        for call in (p.moments, lambda: p.term_moments([(1, 2)])):
            with pytest.raises(gml.GMLError) as e:
                call()
            assert e.value.code == _lib.GML_EUNSUPPORTED and "fractional" in str(e.value)
        assert np.allclose(p.counts(), [1.0, 2.5, 3.0], atol=1e-6, rtol=0)
    with gml.Problem(samples=np.array([[1.0, 1, -1], [2.5, -1, -1]]), ingest="device") as p:  # the other creation route
        with pytest.raises(gml.GMLError) as e:
            p.moments()
        assert e.value.code == _lib.GML_EUNSUPPORTED
    with gml.Problem(spins=S) as p:
        with pytest.raises(gml.GMLError) as e:
            p.term_moments([(1, 2), (2,), (1, 4)])
        assert e.value.code == _lib.GML_EINVAL and "term 2" in str(e.value)
        keys = np.array([[0, 1]], dtype=np.int32)
        sums = np.zeros(1, dtype=np.int64)
        L = _lib.lib()
        assert L.gml_problem_term_moments(p._h, _lib._ptr(keys), 0, 1, _lib._ptr(sums)) == _lib.GML_EINVAL
        assert L.gml_problem_term_moments(p._h, _lib._ptr(keys), 2, -1, _lib._ptr(sums)) == _lib.GML_EINVAL
        assert L.gml_problem_term_moments(p._h, None, 2, 1, _lib._ptr(sums)) == _lib.GML_EINVAL
        assert L.gml_problem_term_moments(p._h, _lib._ptr(keys), 2, 1, None) == _lib.GML_EINVAL
        assert L.gml_problem_moments(p._h, None, None) == _lib.GML_EINVAL


def test_device_memory_returns():
    import torch
    rng = np.random.default_rng(3)
    S = rng.choice(np.array([-1, 1], dtype=np.int8), size=(70000, 300))
    keys = [tuple(int(i) + 1 for i in rng.choice(300, size=3, replace=False)) for _ in range(5000)]
    for counts in (None, rng.integers(1, 50, size=70000).astype(np.float64)):
        with gml.Problem(spins=S, counts=counts) as p:
            torch.cuda.synchronize()
            _lib.trim_cache()
            free0 = torch.cuda.mem_get_info()[0]
            first = p.moments(raw=True) + (p.term_moments(keys, raw=True),)
            for _ in range(19):
                again = p.moments(raw=True) + (p.term_moments(keys, raw=True),)
            assert all(np.array_equal(x, y) for x, y in zip(first, again))
            _lib.trim_cache()
            free1 = torch.cuda.mem_get_info()[0]
            print("free bytes before / after:", free0, free1)
            assert free1 == free0
